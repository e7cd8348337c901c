// tk_kat_bits.h - TEST SUPPORT: one known-answer item of the block syntax (tk_bits.h) run by one team, every form the engine has of it.  Shared by the device
// entry points thor_hip_kat_coeff_syntax / thor_hip_kat_block_syntax (hip_kat.h) and their host twin (tests/hostsim/kat_host_bits.cpp), so that both builds are
// driven the same way.  Known answers: the reference's put_vlc (enc/putvlc.c:73-160), write_mv (enc/write_bits.c:123-143), write_coeff (:145-241),
// write_super_mode (:257-358) and write_block (:360-600), recorded by tests/golden/gen_kat9.py.
#pragma once
#include "tk_bits.h"

namespace tk {
// Parameter row of a block-syntax item: 0 kind (0 write_block, 1 write_super_mode, 2 one put_vlc codeword: table [2], symbol [3], 3 write_mv of mv0[0] against
// mvp), 1 split_flag, 2 frame_type, 3 num_ref, 4 enable_bipred, 5 interp_ref, 6 max_pb_part, 7 max_tb_part, 8 num_intra_modes, 9 size, 10 encode_this_size,
// 11 ctx_index, 12 ctx_cbp, 13 num_skip, 14 num_merge, 15 mvp.x, 16 mvp.y, 17 mode, 18 intra_mode, 19 skip_idx, 20 pb_part, 21 ref0, 22 ref1, 23 dir, 24 tb_param,
// 25 tb_split, 26..28 cbp y / u / v, 29..36 mv0[4] (x, y), 37..44 mv1[4], 45..56 the coefficient-pool index of luma TU 0..3, U 0..3, V 0..3 (-1: none; the
// callers resolve them into the coefficient buffers).
// Result row: 0 bs_block_head_t<false>, 1 / 2 bs_block_t<false, SP_LDS / SP_GLOBAL> without ybits, 3 / 4 the same with ybits filled the way tk_block_rd.h's
// prune_after_luma fills them, 5 / 6 length and ovf of the cooperative emission (every lane, store on lane 0), 7 / 8 of the emission by lane 0 alone, 9 unused.
// -1: not applicable (SP_LDS with chroma buffers that only exist in global memory: tb-split blocks of 64 and 128).  Kinds 1..3: 1 the counting instance
// (E = false), 3 the emitting instance with emit == 0 (how the quadtree walk counts a split flag), 5..8 as above.
enum { kKatBlPar = 57, kKatBlOut = 10 };
// Parameter row of a coefficient item: size, type, start bit, capacity in bits.  Result row: 0 / 1 coeff_bits_team<SP_LDS / SP_GLOBAL>, 2 / 3 final pos and
// ovf of bs_coeff by lane 0 alone between bs_open / bs_close, 4 / 5 of bs_coeff_team by every lane (store on lane 0).
enum { kKatCoPar = 4, kKatCoOut = 6 };

TK_DEV void kat_unpack(const int* q, SynCtx& s, BlkParam& p) {
  s.frame_type = q[2]; s.num_ref = q[3]; s.enable_bipred = q[4]; s.interp_ref = q[5]; s.max_pb_part = q[6]; s.max_tb_part = q[7]; s.num_intra_modes = q[8];
  s.size = q[9]; s.encode_this_size = q[10]; s.ctx_index = q[11]; s.ctx_cbp = q[12]; s.num_skip = q[13]; s.num_merge = q[14]; s.mvp = mk_mv(q[15], q[16]);
  p.mode = (int8_t)q[17]; p.intra_mode = (int8_t)q[18]; p.skip_idx = (int8_t)q[19]; p.pb_part = (int8_t)q[20]; p.ref0 = (int8_t)q[21]; p.ref1 = (int8_t)q[22];
  p.dir = (int8_t)q[23]; p.tb_param = (int8_t)q[24]; p.tb_split = (int8_t)q[25]; p.cbp_y = (uint8_t)q[26]; p.cbp_u = (uint8_t)q[27]; p.cbp_v = (uint8_t)q[28];
  for (int k = 0; k < 4; k++) { p.mv0[k] = mk_mv(q[29 + 2 * k], q[30 + 2 * k]); p.mv1[k] = mk_mv(q[37 + 2 * k], q[38 + 2 * k]); }
}
TK_DEV BitSink kat_sink(uint32_t* buf, int pos, int cap, int emit, int store) {
  BitSink b;
  b.buf = buf; b.pos = pos; b.cap = cap; b.emit = emit; b.ovf = 0; b.store = store;
  return b;
}

// lc: the coefficients in the team's workspace (LDS on the device), gc: the same in global memory.  Every lane of the team calls.
TK_DEV void kat_coeff_item(const Team t, const int* q, const int16_t* lc, const int16_t* gc, uint32_t* buf1, uint32_t* bufT, int* out) {
  const int size = q[0], type = q[1];
  const int n_lds = coeff_bits_team<SP_LDS>(t, lc, size, type);
  const int n_glb = coeff_bits_team<SP_GLOBAL>(t, gc, size, type);
  BitSink a = kat_sink(buf1, q[2], q[3], 1, 1);
  if (t.rank == 0) {
    bs_open(a);
    bs_coeff(a, gc, size, type);
    bs_close(a);
  }
  BitSink b = kat_sink(bufT, q[2], q[3], 1, t.rank == 0);
  bs_open(b);
  bs_coeff_team(b, t, lc, size, type);
  bs_close(b);
  if (t.rank == 0) { out[0] = n_lds; out[1] = n_glb; out[2] = a.pos; out[3] = a.ovf; out[4] = b.pos; out[5] = b.ovf; }
}

// ly / lu / lv: the coefficient buffers in the team's workspace (lu == nullptr: the chroma buffers of this item only exist in global memory), gy / gu / gv: all
// three in global memory; TU t of a tb-split block at t * qs^2 (tk_bits.h).  bufC / buf1: cap bits each.  Every lane of the team calls.
TK_DEV void kat_block_item(const Team t, const int* q, const int16_t* ly, const int16_t* lu, const int16_t* lv, const int16_t* gy, const int16_t* gu,
                           const int16_t* gv, int cap, uint32_t* bufC, uint32_t* buf1, int* out) {
  SynCtx s;
  BlkParam p;
  kat_unpack(q, s, p);
  const int kind = q[0], split_flag = q[1];
  int o[kKatBlOut];
  for (int k = 0; k < kKatBlOut; k++) o[k] = -1;
  const BitSink cnt = kat_sink(nullptr, 0, 0, 0, 1);
  BitSink wc = kat_sink(bufC, 0, cap, 1, t.rank == 0), w1 = kat_sink(buf1, 0, cap, 1, 1);
  if (kind == 0) {
    BitSink h = cnt;
    bs_block_head_t<false>(h, uniform_syn(s), uniform_blk(p));
    o[0] = h.pos;
    // the luma lengths as prune_after_luma (tk_block_rd.h) leaves them in PruneCtx::ybits
    int yb[4] = {0, 0, 0, 0};
    const int coeff_type = (p.mode == M_INTRA) << 1;
    if (p.mode != M_SKIP) {
      if (!p.tb_split) yb[0] = p.cbp_y ? coeff_bits_team<SP_LDS>(t, ly, s.size, coeff_type) : 0;
      else {
        const int qy = s.size / 2 < kMaxQuant ? s.size / 2 : kMaxQuant;
        for (int tu = 0; tu < 4; tu++) yb[tu] = ((p.cbp_y >> (3 - tu)) & 1) ? coeff_bits_team<SP_LDS>(t, ly + tu * qy * qy, s.size / 2, coeff_type) : 0;
      }
    }
    BitSink c;
    if (lu) {
      c = cnt; o[1] = bs_block_t<false, SP_LDS>(c, s, p, ly, lu, lv, &t, nullptr);
      c = cnt; o[3] = bs_block_t<false, SP_LDS>(c, s, p, ly, lu, lv, &t, yb);
    }
    c = cnt; o[2] = bs_block_t<false, SP_GLOBAL>(c, s, p, ly, gu, gv, &t, nullptr);
    c = cnt; o[4] = bs_block_t<false, SP_GLOBAL>(c, s, p, ly, gu, gv, &t, yb);
    bs_open(wc);
    bs_block_t<true>(wc, s, p, ly, lu ? lu : gu, lu ? lv : gv, &t, nullptr);
    bs_close(wc);
    if (t.rank == 0) {
      bs_open(w1);
      bs_block_t<true>(w1, s, p, gy, gu, gv, nullptr, nullptr);
      bs_close(w1);
    }
  } else {
    BitSink c = cnt, e = kat_sink(nullptr, 0, 0, 0, 1);
    bs_open(wc);
    if (t.rank == 0) bs_open(w1);
    if (kind == 1) {
      bs_super_mode_t<false>(c, s, p.mode, p.ref0, split_flag);
      bs_super_mode(e, s, p.mode, p.ref0, split_flag);
      bs_super_mode(wc, s, p.mode, p.ref0, split_flag);
      if (t.rank == 0) bs_super_mode(w1, s, p.mode, p.ref0, split_flag);
    } else if (kind == 2) {
      bs_vlc_t<false>(c, q[2], (uint32_t)q[3]);
      e.pos = vlc_len(q[2], (uint32_t)q[3]);
      bs_vlc(wc, q[2], (uint32_t)q[3]);
      if (t.rank == 0) bs_vlc(w1, q[2], (uint32_t)q[3]);
    } else {
      bs_mv_t<false>(c, p.mv0[0], s.mvp);
      bs_mv_t<true>(e, p.mv0[0], s.mvp);
      bs_mv_t<true>(wc, p.mv0[0], s.mvp);
      if (t.rank == 0) bs_mv_t<true>(w1, p.mv0[0], s.mvp);
    }
    bs_close(wc);
    if (t.rank == 0) bs_close(w1);
    o[1] = c.pos; o[3] = e.pos;
  }
  o[5] = wc.pos; o[6] = wc.ovf;
  if (t.rank == 0) {
    o[7] = w1.pos; o[8] = w1.ovf;
    for (int k = 0; k < kKatBlOut; k++) out[k] = o[k];
  }
}
// Host side of both callers: checks one parameter row and resolves its pool indices (pool: npool blocks of 256 coefficients, row-major qs x qs in the first
// qs^2 entries) into the three coefficient buffers of the item (dst: 3 x 1024, the engine's layout).  Returns 0, or 1 for a row the syntax functions must not
// be given (they index the buffers by size, tb_split and the cbp masks).
static inline int kat_block_resolve(const int* q, const int16_t* pool, int npool, int16_t* dst) {
  for (int k = 0; k < 3 * 1024; k++) dst[k] = 0;
  if (q[0] < 0 || q[0] > 3) return 1;
  if (q[0] == 2) {
    const int n = q[2];
    if (!((n >= 0 && n <= 8) || (n >= 10 && n <= 18)) || q[3] < 0) return 1;
    return 0;
  }
  const int size = q[9], tb_split = q[25];
  if (size < 8 || size > 128 || (size & (size - 1)) || q[17] < 0 || q[17] > 4 || q[20] < 0 || q[20] > 3 || (tb_split & ~1) || (q[1] & ~1) || (q[10] & ~1)) return 1;
  for (int k = 26; k <= 28; k++) if (q[k] < 0 || q[k] > (tb_split ? 15 : 1)) return 1;
  for (int k = 15; k <= 16; k++) if (q[k] < -32768 || q[k] > 32767) return 1;
  for (int k = 29; k <= 44; k++) if (q[k] < -32768 || q[k] > 32767) return 1;
  if (q[0] != 0) return 0;
  const int size_uv = size >> 1;
  for (int pl = 0; pl < 3; pl++) {
    const int split = tb_split && (pl == 0 || size_uv > 4);
    const int tu = split ? (pl ? size_uv : size) / 2 : (pl ? size_uv : size);
    const int qs = tu < kMaxQuant ? tu : kMaxQuant;
    for (int t = 0; t < 4; t++) {
      const int idx = q[45 + 4 * pl + t];
      if (idx < 0) continue;
      if (idx >= npool || (!split && t > 0)) return 1;
      for (int k = 0; k < qs * qs; k++) dst[pl * 1024 + t * qs * qs + k] = pool[(size_t)idx * 256 + k];
    }
  }
  return 0;
}
static inline int kat_coeff_check(const int* q, int words) {
  const int size = q[0];
  return size < 4 || size > 128 || (size & (size - 1)) || (q[1] & ~3) || q[2] < 0 || q[2] > 63 || q[3] < 0 || q[3] > words * 32;
}
}  // namespace tk
