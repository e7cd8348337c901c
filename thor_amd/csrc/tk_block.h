// tk_block.h - the per-superblock decision engine: quadtree recursion, early skip, RDO trials,
// final encode (recon + cell state + bit emission).
// Specification followed: enc/encode_block.c:2401-2566 (process_block), :1835-2121
// (mode_decision_rdo), :1340-1514 (encode_block), :1100-1338 (encode_and_reconstruct_*),
// :1679-1833 (search_bipred_prediction_params), :1033-1098 (search_inter_prediction_params),
// :2123-2392 (early skip), :916-926 (cost_calc), :1568-1613 (copy_deblock_data);
// common/inter_prediction.c:413-834 (get_mv_pred / get_mv_merge / get_mv_skip);
// common/common_block.c:283-309 (find_block_contexts), :347-428 (improve_uv_prediction);
// common/common_block.h:52-95 (availability).
#pragma once
// The parts below the superblock level, in dependency order (definition order inside namespace tk is the order of the code
// object); the superblock level itself - early skip, final_encode, process_sb - follows here.
#include "tk_block_ws.h"
#include "tk_block_ctx.h"
#include "tk_block_rd.h"
#include "tk_block_search.h"
#include "tk_block_md.h"
#include "tk_block_queue.h"

namespace tk {

// ---------------------------------------------------------------------------------
// Early skip (encode_block.c:2123-2392)
// ---------------------------------------------------------------------------------
template <typename PIX, int SP>
TK_DEV int early_skip_sub(const Team t, JobR<PIX> J, WsP<PIX> ws, const PIX* org_, int ostride,
                          const PIX* pred_, int pstride, int size, int qp, float thr) {
  const auto org = spc<SP>(org_);
  const auto pred = spc<SP>(pred_);
  const auto xin = ldsc(ws->xfp->in);
  const auto xcoef = ldsc(ws->xfp->coef);
  // luma: 2x2 average + (N/2) transform (size > 4 always here), threshold 0.5*thr
  const int bd = J.cfg.bitdepth;
  const int s2 = size / 2;
  for (int k = t.rank; k < s2 * s2; k += t.size) {
    int i, j;
    split2(mk_pow2(s2), k, i, j);
    int a = (int16_t)((int)org[(2 * i) * ostride + 2 * j] - (int)pred[(2 * i) * pstride + 2 * j]);
    int b = (int16_t)((int)org[(2 * i) * ostride + 2 * j + 1] - (int)pred[(2 * i) * pstride + 2 * j + 1]);
    int cc = (int16_t)((int)org[(2 * i + 1) * ostride + 2 * j] - (int)pred[(2 * i + 1) * pstride + 2 * j]);
    int d = (int16_t)((int)org[(2 * i + 1) * ostride + 2 * j + 1] - (int)pred[(2 * i + 1) * pstride + 2 * j + 1]);
    xin[i * s2 + j] = (int16_t)((a + b + cc + d + 2) >> 2);  // row-major (fwd_core layout)
  }
  t.sync();
  fwd_transform_block(t, ws->xfp, s2, bd);
  const int shift2 = 21 - ilog2(s2) + qp / 6;
  const double fql = (double)(1 << shift2) / (double)quant_scale(qp % 6);
  const double rel = 0.5 * thr;  // float -> double promotion as in the reference
  const int threshold = (int)(rel * fql);
  int f = 0;
  for (int k = t.rank; k < s2 * s2; k += t.size)
    if (iabs((int)xcoef[k]) > threshold) f = 1;
  const int r = team_ballot(t, f) != 0ull;   // any lane: no LDS flag round trip
  t.sync();
  return r;
}

template <typename PIX, int SP>
TK_DEV int early_skip_subC(const Team t, JobR<PIX> J, WsP<PIX> ws, const PIX* org_, int ostride,
                           const PIX* pred_, int pstride, int size, int qp, float thr) {
  const auto org = spc<SP>(org_);
  const auto pred = spc<SP>(pred_);
  const int shift2 = 21 - 5 + qp / 6;
  const double fql = (double)(1 << shift2) / (double)quant_scale(qp % 6);
  const int threshold = ((int)(thr * fql)) << (J.cfg.bitdepth - 8);
  // calc_cbp as the reference EXECUTES it, i.e. calc_cbp_simd (enc/enc_kernels.c:827-907, selected at
  // encode_block.c:2225 because use_simd = 1): int16 column sums of the residual; for 16/8 wide
  // blocks |sum| > thr per column; for 4x4 the SIMD code tests (col[2k+1] + |col[2k]|) > thr, which
  // is NOT the scalar |col[2k] + col[2k+1]| > thr - the oracle binary runs the SIMD form.
  const int ncol = size == 4 ? 2 : size;
  int f = 0;
  for (int col = t.rank; col < ncol; col += t.size) {
    if (size == 4) {
      int lo = 0, hi = 0;
      for (int i = 0; i < 4; i++) {
        lo = (int16_t)(lo + (int16_t)((int)org[i * ostride + 2 * col] - (int)pred[i * pstride + 2 * col]));
        hi = (int16_t)(hi + (int16_t)((int)org[i * ostride + 2 * col + 1] - (int)pred[i * pstride + 2 * col + 1]));
      }
      if (hi + (int)(int16_t)iabs(lo) > threshold) f = 1;
    } else {
      int sum = 0;
      for (int i = 0; i < size; i++) sum = (int16_t)(sum + (int16_t)((int)org[i * ostride + col] - (int)pred[i * pstride + col]));
      if ((int16_t)iabs(sum) > (int16_t)threshold) f = 1;
    }
  }
  const int r = team_ballot(t, f) != 0ull;
  t.sync();
  return r;
}

template <typename PIX, int SP>
TK_DEVNI int check_early_skip(const Team t, JobR<PIX> J, WsP<PIX> ws, const Node& nd, const BlkParam& p) {
  const auto& c = J.cfg;
  const int size = nd.size, size0 = size < 32 ? size : 32;
  const int qpY = J.qp, qpC = TK_TAB.chroma_qp[qpY];
  float thr = c.early_skip_thr;
  if (c.encoder_speed > 1 && nd.size == sb_size_of(c)) thr += thr / 4;  // encode_block.c:2256-2257
  const int size0c = size0 >> 1;
  int significant = 0;
  for (int i = 0; i < size && !significant; i += size0)
    for (int j = 0; j < size && !significant; j += size0) {
      struct { int ypos, xpos; } sub = {nd.ypos + i, nd.xpos + j};
      const int yc = sub.ypos >> 1, xc = sub.xpos >> 1;
      if (p.dir == 2) {
        pred_inter_yuv<SP>(t, lds_ld(&J.ref[p.ref0]), ws->p0_y, ws->p0_u, ws->p0_v, sub.ypos, sub.xpos, size0, size0, size0, p.mv0,
                       J.sign_ge[p.ref0], c.width, c.height, c.enable_bipred, 0, c.bitdepth);
        pred_inter_yuv<SP>(t, lds_ld(&J.ref[p.ref1]), ws->p1_y, ws->p1_u, ws->p1_v, sub.ypos, sub.xpos, size0, size0, size0, p.mv1,
                       J.sign_ge[p.ref1], c.width, c.height, c.enable_bipred, 0, c.bitdepth);
        t.sync();
        average_yuv<SP>(t, ws->pred_y, ws->pred_u, ws->pred_v, ws->p0_y, ws->p0_u, ws->p0_v, ws->p1_y, ws->p1_u, ws->p1_v,
                    size0, size0, size0);
      } else {
        pred_inter_yuv<SP>(t, lds_ld(&J.ref[p.ref0]), ws->pred_y, ws->pred_u, ws->pred_v, sub.ypos, sub.xpos, size0, size0, size0,
                       p.mv0, J.sign[p.ref0], c.width, c.height, c.enable_bipred, 0, c.bitdepth);
      }
      t.sync();
      significant = early_skip_sub<PIX, SP>(t, J, ws, ws->org_y + i * ws->org_sy + j, ws->org_sy, ws->pred_y, size0,
                                   size0, qpY, thr);
      if (!significant)
        significant = early_skip_subC<PIX, SP>(t, J, ws, ws->org_u + (i >> 1) * ws->org_sc + (j >> 1), ws->org_sc, ws->pred_u, size0c, size0c, qpC, thr);
      if (!significant)
        significant = early_skip_subC<PIX, SP>(t, J, ws, ws->org_v + (i >> 1) * ws->org_sc + (j >> 1), ws->org_sc, ws->pred_v, size0c, size0c, qpC, thr);
    }
  return !significant;
}

// ---------------------------------------------------------------------------------
// Final encode of a CB: recompute (encode_block final), write recon + cell state, emit bits.
// ---------------------------------------------------------------------------------
template <typename PIX, int SP>
TK_DEVNI int final_encode(const Team t, JobR<PIX> J, WsP<PIX> ws, Node& nd, BitSink& out, const BigWs<PIX>* snap = nullptr,
                          int trial_bits = -1) {
  TK_PROF_T0();
  TK_PROFMD_MARK(pfe0_);
  BlkParam p = lds_ld(&nd.best);
  const int size = nd.size, sc = size >> 1;
  const int yc = nd.ypos >> 1, xc = nd.xpos >> 1;
  int nbits = 0;
  if (snap) {
    // the winning trial of the parallel decision left its reconstruction and coefficients in its wave's snapshot: emit + copy
    {
      // cooperative emission: every lane runs the syntax on the same values, lane 0 writes the words (tk_bits.h:bs_coeff_team)
      BitSink w = out;
      w.store = t.rank == 0;
      bs_open(w);
      bs_block_t<true>(w, lds_ld(&nd.syn), p, snap->best_cy, snap->best_cu, snap->best_cv, &t, nullptr);
      bs_close(w);
      out.ovf |= w.ovf;
      nbits = w.pos - out.pos;
    }
    nbits = team_bcast0(t, nbits);
    out.pos += nbits;
    if (TK_PROFMD_ON(4)) TK_PROFMD_ACC(ws, 24, pfe0_);
    copy_block<SP_GLOBAL, SP_GLOBAL>(t, J.rec.y + nd.ypos * J.rec.sy + nd.xpos, J.rec.sy, snap->best_y, size, nd.bw, nd.bh);
    copy_block<SP_GLOBAL, SP_GLOBAL>(t, J.rec.u + yc * J.rec.sc + xc, J.rec.sc, snap->best_u, sc, nd.bw >> 1, nd.bh >> 1);
    copy_block<SP_GLOBAL, SP_GLOBAL>(t, J.rec.v + yc * J.rec.sc + xc, J.rec.sc, snap->best_v, sc, nd.bw >> 1, nd.bh >> 1);
  } else {
    if (trial_bits >= 0) {
      // skip candidate whose trial was the block's last encode_block: its reconstruction is still in ws->rec_*, nd.best carries
      // the fields the trial set, a skip block has no coefficients - the second encode_block would rebuild the same state
      nbits = trial_bits;
    } else {
      BitSink cnt;
      cnt.buf = nullptr; cnt.pos = 0; cnt.cap = 0; cnt.emit = 0; cnt.ovf = 0;
      nbits = encode_block<PIX, SP>(t, J, ws, nd, p, cnt);
    }
    // bits (cooperative emission), then recon copy and cells
    {
      BitSink w = out;
      w.store = t.rank == 0;
      bs_open(w);
      bs_block_t<true>(w, lds_ld(&nd.syn), p, ws->coef_y, ws->coef_u, ws->coef_v, &t, nullptr);
      bs_close(w);
      out.ovf |= w.ovf;
    }
    out.pos += nbits;
    copy_block<SP_GLOBAL, SP>(t, J.rec.y + nd.ypos * J.rec.sy + nd.xpos, J.rec.sy, ws->rec_y, size, nd.bw, nd.bh);
    copy_block<SP_GLOBAL, SP>(t, J.rec.u + yc * J.rec.sc + xc, J.rec.sc, ws->rec_u, sc, nd.bw >> 1, nd.bh >> 1);
    copy_block<SP_GLOBAL, SP>(t, J.rec.v + yc * J.rec.sc + xc, J.rec.sc, ws->rec_v, sc, nd.bw >> 1, nd.bh >> 1);
  }
  // copy_deblock_data (encode_block.c:1568-1613)
  const int tbs = p.tb_param > 0 ? 1 : 0;
  const int pb = p.mode == M_INTER ? p.pb_part : P_NONE;
  const int div = size / (2 * kMinPb);
  const int cw = nd.bw / kMinPb, ch = nd.bh / kMinPb;
  const int cbpbits = tbs ? 7 : ((p.cbp_y ? 1 : 0) | (p.cbp_u ? 2 : 0) | (p.cbp_v ? 4 : 0));
  for (int k = t.rank; k < cw * ch; k += t.size) {
    int m, n;
    split2(mk_div(cw), k, m, n);
    int m0 = div > 0 ? m / div : 0, n0 = div > 0 ? n / div : 0;
    int index = 2 * m0 + n0;
    DbCell& cell = J.cells[(nd.ypos / kMinPb + m) * J.cell_stride + nd.xpos / kMinPb + n];
    cell.mv0 = p.mv0[index];
    cell.mv1 = p.mv1[index];
    cell.mode = (uint8_t)p.mode;
    cell.size = (uint8_t)size;
    cell.tbpb = (uint8_t)(tbs | (pb << 1));
    cell.cbp = (uint8_t)cbpbits;
    cell.ref0 = p.ref0;
    cell.ref1 = p.ref1;
    cell.dir = p.dir;
    cell.pad = 0;
  }
  t.sync();
  TK_PROF_ADD(ws, PF_FINAL);
  return nbits;
}

// ---------------------------------------------------------------------------------
// process_block (encode_block.c:2401-2566) as an explicit-stack traversal of one superblock.
// ---------------------------------------------------------------------------------
// Runs on the master wave (wg.wave == 0); the other waves of the workgroup sit in wg_helper_loop meanwhile.  The
// shared tables (ws->sh->tabs) must have been filled (xform_tables_fill).
// (sb_y, sb_x): the superblock's grid index times kMaxSb, as every caller passes it (k * kMaxSb, l * kMaxSb).  The origin in samples is the
// grid index times the sequence's superblock size, (arg / kMaxSb) << log2_sb_size = arg >> sb_shift: the identity for 128x128 superblocks.
template <typename PIX>
TK_DEV void process_sb(const Wg wg, const Team t, JobR<PIX> J, WsP<PIX> ws, int sb_y, int sb_x, BitSink& out) {
  TK_PROF_T0();
  const auto& c = J.cfg;
  const int fw = c.width, fh = c.height;
  const int sb_size = sb_size_of(c);   // used up to the root node only: the walk below reads it again where it needs it
  sb_y = (sb_y / kMaxSb) * sb_size; sb_x = (sb_x / kMaxSb) * sb_size;
  if (t.rank == 0)
  { MeLists* L = ws->mep->lists; for (int r = 0; r < kMaxRefs; r++) { L->mvcand_num[r] = 0; L->mvcand_mask[r] = 0; } L->best_ref = -1; }
  t.sync();
  if (J.stats && J.frame_type != F_I && t.rank == 0) {
    team_add64(&J.stats[2], 1ull);
    team_add64(&J.stats[3], (unsigned long long)(tmin(sb_size, fw - sb_x) * tmin(sb_size, fh - sb_y)));
  }
  int sp = 0;
  unsigned ret = 0;  // value "returned" by the node that was just popped
  int have_ret = 0;
  {
    Node& n = ws->stack[0];
    if (t.rank == 0) { n.size = sb_size; n.ypos = sb_y; n.xpos = sb_x; n.stage = 0; }
    t.sync();
  }
  while (sp >= 0) {
    Node& nd = ws->stack[sp];
    if (nd.stage == 0) {
      // ---- entry
      const int size = nd.size, ypos = nd.ypos, xpos = nd.xpos;
      if (ypos + kMinBlk > fh || xpos + kMinBlk > fw) { ret = 0; have_ret = 1; sp--; continue; }
      TK_PROFMD_MARK(pen_);
      ws_select(ws, tk_uniform(size));
      t.sync();
      if (t.rank == 0) {
        nd.bw = tmin(size, fw - xpos);
        nd.bh = tmin(size, fh - ypos);
        nd.encode_this_size = ypos + size <= fh && xpos + size <= fw;
        nd.encode_rect = !nd.encode_this_size && J.frame_type != F_I;
        nd.cost_small = 1u << 28;
        nd.bitpos0 = out.pos;
        nd.child = 0;
        nd.md_done = 0;
        nd.cost_this = 1u << 28;
        SynCtx& s = nd.syn;
        s.frame_type = J.frame_type; s.num_ref = J.num_ref; s.enable_bipred = c.enable_bipred; s.interp_ref = J.interp_ref;
        s.max_pb_part = c.enable_pb_split ? 4 : 1; s.max_tb_part = c.enable_tb_split == 1 ? 2 : 1;
        s.num_intra_modes = J.num_intra_modes; s.size = size; s.encode_this_size = nd.encode_this_size;
        s.num_skip = 0; s.num_merge = 0; s.mvp = mk_mv(0, 0);
        find_contexts(J.cells, J.cell_stride, ypos, xpos, fh, fw, size, c.use_block_contexts, &s);
        if (J.frame_type != F_I && (nd.encode_this_size || nd.encode_rect)) {
          s.num_skip = get_mv_cands(J.cells, J.cell_stride, ypos, xpos, fw, fh, size, sb_size_of(c), nd.skip);
          s.num_merge = get_mv_cands(J.cells, J.cell_stride, ypos, xpos, fw, fh, size, sb_size_of(c), nd.merge);
        }
      }
      t.sync();
      org_select(t, J, ws, tk_uniform(size), ypos, xpos, tk_uniform(nd.bw), tk_uniform(nd.bh), 1);
      if (TK_PROFMD_ON(4)) TK_PROFMD_ACC(ws, 22, pen_);
      TK_PROFMD_MARK(pes_);
      // ---- early skip
      const int lds_blk = tk_uniform(size <= kLdsBlk);   // address space of this block's sample buffers (SP_LDS / SP_GLOBAL instances)
      if (nd.encode_this_size && J.frame_type != F_I && c.early_skip_thr > 0.0f) {
        unsigned min_cost = kCostInit;
        int any = 0;
        int best_bits = -1;   // >= 0: the best candidate's trial was the last encode_block (its reconstruction is in ws->rec_*)
        BlkParam p;
        p.intra_mode = 0; p.pb_part = P_NONE; p.tb_param = 0; p.tb_split = 0; p.cbp_y = p.cbp_u = p.cbp_v = 0;
        for (int k = 0; k < nd.syn.num_skip; k++) {
          set_cand(p, nd.skip[k], k, M_SKIP);
          TK_PROF_T0();
          int es_ = lds_blk ? check_early_skip<PIX, SP_LDS>(t, J, ws, nd, p) : check_early_skip<PIX, SP_GLOBAL>(t, J, ws, nd, p);
          TK_PROF_ADD(ws, PF_ESKIP);
          if (es_) {
            any = 1;
            // The check of a block of up to 32x32 predicts the whole block in one piece with the arguments predict_inter uses for
            // a uni-directional skip candidate, into the same buffers, and only reads them afterwards: the trial takes it over.
            const int reuse = tk_uniform(size <= 32 && p.dir != 2) ? 2 : 0;
            int nb = 0;
            unsigned cost = lds_blk ? rdo_trial<PIX, SP_LDS>(t, J, ws, nd, p, J.lambda, reuse, 0xffffffffu, nullptr, 0, &nb)
                                    : rdo_trial<PIX, SP_GLOBAL>(t, J, ws, nd, p, J.lambda, reuse, 0xffffffffu, nullptr, 0, &nb);
            if (cost < min_cost) { min_cost = cost; best_bits = nb; if (t.rank == 0) keep_best(nd, p); t.sync(); }
            else best_bits = -1;
          }
        }
        if (any) {
          if (J.stats && t.rank == 0) {
            team_add64(&J.stats[0], (unsigned long long)(nd.bw * nd.bh));
            if (nd.size == sb_size_of(c)) team_add64(&J.stats[1], 1ull);
          }
          const int nbits = lds_blk ? final_encode<PIX, SP_LDS>(t, J, ws, nd, out, nullptr, best_bits)
                                    : final_encode<PIX, SP_GLOBAL>(t, J, ws, nd, out, nullptr, best_bits);
          (void)nbits;
          // The reference recomputes cost_calc on the final reconstruction (encode_block.c:2483-2488): the final encode repeats the
          // winning trial (same prediction, same bits), so that value is the trial's cost.
          ret = min_cost;
#if TK_HOST
          if (getenv("THOR_DBG")) fprintf(stderr, "F %d y %d x %d s %d ES mode %d idx %d cost %u bits %d\n", J.frame_num, nd.ypos, nd.xpos, nd.size, nd.best.mode, nd.best.skip_idx, ret, nbits);
#endif
          have_ret = 1;
          sp--;
          if (TK_PROFMD_ON(4)) TK_PROFMD_ACC(ws, 23, pes_);
          continue;
        }
      }
      if (TK_PROFMD_ON(4)) TK_PROFMD_ACC(ws, 23, pes_);
      // ---- split signalling + children (bottom-up), unless this is a top-down 16x16 (encode_block.c:2418)
      const int top_down = size == 2 * kMinBlk && nd.encode_this_size && J.frame_type != F_I && c.encoder_speed > 0;
      if (size > kMinBlk && !top_down) {
        if (t.rank == 0) {
          BitSink w = out;
          bs_open(w);
          bs_super_mode(w, nd.syn, 0, 0, 1);
          bs_close(w);
          out.ovf |= w.ovf;
          nd.cost_small = 0;
        }
        {
          BitSink cnt = out;
          cnt.emit = 0;
          bs_super_mode(cnt, nd.syn, 0, 0, 1);
          out.pos = cnt.pos;
        }
        t.sync();
        if (t.rank == 0) nd.stage = 1;
        t.sync();
      } else {
        if (t.rank == 0) nd.stage = 2;
        t.sync();
      }
      have_ret = 0;
      continue;
    }
    if (nd.stage == 1) {
      // ---- children TL, BL, TR, BR (encode_block.c:2513-2516)
      if (have_ret) {
        if (t.rank == 0) nd.cost_small += ret;
        have_ret = 0;
        t.sync();
      }
      if (nd.child < 4) {
        const int ch = nd.child, hs = nd.size / 2;
        Node& cn = ws->stack[sp + 1];
        t.sync();
        if (t.rank == 0) {
          cn.size = hs;
          cn.ypos = nd.ypos + ((ch & 1) ? hs : 0);   // order: (0,0) (1,0) (0,1) (1,1) in (y,x)
          cn.xpos = nd.xpos + ((ch & 2) ? hs : 0);
          cn.stage = 0;
          nd.child = ch + 1;
        }
        t.sync();
        sp++;
        continue;
      }
      if (t.rank == 0) nd.stage = 2;
      t.sync();
    }
    // ---- stage 2: decide this size
    {
      ws_select(ws, tk_uniform(nd.size));
      org_select(t, J, ws, tk_uniform(nd.size), nd.ypos, nd.xpos, tk_uniform(nd.bw), tk_uniform(nd.bh), 1);  // the children replaced the LDS copy
      unsigned cost = 1u << 28;
      int snap_wave = -1;
      if (nd.encode_this_size || nd.encode_rect) {
        if (!nd.md_done) {
          const int rect = nd.bw != nd.size || nd.bh != nd.size;
          if (c.encoder_speed == 0 && c.intra_rdo && !rect) cost = mode_decision_par(wg, t, J, ws, sp, &snap_wave);
          else cost = nd.size <= kLdsBlk ? mode_decision<PIX, SP_LDS>(t, J, ws, nd) : mode_decision<PIX, SP_GLOBAL>(t, J, ws, nd);
          t.sync();
#if TK_HOST
          if (getenv("THOR_DBG")) fprintf(stderr, "F %d y %d x %d s %d RDO mode %d cost %u small %u ref %d part %d tb %d mv %d %d\n", J.frame_num, nd.ypos, nd.xpos, nd.size, nd.best.mode, cost, nd.cost_small, nd.best.ref0, nd.best.pb_part, nd.best.tb_param, nd.best.mv0[0].x, nd.best.mv0[0].y);
#endif
          // top-down 16x16 (encoder_speed > 0, encode_block.c:2418-2419, 2528-2537): the children are only
          // tried when this size costs more than size^2 * iq_8x8[qp] / 8
          const int top_down = nd.size == 2 * kMinBlk && nd.encode_this_size && J.frame_type != F_I && c.encoder_speed > 0;
          if (top_down && cost > (unsigned)(nd.size * nd.size * TK_TAB.iq_8x8[J.qp] / 8)) {
            out.pos = nd.bitpos0;
            if (t.rank == 0) {
              BitSink w = out;
              bs_open(w);
              bs_super_mode(w, nd.syn, 0, 0, 1);
              bs_close(w);
              out.ovf |= w.ovf;
              nd.cost_small = 0;
              nd.md_done = 1;
              nd.cost_this = cost;
              nd.stage = 1;
            }
            {
              BitSink cnt = out;
              cnt.emit = 0;
              bs_super_mode(cnt, nd.syn, 0, 0, 1);
              out.pos = cnt.pos;
            }
            t.sync();
            have_ret = 0;
            continue;
          }
        } else cost = nd.cost_this;
        if (cost <= nd.cost_small) {
          out.pos = nd.bitpos0;
          // decided just now by the parallel decision: the winner's wave still holds its trial (snapshot_trial)
          const BigWs<PIX>* snap = snap_wave >= 0 ? (const BigWs<PIX>*)ldsc(ws->sh)->wsnap[snap_wave] : nullptr;
          TK_PROFMD_MARK(pfe_);
          if (nd.size <= kLdsBlk) final_encode<PIX, SP_LDS>(t, J, ws, nd, out, snap);
          else final_encode<PIX, SP_GLOBAL>(t, J, ws, nd, out, snap);
          if (TK_PROFMD_ON(4)) TK_PROFMD_ACC(ws, 25, pfe_);   // whole call; slot 24 holds the emission part of the snapshot path
        }
      }
      ret = cost < nd.cost_small ? cost : nd.cost_small;
      have_ret = 1;
      sp--;
    }
  }
  // release the parked waves
  t.sync();
  if (t.rank == 0) ws->sh->cmd = WG_CMD_EXIT;
  t.sync();
  wg.barrier();
  wg.barrier();  // all parked waves have seen WG_CMD_EXIT (see wg_helper_loop)
  TK_PROF_ADD(ws, PF_SB);
}

}  // namespace tk
