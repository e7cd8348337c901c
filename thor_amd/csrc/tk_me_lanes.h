// tk_me_lanes.h - the lane-per-candidate passes: me_cand_fullpel, me_cand8_subpel, me_cand16_subpel.
#pragma once
#include "tk_me_seg.h"

namespace tk {
// ---------------------------------------------------------------------------------------------------------------------------------
// Full-pel search of an 8-bit PU of up to 32x32 samples with ONE LANE PER CANDIDATE (round 5).
// tools/ubench_me.cpp: with nothing else on the CU a search of a 4x4 PU costs the generic passes of motion_estimate 21 k cycles (4.3 k
// per telescope step, 22 k per step for 32x32).  A pass there is ~450 wave-instructions at ~5 cycles each, and most of them are not sample
// work: the lanes of a candidate GROUP (one row segment per lane) all form the candidate's vector, clip it, price it (two vector-bit
// counts + a double-precision multiply-add: ~45 instructions) - and a lane does that for every candidate SET of the pass (4 per lane for
// an 8x8 PU, 24 for a 32x32 one).  A wavefront issues one vector instruction per 4 clocks whatever the lanes do, so the instruction
// count per lane is the time.  Here lane c IS candidate c of the pass (25 grid points, <= 64 list entries, 6 hexagon points): it forms,
// clips and prices its vector ONCE and walks the rows of the block itself - per 16-byte row segment one broadcast read of the original
// (same address in every lane), one unaligned read of its own displaced segment from the staged window (or the plane) and v_sad_u8.
// 8x8: ~130 instructions per pass instead of ~450; 32x32: ~900 instead of ~5 000.  No cross-lane work except the final minimum.
// Same passes, same order, same costs, winner = min over (cost, evaluation index) = the reference's sequential strict-'<' scan
// (enc/encode_block.c:517-616); no duplicate-candidate bookkeeping (a vector evaluated twice cannot win twice).
//   NB: bytes per row segment (4, 8: the PU width; 16: widths 16 and 32 = one or two segments per row)
//   Round 6: PIX = uint16_t too (the reference's _hbd searches: SAD >> (bitdepth - 8), enc/encode_block.c:417-428): the same walk with v_sad_u16 on
//   16-byte segments of eight samples - one (8 wide), two (16) or four (32) segments per row, `sh` = bitdepth - 8.
template <typename PIX, int NB, int SP>
TK_DEVNI unsigned long long me_cand_fullpel(const Team t, MeWs* w_, const PIX* org_, const PIX* ref, int a_cb, int a_ostride, int a_width, int a_height,
                                            int a_rstride, int a_sign, int a_fw, int a_fh, int a_xpos, int a_ypos, double a_lam, const uint32_t* win_w32, int win_ox,
                                            int win_oy, int win_Ww, int win_Wh, int win_pitch, int win_on, mv_t mvc, mv_t mvp, int ref_idx, int a_sh) {
  constexpr int S = (int)sizeof(PIX), SPS = 16 / S;   // bytes per sample, samples per 16-byte segment
  const int sh = tk_uniform(a_sh);
  // (scalars one by one and the result in registers: a struct - by reference or by value - is a trip through the caller's stack in scratch memory)
  MeWin win_in;
  win_in.w32 = win_w32; win_in.ox = win_ox; win_in.oy = win_oy; win_in.Ww = win_Ww; win_in.Wh = win_Wh; win_in.pitch = win_pitch; win_in.on = win_on;
  const auto lists = ldsc(lds_ld(&w_->lists));
  // wave-uniform scalars
  const int cb = tk_uniform(a_cb), ostride = tk_uniform(a_ostride), width = tk_uniform(a_width), height = tk_uniform(a_height);
  const int rstride = tk_uniform(a_rstride), sign = tk_uniform(a_sign), fw = tk_uniform(a_fw), fh = tk_uniform(a_fh);
  const int xpos = tk_uniform(a_xpos), ypos = tk_uniform(a_ypos);
  const double lam = tk_uniform_f64(a_lam);
  const MeWin win = uniform(win_in);
  mvc = uniform(mvc);
  mvp = uniform(mvp);
  ref_idx = tk_uniform(ref_idx);
  org_ = tk_uniform_ptr(org_);
  ref = tk_uniform_ptr(ref);
  const int s = sign ? -1 : 1;
  const int spr = NB == 16 ? ((width * S) >> 4) : 1;   // 16-byte segments per row
  unsigned min_sad = kCostInit;
  mv_t mv_opt = mk_mv(0, 0);
  mv_t mv_ref = mk_mv(((mvc.x + 2) >> 2) << 2, ((mvc.y + 2) >> 2) << 2);
  auto clip_free = [&](mv_t ctr, int R) -> int {   // motion_estimate's test: no vector within +-R quarter-pels of ctr needs clipping
    const int ext = kPadY - 16, cy = s * ctr.y, cx = s * ctr.x;
    return ypos + ((cy - R) >> 2) >= -ext && ypos + ((cy + R + 3) >> 2) + cb <= fh + ext && xpos + ((cx - R) >> 2) >= -ext && xpos + ((cx + R + 3) >> 2) + cb <= fw + ext;
  };
  // SAD of the block displaced by (dx + off, dy) against the original: the lane's own walk over the rows, four rows in flight (heights are
  // multiples of four); window / plane and one / two segments per row are decided outside the loop (straight-line bodies: all eight or
  // sixteen reads of an iteration are issued before the first SAD waits for them)
  auto rows_sad = [&](auto win_tag, auto spr_tag, int dx, int dy, int off) -> unsigned {
    constexpr int WIN = decltype(win_tag)::value, SPR = decltype(spr_tag)::value, ROWS = SPR >= 4 ? 1 : 4 / SPR;   // four segments in flight
    unsigned sad = 0;
    int wb = mul24(dy - win.oy, win.pitch) + (dx + off - win.ox) * S;   // bytes
    const PIX* gb = ref + mul24(dy, rstride) + (dx + off);
    const PIX* ob = org_;
    for (int i = 0; i < height; i += ROWS) {
      Seg16 o[ROWS * SPR], r[ROWS * SPR];
      TK_UNROLL
      for (int k = 0; k < ROWS; k++)
        TK_UNROLL
        for (int sg = 0; sg < SPR; sg++) {
          o[k * SPR + sg] = seg_load<SP, NB>(ob + mul24(k, ostride) + SPS * sg);   // the same address in every lane
          if constexpr (WIN) r[k * SPR + sg] = win_seg<NB>(win.w32, wb + mul24(k, win.pitch) + 16 * sg);
          else r[k * SPR + sg] = seg_load<SP_GLOBAL, NB>(gb + mul24(k, rstride) + SPS * sg);
        }
      TK_UNROLL
      for (int q = 0; q < ROWS * SPR; q++) sad = (unsigned)seg_sad<PIX, NB>(o[q], r[q], (int)sad);
      wb += ROWS * win.pitch; gb += ROWS * rstride; ob += ROWS * ostride;
    }
    return sad;
  };
  struct T0 { enum { value = 0 }; };
  struct T1 { enum { value = 1 }; };
  struct T2 { enum { value = 2 }; };
  struct T4 { enum { value = 4 }; };
  auto block_sad = [&](int use_win, int dx, int dy, int off) -> unsigned {
    if constexpr (NB == 16) {
      if (spr == 2) return use_win ? rows_sad(T1(), T2(), dx, dy, off) : rows_sad(T0(), T2(), dx, dy, off);
      if constexpr (S == 2) { if (spr == 4) return use_win ? rows_sad(T1(), T4(), dx, dy, off) : rows_sad(T0(), T4(), dx, dy, off); }
    }
    return use_win ? rows_sad(T1(), T1(), dx, dy, off) : rows_sad(T0(), T1(), dx, dy, off);
  };
  // Cost of THIS LANE's candidate (vector m, not yet clipped; `valid` lanes only - the others return ~0u).  Every vector is clipped with clip_mv,
  // which leaves a vector inside the clip-free area alone: the same vectors motion_estimate evaluates with or without its `noclip` short cut.
  // WIDE (16x16 coding blocks, candidate list): the cost is that of the best x offset of {-3, -1, 0, 1, 3} (first minimum) with the vector moved
  // there (encode_block.c:430-453); *osel = that offset's index.
  auto lane_cost = [&](mv_t m, int valid, auto wide_tag, unsigned* osel) -> unsigned {
    constexpr int WIDE = decltype(wide_tag)::value;
    m = clip_mv(m, ypos, xpos, fw, fh, cb, cb, sign);
    {  // lanes without a candidate evaluate lane 0's vector (always a candidate) and drop the result: their own may point outside the staged window
      const int mp0 = team_bcast0(t, (int)(uint16_t)m.x | ((int)m.y << 16));
      if (!valid) m = mk_mv((int16_t)(mp0 & 0xffff), mp0 >> 16);
    }
    const int dx = s * (m.x >> 2), dy = s * (m.y >> 2);
    const int x0 = dx - (WIDE ? 3 : 0), x1 = dx + (WIDE ? 3 : 0);
    const int outside = valid && !(x0 >= win.ox && x1 + width <= win.ox + win.Ww && dy >= win.oy && dy + height <= win.oy + win.Wh);
    const int use_win = win.on && team_ballot(t, outside) == 0ull;
    unsigned sad;
    int mx = m.x;
    if constexpr (WIDE) {
      sad = 1u << 31;
      int bx = 0;
      for (int q = 0; q < 5; q++) {
        const int off = q == 0 ? -3 : q == 1 ? -1 : q == 2 ? 0 : q == 3 ? 1 : 3;
        const unsigned v = block_sad(use_win, dx, dy, off);
        if (v < sad) { sad = v; bx = off; *osel = (unsigned)q; }
      }
      mx = (int16_t)(m.x + ((s * bx) << 2));
    } else
      sad = block_sad(use_win, dx, dy, 0);
    const unsigned cost = (sad >> sh) + mv_cost(lam, m.y - mvp.y, mx - mvp.x);
    return valid ? cost : ~0u;
  };
  // min over the lanes [lo, lo + n) of (cost << 8 | lane - lo): the first candidate in evaluation order among the cheapest; ~0u for n == 0
  auto range_min = [&](unsigned cost, int lo, int n) -> unsigned {
    const int c = t.rank - lo;
    unsigned k = (cost << 8) | (unsigned)(c & 0xff);
    if (c < 0 || c >= n || cost == ~0u) k = ~0u;
    return team_min32(t, k);
  };
  struct NoWide { enum { value = 0 }; };
  struct Wide { enum { value = 1 }; };
  auto grid_mv = [&](mv_t centre, int step, int c) -> mv_t {   // point c of the 5x5 grid of spacing `step` around centre; the centre is skipped after the first step
    const int idx = (step < 32 && c >= 12) ? c + 1 : c;
    const int q = mul24(idx, 13) >> 6;   // idx / 5
    return mk_mv(centre.x + mul24(idx - q - (q << 2) - 2, step), centre.y + mul24(q - 2, step));
  };
  auto take = [&](mv_t m) {   // new optimum (clipped the way its candidate was), wave-uniform
    m = clip_mv(m, ypos, xpos, fw, fh, cb, cb, sign);
    mv_opt = mk_mv(tk_uniform(m.x), tk_uniform(m.y));
  };
  // --- telescope (encode_block.c:529-561): steps of 32, 16, 8, 4 quarter-pels.  A step is evaluated TOGETHER with the next one around the same
  // centre (25 + 24 or 24 + 24 lanes): when the step leaves the optimum on its centre - the usual case with a good predictor - the next step's grid is
  // exactly that one and its costs are already there; otherwise they are dropped and the next step runs from its real centre.
  for (int step = 32; step >= 4;) {
#ifdef TK_ME_NOSPEC   // tools/ubench_me.cpp: every step / round a pass of its own
    const int n1 = step < 32 ? 24 : 25, n2 = 0;
#else
    const int n1 = step < 32 ? 24 : 25, n2 = step > 4 ? 24 : 0;
#endif
    const mv_t centre = mv_ref;
    const int c1 = t.rank, c2 = t.rank - n1;
    const int v1 = c1 < n1, v2 = c2 >= 0 && c2 < n2;
    const mv_t m = v2 ? grid_mv(centre, step >> 1, c2) : grid_mv(centre, step, v1 ? c1 : 0);
    const unsigned cost = lane_cost(m, v1 || v2, NoWide(), nullptr);
    const unsigned k1 = range_min(cost, 0, n1);
    if (k1 != ~0u && (k1 >> 8) < min_sad) { min_sad = k1 >> 8; take(grid_mv(centre, step, (int)(k1 & 0xffu))); }
    mv_ref = mv_opt;
    step >>= 1;
    if (n2 && mv_ref.x == centre.x && mv_ref.y == centre.y) {   // the next step's centre is this one's: its costs are in lanes n1 .. n1 + 23
      const unsigned k2 = range_min(cost, n1, n2);
      if (k2 != ~0u && (k2 >> 8) < min_sad) { min_sad = k2 >> 8; take(grid_mv(centre, step, (int)(k2 & 0xffu))); }
      mv_ref = mv_opt;
      step >>= 1;
    }
  }
  // --- candidate list (encode_block.c:564-581)
  {
    const int n = TKU(lists->mvcand_num[ref_idx]);
    if (n > 0) {
      auto list_mv = [&](int c) -> mv_t { return mk_mv((int16_t)(lists->mvcand[ref_idx][c].x << 2), (int16_t)(lists->mvcand[ref_idx][c].y << 2)); };
      const int valid = t.rank < n;
      const mv_t m = list_mv(valid ? t.rank : 0);
      if (cb == 16) {
        unsigned osel = 0;
        const unsigned cost = lane_cost(m, valid, Wide(), &osel);
        const unsigned k = range_min(cost, 0, n);
        if (k != ~0u && (k >> 8) < min_sad) {
          min_sad = k >> 8;
          const int c = (int)(k & 0xffu);
          const int q = team_read_lane(t, (int)osel, c);   // the winner's offset
          mv_t mm = clip_mv(list_mv(c), ypos, xpos, fw, fh, cb, cb, sign);
          const int bx = q == 0 ? -3 : q == 1 ? -1 : q == 2 ? 0 : q == 3 ? 1 : 3;
          mm.x = (int16_t)(mm.x + ((s * bx) << 2));
          mv_opt = mk_mv(tk_uniform(mm.x), tk_uniform(mm.y));   // (the moved vector is not clipped again: encode_block.c:447-451)
        }
      } else {
        const unsigned cost = lane_cost(m, valid, NoWide(), nullptr);
        const unsigned k = range_min(cost, 0, n);
        if (k != ~0u && (k >> 8) < min_sad) { min_sad = k >> 8; take(list_mv((int)(k & 0xffu))); }
      }
    }
    mv_ref = mv_opt;
  }
  // --- hexagon refinement (encode_block.c:583-616): up to 5 rounds of 6, then 3 points.  A round is evaluated together with the next round of
  // every direction it can move in (6 + 6 x 3 or 3 + 3 x 3 lanes): the usual search ends after one or two rounds = one pass.
  {
    auto hex_off = [&](int dir, int* ox, int* oy) {
      *ox = dir == 0 ? 1 : dir == 1 ? 2 : dir == 2 ? 1 : dir == 3 ? -1 : dir == 4 ? -2 : -1;
      *oy = dir == 0 ? -1 : dir == 1 ? 0 : dir == 2 ? 1 : dir == 3 ? 1 : dir == 4 ? 0 : -1;
    };
    int start = 0, end = 5;
    for (int round = 1; round < 6;) {
      const int n = (end - start + 6) % 6 + 1;   // 6 in the first round, 3 afterwards
      const mv_t centre = mv_ref;
      // lanes [0, n): this round; lanes [n + 3 j, n + 3 j + 3): the next round if this one moves to its point j (new start = that direction - 1)
      const int L = t.rank;
      int ox, oy, valid = L < n * 4;
      mv_t m;
      {
        const int j = L < n ? L : mul24(L - n, 11) >> 5;   // (L - n) / 3 for L - n < 32
        const int dir1 = (start + (j < n ? j : 0)) % 6;
        hex_off(dir1, &ox, &oy);
        m = mk_mv(centre.x + ox * 4, centre.y + oy * 4);
        if (L >= n) {
          const int st2 = dir1 ? dir1 - 1 : 5;
          const int dir2 = (st2 + (L - n - mul24(j, 3))) % 6;
          hex_off(dir2, &ox, &oy);
          m = mk_mv(m.x + ox * 4, m.y + oy * 4);
        }
      }
#ifdef TK_ME_NOSPEC
      const int speculate = 0;
#else
      const int speculate = round < 5;
#endif
      if (!speculate) valid = L < n;
      const unsigned cost = lane_cost(m, valid, NoWide(), nullptr);
      int which = -1;
      const unsigned k = range_min(cost, 0, n);
      auto hex_mv = [&](mv_t ctr, int st, int c) -> mv_t { int x, y; hex_off((st + c) % 6, &x, &y); return mk_mv(ctr.x + x * 4, ctr.y + y * 4); };
      if (k != ~0u && (k >> 8) < min_sad) { min_sad = k >> 8; which = (int)(k & 0xffu); take(hex_mv(centre, start, which)); }
      int best_dir = which < 0 ? -1 : (start + which) % 6;
      // (the next round's centre is the point as this round evaluated it; a clipped point is not the speculated centre: fall back to a fresh pass)
      const mv_t raw = which < 0 ? centre : hex_mv(centre, start, which);
      mv_ref = mv_opt;
      const int start0 = start;
      start = best_dir ? best_dir - 1 : 5;
      end = start + 2;
      end -= (end >= 6) * 6;
      round++;
      if (best_dir < 0) break;
      if (speculate && round < 6 && raw.x == mv_ref.x && raw.y == mv_ref.y) {
        // the next round around the new centre: its three points are lanes n + 3 * which ..
        (void)start0;
        const mv_t centre2 = mv_ref;
        const unsigned k2 = range_min(cost, n + 3 * which, 3);
        int which2 = -1;
        if (k2 != ~0u && (k2 >> 8) < min_sad) { min_sad = k2 >> 8; which2 = (int)(k2 & 0xffu); take(hex_mv(centre2, start, which2)); }
        best_dir = which2 < 0 ? -1 : (start + which2) % 6;
        mv_ref = mv_opt;
        start = best_dir ? best_dir - 1 : 5;
        end = start + 2;
        end -= (end >= 6) * 6;
        round++;
        if (best_dir < 0) break;
      }
    }
  }
  return ((unsigned long long)min_sad << 32) | ((unsigned long long)(uint16_t)mv_opt.x << 16) | (unsigned long long)(uint16_t)mv_opt.y;
}


// ---------------------------------------------------------------------------------------------------------------------------------
// One sub-pel pass (the eight half- or quarter-pel neighbours of `base`, encode_block.c:628-663) of an 8-bit PU of up to 32x32 samples with
// EIGHT LANES PER CANDIDATE (round 5).  tools/ubench_me.cpp: the generic pass costs ~8.5 k cycles for a 4x4 or 8x8 PU - nine luma_setups,
// eight tap tables and eight vector prices formed by every lane (~900 wave-instructions) around ~200 instructions of sample work.  Here lane
// (c, p) = candidate c = lane / 8, part p = lane % 8: a lane sets up, interpolates and prices ITS candidate only.  The PU is cut into
// column strips of 8 (4 for 4-row PUs) samples; a strip needs the 13 (9) window rows around it once: per row two v_dot4 on the eight
// bytes as loaded give the horizontal sum, six 24-bit multiply-adds per sample the vertical one (the strip form of subk8_strip_dy).
// The (1/2, 1/2) position's 12-tap filter (inter_prediction.c:146-160) is the same machinery with two horizontal tap sets (rows 1, 4:
// {0,0,1,1,0,0}; rows 2, 3: {0,1,2,2,1,0}), vertical weights {0,1,1,1,1,0} and rounding (sum + 8) >> 4, so the lanes of different
// candidates do not diverge; the second tap set is only formed when some candidate of the pass is such a position (wave-uniform).
// Requires every candidate's interpolation window inside the staged LDS window; returns 0xffffffff (the caller runs the generic pass) otherwise,
// else min over the candidates of (cost << 8 | c), cost exactly motion_estimate's.
template <int SP>
TK_DEVNI unsigned me_cand8_subpel(const Team t, const uint8_t* org_, int a_ostride, int a_width, int a_height, int a_sign, int a_fw, int a_fh, int a_xpos, int a_ypos,
                                  int a_bipred, double a_lam, const uint32_t* win_w32, int win_ox, int win_oy, int win_Ww, int win_Wh, int win_pitch, int win_on, mv_t base,
                                  int d, mv_t mvp) {
  enum : unsigned { kNone = 0xffffffffu };   // "not in the window": the caller runs the generic pass (a real key is below it: costs fit 24 bits)
  struct { int ostride, width, height, sign, fwidth, fheight, xpos, ypos, enable_bipred; double lam; } a_in = {a_ostride, a_width, a_height, a_sign, a_fw, a_fh, a_xpos, a_ypos, a_bipred, a_lam};
  MeWin win_in;
  win_in.w32 = win_w32; win_in.ox = win_ox; win_in.oy = win_oy; win_in.Ww = win_Ww; win_in.Wh = win_Wh; win_in.pitch = win_pitch; win_in.on = win_on;
  const int ostride = tk_uniform(a_in.ostride), width = tk_uniform(a_in.width), height = tk_uniform(a_in.height), sign = tk_uniform(a_in.sign);
  const int fw = tk_uniform(a_in.fwidth), fh = tk_uniform(a_in.fheight), xpos = tk_uniform(a_in.xpos), ypos = tk_uniform(a_in.ypos);
  const int bip = tk_uniform(a_in.enable_bipred);
  const double lam = tk_uniform_f64(a_in.lam);
  const MeWin win = uniform(win_in);
  base = uniform(base);
  mvp = uniform(mvp);
  d = tk_uniform(d);
  org_ = tk_uniform_ptr(org_);
  if (!win.on) return kNone;
  const int c = t.rank >> 3, part = t.rank & 7;
  // order: (0,-d) (-d,0) (d,0) (0,d) (-d,-d) (-d,d) (d,-d) (d,d) as (y,x)
  const int oy = c == 0 ? 0 : c == 1 ? -d : c == 2 ? d : c == 3 ? 0 : c == 4 ? -d : c == 5 ? -d : d;
  const int ox = c == 0 ? -d : c == 1 ? 0 : c == 2 ? 0 : c == 3 ? d : c == 4 ? -d : c == 5 ? d : c == 6 ? -d : d;
  const mv_t mv = mk_mv(base.x + ox, base.y + oy);
  const SubPel sp = luma_setup(mv, sign, width, height, fw, fh, xpos, ypos, bip);
  const int centre = sp.ver_frac == 2 && sp.hor_frac == 2 && bip < 2;
  // interpolation window of the whole PU for this candidate: rows ver_int - 2 .. ver_int + height + 2, columns hor_int - 2 .. hor_int + width + 5
  const int outside = !(sp.hor_int - 2 >= win.ox && sp.hor_int + width + 6 <= win.ox + win.Ww && sp.ver_int - 2 >= win.oy && sp.ver_int + height + 3 <= win.oy + win.Wh);
  if (team_ballot(t, outside) != 0ull) return kNone;
  const int dual = team_ballot(t, centre) != 0ull;   // wave-uniform
  // per-lane filter description (see the header): horizontal taps A (vertical positions 0, 1, 4, 5) and B (2, 3) as int8 lanes, vertical weights
  const unsigned long long thA = centre ? 0x0000000001010000ull : sp.ph, thB = centre ? 0x0000000102020100ull : sp.ph;
  const int biasA = centre ? 128 * 2 : 128 * 64, biasB = centre ? 128 * 6 : 128 * 64;
  int tv[6];
  for (int m = 0; m < 6; m++) tv[m] = centre ? (m >= 1 && m <= 4 ? 1 : 0) : sp.tv[m];
  const int rnd = centre ? 8 : 2048, rsh = centre ? 4 : 12;
  const int lgw = ilog2((unsigned)width);
  const int SH = height == 4 ? 4 : 8;                      // strip height
  const int units = width * (height == 4 ? 1 : (height >> 3));
  unsigned sad = 0;
  auto strip = [&](auto sh_tag, auto dual_tag, int i0, int j) {
    constexpr int SHC = decltype(sh_tag)::value, DUAL = decltype(dual_tag)::value, NR = SHC + 5;
    const int woff = mul24(i0 + sp.ver_int - 2 - win.oy, win.pitch) + (j + sp.hor_int - 2 - win.ox);
    int hA[NR], hB[NR];
    TK_UNROLL
    for (int r = 0; r < NR; r++) {
      const Seg16 sg = win_seg<8>(win.w32, woff + mul24(r, win.pitch));
      const unsigned lo = sg.d[0] ^ 0x80808080u, hi = sg.d[1] ^ 0x80808080u;   // samples - 128 as int8 lanes
      hA[r] = dot4_i8((int)(unsigned)thA, (int)lo, dot4_i8((int)(unsigned)(thA >> 32), (int)hi, biasA));
      if constexpr (DUAL) hB[r] = dot4_i8((int)(unsigned)thB, (int)lo, dot4_i8((int)(unsigned)(thB >> 32), (int)hi, biasB));
      else hB[r] = hA[r];
    }
    TK_UNROLL
    for (int q = 0; q < SHC; q++) {
      int sum = mul24(tv[0], hA[q]) + mul24(tv[1], hA[q + 1]) + mul24(tv[2], hB[q + 2]) + mul24(tv[3], hB[q + 3]) + mul24(tv[4], hA[q + 4]) + mul24(tv[5], hA[q + 5]);
      const int pr = sat_pix((sum + rnd) >> rsh, 8);
      const int o = (int)spc<SP>(org_)[mul24(i0 + q, ostride) + j];
      sad += (unsigned)(o > pr ? o - pr : pr - o);
    }
  };
  struct S4 { enum { value = 4 }; };
  struct S8 { enum { value = 8 }; };
  struct D0 { enum { value = 0 }; };
  struct D1 { enum { value = 1 }; };
  for (int u = part; u < units; u += 8) {
    const int j = u & (width - 1), i0 = (u >> lgw) << 3;
    if (SH == 4) { if (dual) strip(S4(), D1(), 0, j); else strip(S4(), D0(), 0, j); }
    else { if (dual) strip(S8(), D1(), i0, j); else strip(S8(), D0(), i0, j); }
  }
  const unsigned tot = (unsigned)team_group_sum(t, (int)sad, 8);
  const unsigned cost = tot + mv_cost(lam, mv.y - mvp.y, mv.x - mvp.x);
  unsigned k = (cost << 8) | (unsigned)c;
  if (part != 0) k = ~0u;
  return team_min32(t, k);
}


// The same pass on 16-bit samples (round 6): lane (c, p) = candidate c = lane / 8, part p = lane % 8; a strip is one column of 8 (4) samples whose 13 (9)
// window rows are read once - six samples = three dwords at the candidate's byte offset (win_seg: any alignment), the six horizontal taps packed in
// pairs: three v_dot2_i32_i16 per row sum (|sum| <= 94 * 4095 < 2^19), six 24-bit multiply-adds per sample vertically; the (1/2, 1/2) position's 12-tap
// filter as two horizontal tap sets with vertical weights {0,1,1,1,1,0} and (sum + 8) >> 4, exactly as in me_cand8_subpel.  SAD >> (bitdepth - 8).
template <int SP>
TK_DEVNI unsigned me_cand16_subpel(const Team t, const uint16_t* org_, int a_ostride, int a_width, int a_height, int a_sign, int a_fw, int a_fh, int a_xpos, int a_ypos,
                                   int a_bipred, double a_lam, const uint32_t* win_w32, int win_ox, int win_oy, int win_Ww, int win_Wh, int win_pitch, int win_on, mv_t base,
                                   int d, mv_t mvp, int a_bitdepth) {
  enum : unsigned { kNone = 0xffffffffu };
  struct { int ostride, width, height, sign, fwidth, fheight, xpos, ypos, enable_bipred, bitdepth; double lam; } a_in = {a_ostride, a_width, a_height, a_sign, a_fw, a_fh, a_xpos, a_ypos, a_bipred, a_bitdepth, a_lam};
  MeWin win_in;
  win_in.w32 = win_w32; win_in.ox = win_ox; win_in.oy = win_oy; win_in.Ww = win_Ww; win_in.Wh = win_Wh; win_in.pitch = win_pitch; win_in.on = win_on;
  const int ostride = tk_uniform(a_in.ostride), width = tk_uniform(a_in.width), height = tk_uniform(a_in.height), sign = tk_uniform(a_in.sign);
  const int fw = tk_uniform(a_in.fwidth), fh = tk_uniform(a_in.fheight), xpos = tk_uniform(a_in.xpos), ypos = tk_uniform(a_in.ypos);
  const int bip = tk_uniform(a_in.enable_bipred), bitdepth = tk_uniform(a_in.bitdepth);
  const double lam = tk_uniform_f64(a_in.lam);
  const MeWin win = uniform(win_in);
  base = uniform(base);
  mvp = uniform(mvp);
  d = tk_uniform(d);
  org_ = tk_uniform_ptr(org_);
  if (!win.on) return kNone;
  const int c = t.rank >> 3, part = t.rank & 7;
  const int oy = c == 0 ? 0 : c == 1 ? -d : c == 2 ? d : c == 3 ? 0 : c == 4 ? -d : c == 5 ? -d : d;
  const int ox = c == 0 ? -d : c == 1 ? 0 : c == 2 ? 0 : c == 3 ? d : c == 4 ? -d : c == 5 ? d : c == 6 ? -d : d;
  const mv_t mv = mk_mv(base.x + ox, base.y + oy);
  const SubPel sp = luma_setup(mv, sign, width, height, fw, fh, xpos, ypos, bip);
  const int centre = sp.ver_frac == 2 && sp.hor_frac == 2 && bip < 2;
  const int outside = !(sp.hor_int - 2 >= win.ox && sp.hor_int + width + 6 <= win.ox + win.Ww && sp.ver_int - 2 >= win.oy && sp.ver_int + height + 3 <= win.oy + win.Wh);
  if (team_ballot(t, outside) != 0ull) return kNone;
  const int dual = team_ballot(t, centre) != 0ull;   // wave-uniform
  auto pair = [](int a, int b) -> uint32_t { return (uint32_t)(uint16_t)(int16_t)a | ((uint32_t)(uint16_t)(int16_t)b << 16); };
  uint32_t tA[3], tB[3];
  for (int q = 0; q < 3; q++) {
    tA[q] = centre ? (q == 1 ? pair(1, 1) : 0u) : pair(sp.th[2 * q], sp.th[2 * q + 1]);                                        // rows 0, 1, 4, 5: {0,0,1,1,0,0}
    tB[q] = centre ? (q == 0 ? pair(0, 1) : q == 1 ? pair(2, 2) : pair(1, 0)) : pair(sp.th[2 * q], sp.th[2 * q + 1]);         // rows 2, 3:       {0,1,2,2,1,0}
  }
  int tv[6];
  for (int m = 0; m < 6; m++) tv[m] = centre ? (m >= 1 && m <= 4 ? 1 : 0) : sp.tv[m];
  const int rnd = centre ? 8 : 2048, rsh = centre ? 4 : 12;
  const int lgw = ilog2((unsigned)width);
  const int SH = height == 4 ? 4 : 8;
  const int units = width * (height == 4 ? 1 : (height >> 3));
  unsigned sad = 0;
  auto strip = [&](auto sh_tag, auto dual_tag, int i0, int j) {
    constexpr int SHC = decltype(sh_tag)::value, DUAL = decltype(dual_tag)::value, NR = SHC + 5;
    const int woff = mul24(i0 + sp.ver_int - 2 - win.oy, win.pitch) + ((j + sp.hor_int - 2 - win.ox) << 1);   // bytes
    int hA[NR], hB[NR];
    TK_UNROLL
    for (int r = 0; r < NR; r++) {
      const Seg16 sg = win_seg<12>(win.w32, woff + mul24(r, win.pitch));   // six samples
      hA[r] = dot2_i16(tA[0], sg.d[0], dot2_i16(tA[1], sg.d[1], dot2_i16(tA[2], sg.d[2], 0)));
      if constexpr (DUAL) hB[r] = dot2_i16(tB[0], sg.d[0], dot2_i16(tB[1], sg.d[1], dot2_i16(tB[2], sg.d[2], 0)));
      else hB[r] = hA[r];
    }
    TK_UNROLL
    for (int q = 0; q < SHC; q++) {
      int sum = mul24(tv[0], hA[q]) + mul24(tv[1], hA[q + 1]) + mul24(tv[2], hB[q + 2]) + mul24(tv[3], hB[q + 3]) + mul24(tv[4], hA[q + 4]) + mul24(tv[5], hA[q + 5]);
      const int pr = sat_pix((sum + rnd) >> rsh, bitdepth);
      const int o = (int)spc<SP>(org_)[mul24(i0 + q, ostride) + j];
      sad += (unsigned)(o > pr ? o - pr : pr - o);
    }
  };
  struct S4 { enum { value = 4 }; };
  struct S8 { enum { value = 8 }; };
  struct D0 { enum { value = 0 }; };
  struct D1 { enum { value = 1 }; };
  for (int u = part; u < units; u += 8) {
    const int j = u & (width - 1), i0 = (u >> lgw) << 3;
    if (SH == 4) { if (dual) strip(S4(), D1(), 0, j); else strip(S4(), D0(), 0, j); }
    else { if (dual) strip(S8(), D1(), i0, j); else strip(S8(), D0(), i0, j); }
  }
  const unsigned tot = (unsigned)team_group_sum(t, (int)sad, 8);
  const unsigned cost = (tot >> (bitdepth - 8)) + mv_cost(lam, mv.y - mvp.y, mv.x - mvp.x);
  unsigned k = (cost << 8) | (unsigned)c;
  if (part != 0) k = ~0u;
  return team_min32(t, k);
}
}  // namespace tk
