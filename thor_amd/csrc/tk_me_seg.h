// tk_me_seg.h - motion-search workspace, vector cost and the row-segment evaluator: MeLists, MeWs, eval_min, Seg16, MeWin, seg_sads, eval_fullpel, MeArgs, uniform.
#pragma once
#include "tk_common.h"
#include "tk_pred.h"
#include "tk_xform.h"

namespace tk {
enum { kMeWideChunk = 12, kMeMaxCand = kMeWideChunk * 5 };  // 5-offset SADs are evaluated 12 candidates at a time

// per-SB candidate lists (frame_info.mvcand[], enc/mainenc.h:146-148), reset per SB.  One instance per workgroup:
// the list of reference r is only ever touched by the wavefront that is searching reference r at that moment.
struct MeLists {
  mv_t mvcand[kMaxRefs][64];
  int mvcand_num[kMaxRefs];
  unsigned long long mvcand_mask[kMaxRefs];
  int best_ref;  // frame_info.best_ref (enc/mainenc.h:143): per-SB state of the encoder_speed 2 reference shortcut
};
struct MeWs {  // per wavefront
  int sad[kMeMaxCand];
  mv_t cmv[64];
  MeLists* lists;
  long long* prof;
  uint32_t* win;  // per-wave LDS for the search window (see MeWin below), nullptr: none
  int win_cap;    // its size in bytes
  // A window staged for a whole coding block (me_stage_cb_window): the searches of a reference's HOR / VER / QUAD partitions all start from
  // the same centre, so one (CB + 2R)^2 window serves all eight of them.  cwin_ax / cwin_ay: absolute luma position of its first sample.
  int cwin_valid, cwin_ref, cwin_ax, cwin_ay, cwin_Ww, cwin_Wh, cwin_pitch;
};
TK_DEV int mv_len1(int a) {
  // (selects on values computed up front: as early returns this compiled to four nested exec-masked branches per vector component and candidate)
  a = iabs(a);
  const int big = 10 + ((a - 36) >> 4) + 1;   // a >= 36
  const int mid = 5 + ((a - 4) >> 3) + 1;     // 4 <= a < 36
  int r = a < 36 ? mid : big;
  r = a < 4 ? 5 : r;
  r = a < 2 ? 4 : r;
  r = a < 1 ? 2 : r;
  return r;
}
TK_DEV int quote_mv_bits(int dy, int dx) { return mv_len1(dx) + mv_len1(dy); }
TK_DEV unsigned mv_cost(double lam, int dy, int dx) {
  return (unsigned)mul_add_nofma(lam, (double)quote_mv_bits(dy, dx), 0.5);
}
// add_mvcandidate (encode_block.c:69-82) - call from ONE lane.
TK_DEV void add_mvcand(MeWs* w_, int r, mv_t mv) {
  const auto w = ldsc(lds_ld(&w_->lists));
  mv_t imv = mk_mv((mv.x + 2) >> 2, (mv.y + 2) >> 2);
  unsigned long long m = 1ull << ((((int)imv.y << 3) ^ (int)imv.x) & 63);
  if (!(m & w->mvcand_mask[r])) {
    const int n = w->mvcand_num[r];
    w->mvcand[r][n].x = imv.x; w->mvcand[r][n].y = imv.y;
    w->mvcand_num[r] = n + 1;
  }
  w->mvcand_mask[r] |= m;
}

// Evaluate n candidates and return min over (cost << 32 | index): the first candidate in evaluation
// order among those with the smallest cost - exactly the winner of the reference's sequential
// "if (cost < min) ..." scan.  prep(c) -> per-candidate context, item(ctx, r) -> partial SAD of work
// item r < nit, cost(c, ctx, sad) -> cost.  G lanes share a candidate, partial sums are combined with
// xor-shuffles, the final minimum with a 64-bit wave reduction; no LDS traffic, no barriers.
template <class PrepF, class ItemF, class CostF>
TK_DEV unsigned long long eval_min(const Team t, int n, int nit, PrepF prep, ItemF item, CostF cost) {
  const int G = nit < t.size ? nit : t.size;
  const int P = t.size / G;
  const int slot = t.rank / G, sub = t.rank - slot * G;
  unsigned long long best = ~0ull;
  for (int c0 = 0; c0 < n; c0 += 2 * P) {
    const int ca = c0 + slot, cb = c0 + P + slot;
    const int va = ca < n, vb = cb < n;
    auto xa = prep(va ? ca : 0);
    auto xb = prep(vb ? cb : 0);
    int la = 0, lb = 0;
    if (va) for (int r = sub; r < nit; r += G) la += item(xa, r);
    if (vb) for (int r = sub; r < nit; r += G) lb += item(xb, r);
    la = team_group_sum(t, la, G); lb = team_group_sum(t, lb, G);
    if (sub == 0) {
      if (va) { unsigned long long k = ((unsigned long long)cost(ca, xa, la) << 32) | (unsigned)ca; best = k < best ? k : best; }
      if (vb) { unsigned long long k = ((unsigned long long)cost(cb, xb, lb) << 32) | (unsigned)cb; best = k < best ? k : best; }
    }
  }
  return TKU64(team_min64(t, best));
}

// Row segment of a block: up to 16 bytes (16 8-bit / 8 16-bit samples) held in four dwords, unused dwords zero.
struct Seg16 { uint32_t d[4]; };
#if !TK_HOST
typedef uint32_t __attribute__((ext_vector_type(4))) u32x4;
typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
typedef u32x4 __attribute__((aligned(1), may_alias)) u32x4_unaligned;
typedef u32x2 __attribute__((aligned(1), may_alias)) u32x2_unaligned;
#endif
// NB (4, 8 or 16) bytes at p.  SP: address space of p; LDS / scratch blocks are aligned to the segment size, frame planes
// (global) may be read at any byte offset.
template <int SP, int NB> TK_DEV Seg16 seg_load(const void* p) {
  Seg16 r;
  r.d[0] = r.d[1] = r.d[2] = r.d[3] = 0;
#if TK_HOST
  __builtin_memcpy(&r, p, (size_t)NB);
#else
  if constexpr (SP == SP_LDS) {
    const auto q = (const TK_LDS uint8_t*)(uint32_t)(uintptr_t)p;
    if constexpr (NB == 16) { const u32x4 v = *(const TK_LDS u32x4*)q; r.d[0] = v.x; r.d[1] = v.y; r.d[2] = v.z; r.d[3] = v.w; }
    else if constexpr (NB == 8) { const u32x2 v = *(const TK_LDS u32x2*)q; r.d[0] = v.x; r.d[1] = v.y; }
    else r.d[0] = *(const TK_LDS uint32_t*)q;
  } else {
    const auto q = (const TK_GLOBAL uint8_t*)p;
    if constexpr (NB == 16) { const u32x4 v = *(const TK_GLOBAL u32x4_unaligned*)q; r.d[0] = v.x; r.d[1] = v.y; r.d[2] = v.z; r.d[3] = v.w; }
    else if constexpr (NB == 8) { const u32x2 v = *(const TK_GLOBAL u32x2_unaligned*)q; r.d[0] = v.x; r.d[1] = v.y; }
    else r.d[0] = *(const TK_GLOBAL u32_unaligned*)q;
  }
#endif
  return r;
}
// sum of absolute sample differences of two NB-byte segments, added to acc
template <typename PIX, int NB> TK_DEV int seg_sad(const Seg16& a, const Seg16& b, int acc) {
#if TK_HOST
  const PIX* x = (const PIX*)a.d;
  const PIX* y = (const PIX*)b.d;
  for (int k = 0; k < (int)(NB / sizeof(PIX)); k++) acc += iabs((int)x[k] - (int)y[k]);
  return acc;
#else
  unsigned s = (unsigned)acc;
  if constexpr (sizeof(PIX) == 1) { for (int k = 0; k < NB / 4; k++) s = __builtin_amdgcn_sad_u8(a.d[k], b.d[k], s); }    // 4 samples per lane-op
  else { for (int k = 0; k < NB / 4; k++) s = __builtin_amdgcn_sad_u16(a.d[k], b.d[k], s); }                             // 2 samples per lane-op
  return (int)s;
#endif
}

// Truncating average (a + b) >> 1 per sample of two segments (bi-prediction, inter_prediction.c:228-247): per dword
// (a & b) + (((a ^ b) >> 1) & M), M = every bit but each sample's top one.
template <typename PIX> TK_DEV Seg16 seg_avg(const Seg16& a, const Seg16& b) {
  const uint32_t M = sizeof(PIX) == 1 ? 0x7f7f7f7fu : 0x7fff7fffu;
  Seg16 r;
  for (int k = 0; k < 4; k++) r.d[k] = (a.d[k] & b.d[k]) + (((a.d[k] ^ b.d[k]) >> 1) & M);
  return r;
}
// A candidate type with a second reference pointer `p2` is bi-predicted: its block is the truncating average of the blocks at p and p2
// (same stride); such candidates always read the planes.
template <class T, class = void> struct CandHasP2 { enum { value = 0 }; };
template <class T> struct CandHasP2<T, decltype((void)((T*)nullptr)->p2)> { enum { value = 1 }; };

// LDS search window of one motion search: the (w + 2R) x (h + 2R) samples of the reference plane around the search centre, staged
// once per search with coalesced 16-byte row loads; the telescope, candidate-list, 5-offset, hexagon and sub-pel passes whose
// blocks lie inside read it with aligned ds_read + v_alignbyte instead of gathering from the vector L1 (one coalesced global
// round trip per search instead of one gather round trip per pass; profiles/r03_ubench_l1gather.log).  Samples of 1 or 2 bytes;
// the reach R is the largest multiple of 4 up to kMeWinR for which the window fits the wave's LDS budget (MeWs::win_cap), at
// least kMeWinRmin - otherwise the search reads the plane.  Row pitch = row bytes + 4: consecutive rows start in different banks.
// Origin (ox, oy) is relative to the PU's co-located position in the reference plane.  The window lives in the wave's transform
// workspace (idle during a search) and the bytes that follow it (SmallWs::win_extra).
struct MeWin {
  const uint32_t* w32;
  int ox, oy, Ww, Wh;   // samples
  int pitch;            // bytes
  int on;
};
enum { kMeWinR = 20, kMeWinRmin = 8 };
TK_DEV int me_win_bytes(int w, int h, int R, int S) { return ((w + 2 * R) * S + 4) * (h + 2 * R) + 4; }
// NB bytes at byte offset `off` of the window (any alignment): NB/4 + 1 aligned dwords, funnel-shifted
template <int NB> TK_DEV Seg16 win_seg(const uint32_t* w32, int off) {
  Seg16 r;
  r.d[0] = r.d[1] = r.d[2] = r.d[3] = 0;
  const int d = off >> 2;
  const unsigned sh = (unsigned)(off & 3);
  uint32_t a[NB / 4 + 1];
#if TK_HOST
  for (int k = 0; k <= NB / 4; k++) a[k] = w32[d + k];
  for (int k = 0; k < NB / 4; k++) r.d[k] = (uint32_t)((((unsigned long long)a[k + 1] << 32) | a[k]) >> (8 * sh));
#else
  const TK_LDS uint32_t* l = (const TK_LDS uint32_t*)(uint32_t)(uintptr_t)w32 + d;
  TK_UNROLL
  for (int k = 0; k <= NB / 4; k++) a[k] = l[k];
  TK_UNROLL
  for (int k = 0; k < NB / 4; k++) r.d[k] = __builtin_amdgcn_alignbyte(a[k + 1], a[k], sh);
#endif
  return r;
}

// Core of the full-pel passes: SAD of the org block against n candidate blocks; sink(c, x, sad, mine) is called in every lane
// for every evaluated candidate slot (mine = this lane reports candidate c: first lane of its group, c < n).
// Work item = one row segment of a candidate block (up to 16 bytes: ONE memory instruction per lane instead of one per four
// samples).  PUs of up to `team size` segments (8-bit: everything up to 32x32): one segment per lane and candidate,
// G = segments-per-candidate lanes form a group, team/G candidates are evaluated side by side and up to four such candidate
// sets are in flight per lane; the group sum is a DPP butterfly.  Larger PUs: the whole team works on one candidate, four
// segments per lane in flight.  cand(c) -> {clipped mv, displacement (dx, dy), pointer to the displaced reference block}.
// An iteration whose candidate blocks all lie inside the staged window reads LDS, otherwise the reference plane.
// One iteration of the small-PU path: U candidate sets (U * P candidates) starting at candidate c0.  Straight-line code: the
// U reference segments are fetched back to back (window or plane, decided once for all of them) before the first SAD; slots
// beyond n evaluate candidate 0 and are masked out in the sink.
template <int SP, typename PIX, int NB, int U, class CandF, class SinkF>
TK_DEV void seg_sads_iter(const Team t, int n, int c0, int P, int G, int slot, int sub, const Seg16& o, int roff, int woff, int width, int height,
                          const MeWin& win, CandF cand, SinkF sink) {
  Seg16 r[U];
  decltype(cand(0)) x[U];
  int outside = 0;
  TK_UNROLL
  for (int u = 0; u < U; u++) {
    const int c = c0 + u * P + slot;
    x[u] = cand(c < n ? c : 0);
    outside |= !(x[u].dx >= win.ox && x[u].dx + width <= win.ox + win.Ww && x[u].dy >= win.oy && x[u].dy + height <= win.oy + win.Wh);
  }
  enum { BI = CandHasP2<decltype(cand(0))>::value };
  const int use_win = !BI && win.on && team_ballot(t, outside) == 0ull;
  if (use_win) {
    TK_UNROLL
    for (int u = 0; u < U; u++) r[u] = win_seg<NB>(win.w32, mul24(x[u].dy, win.pitch) + x[u].dx * (int)sizeof(PIX) + woff);
  } else {
    TK_UNROLL
    for (int u = 0; u < U; u++) r[u] = seg_load<SP_GLOBAL, NB>(x[u].p + roff);
    if constexpr (BI) {
      TK_UNROLL
      for (int u = 0; u < U; u++) r[u] = seg_avg<PIX>(r[u], seg_load<SP_GLOBAL, NB>(x[u].p2 + roff));
    }
  }
  TK_UNROLL
  for (int u = 0; u < U; u++) {
    const int c = c0 + u * P + slot;
    const int sad = team_group_sum(t, seg_sad<PIX, NB>(o, r[u], 0), G);
    sink(c, x[u], sad, c < n && sub == 0);
  }
}
template <int SP, typename PIX, int NB, class CandF, class SinkF>
TK_DEV void seg_sads_nb(const Team t, int n_, const PIX* org, int ostride, int rstride, int width, int height, const MeWin& win,
                        CandF cand, SinkF sink) {
  // wave-uniform scalars (function arguments arrive in vector registers: without this every branch below is exec-mask code)
  const int n = TKU(n_), tsz = TKU(t.size);
  const int lw = NB / (int)sizeof(PIX);              // samples per segment
  const int lgr = TKU(ilog2((unsigned)(width / lw)));   // log2(segments per row)
  const int nit = height << lgr;                       // segments per candidate
  const int G = nit < tsz ? nit : tsz;                 // powers of two
  const int lgG = TKU(ilog2((unsigned)G));
  const int P = tsz >> lgG;
  const int slot = t.rank >> lgG, sub = t.rank & (G - 1);
  if (nit <= tsz) {
    const int i = sub >> lgr, j = (sub & ((1 << lgr) - 1)) * lw;
    // (24-bit multiplies throughout the passes: row / pitch products are small, and v_mul_lo_u32 runs at a quarter of the rate)
    const Seg16 o = seg_load<SP, NB>(org + mul24(i, ostride) + j);
    const int roff = mul24(i, rstride) + j;
    const int woff = mul24(i - win.oy, win.pitch) + (j - win.ox) * (int)sizeof(PIX);   // bytes
    if (n <= P) seg_sads_iter<SP, PIX, NB, 1>(t, n, 0, P, G, slot, sub, o, roff, woff, width, height, win, cand, sink);
    else if (n <= 2 * P) seg_sads_iter<SP, PIX, NB, 2>(t, n, 0, P, G, slot, sub, o, roff, woff, width, height, win, cand, sink);
    else
      for (int c0 = 0; c0 < n; c0 += 4 * P) seg_sads_iter<SP, PIX, NB, 4>(t, n, c0, P, G, slot, sub, o, roff, woff, width, height, win, cand, sink);
  } else {
    const int ipl = nit >> lgG;  // a multiple of 4 except on teams smaller than a wavefront (host simulation)
    for (int c = 0; c < n; c++) {
      const auto x = cand(c);
      // the whole wave works on this candidate: one wave-uniform decision whether its block lies inside the staged window
      const int use_win = TKU(!CandHasP2<decltype(cand(0))>::value && win.on && x.dx >= win.ox && x.dx + width <= win.ox + win.Ww && x.dy >= win.oy && x.dy + height <= win.oy + win.Wh);
      const int wbase = mul24(x.dy - win.oy, win.pitch) + (x.dx - win.ox) * (int)sizeof(PIX);
      int sad = 0;
      for (int k0 = 0; k0 < ipl; k0 += 4) {
        Seg16 o[4], r[4];
        TK_UNROLL
        for (int k = 0; k < 4; k++)
          if (k0 + k < ipl) {
            const int q = sub + (k0 + k) * G, i = q >> lgr, j = (q & ((1 << lgr) - 1)) * lw;
            o[k] = seg_load<SP, NB>(org + mul24(i, ostride) + j);
            if (use_win) r[k] = win_seg<NB>(win.w32, wbase + mul24(i, win.pitch) + j * (int)sizeof(PIX));
            else r[k] = seg_load<SP_GLOBAL, NB>(x.p + mul24(i, rstride) + j);
            if constexpr (CandHasP2<decltype(cand(0))>::value) r[k] = seg_avg<PIX>(r[k], seg_load<SP_GLOBAL, NB>(x.p2 + mul24(i, rstride) + j));
          }
        TK_UNROLL
        for (int k = 0; k < 4; k++)
          if (k0 + k < ipl) sad = seg_sad<PIX, NB>(o[k], r[k], sad);
      }
      sad = team_group_sum(t, sad, G);
      sink(c, x, sad, sub == 0);
    }
  }
}
template <int SP, typename PIX, class CandF, class SinkF>
TK_DEV void seg_sads(const Team t, int n, const PIX* org, int ostride, int rstride, int width, int height, const MeWin& win, CandF cand, SinkF sink) {
  const int nb = (width < 16 / (int)sizeof(PIX) ? width : 16 / (int)sizeof(PIX)) * (int)sizeof(PIX);  // bytes per row segment
  if (nb == 16) seg_sads_nb<SP, PIX, 16>(t, n, org, ostride, rstride, width, height, win, cand, sink);
  else if (nb == 8) seg_sads_nb<SP, PIX, 8>(t, n, org, ostride, rstride, width, height, win, cand, sink);
  else seg_sads_nb<SP, PIX, 4>(t, n, org, ostride, rstride, width, height, win, cand, sink);
}
// Full-pel candidate evaluation: min over the n candidates of (cost << 32 | index) - the first candidate in evaluation order
// among those with the smallest cost, i.e. the winner of the reference's sequential strict-'<' scan.
template <int SP, typename PIX, class CandF, class CostF>
TK_DEV unsigned long long eval_fullpel(const Team t, int n, const PIX* org, int ostride, int rstride, int width, int height,
                                       const MeWin& win, CandF cand, CostF cost) {
  // Costs fit 24 bits - the SAD is at most 128 * 128 * 255 after the bit-depth shift, the vector cost at most sqrt(lambda) * 2 * mv_len1(65535) <
  // 120 * 8208 - and n <= 64: the minimum over (cost << 8 | index) is ONE 32-bit wave reduction (4 DPP v_min + 4 v_readlane) instead of a 64-bit
  // one; the host simulation asserts the bound.
  unsigned best32 = ~0u;
  seg_sads<SP>(t, n, org, ostride, rstride, width, height, win, cand, [&](int c, const decltype(cand(0))& x, int sad, int mine) {
    const unsigned cst = cost(x, sad);
#if TK_HOST
    if (mine && ((cst >> 24) != 0u || c > 255)) { fprintf(stderr, "eval_fullpel: cost %u / index %d does not fit the packed key\n", cst, c); abort(); }
#endif
    unsigned k32 = (cst << 8) | (unsigned)c;
    if (!mine) k32 = ~0u;
    best32 = k32 < best32 ? k32 : best32;
  });
  const unsigned m = team_min32(t, best32);
  return m == ~0u ? ~0ull : (((unsigned long long)(m >> 8)) << 32) | (m & 0xffu);
}

struct MeArgs {
  int cb_size;           // `size` argument of motion_estimate = CB size
  int ostride;           // stride of the original-sample block
  int width, height;     // PU dims
  int rstride;
  int sign, fwidth, fheight, xpos, ypos;  // CB position (Appendix B.16)
  int pu_x, pu_y;        // PU position (absolute, luma samples): only the LDS search window needs it
  int enable_bipred, bitdepth;
  int speed;             // encoder_speed (0 slow .. 2 fast)
  double lam;            // sqrt(lambda)
};
// Wave-uniform copies: every field through readfirstlane (scalar registers on the device; the host simulation checks that the lanes agree).
TK_DEV mv_t uniform(mv_t m) { return mk_mv(tk_uniform(m.x), tk_uniform(m.y)); }
TK_DEV MeArgs uniform(const MeArgs& a) {
  MeArgs u;
  u.cb_size = tk_uniform(a.cb_size); u.ostride = tk_uniform(a.ostride); u.width = tk_uniform(a.width);
  u.height = tk_uniform(a.height); u.rstride = tk_uniform(a.rstride); u.sign = tk_uniform(a.sign);
  u.fwidth = tk_uniform(a.fwidth); u.fheight = tk_uniform(a.fheight); u.xpos = tk_uniform(a.xpos);
  u.ypos = tk_uniform(a.ypos); u.enable_bipred = tk_uniform(a.enable_bipred); u.bitdepth = tk_uniform(a.bitdepth);
  u.speed = tk_uniform(a.speed); u.lam = tk_uniform_f64(a.lam);
  u.pu_x = tk_uniform(a.pu_x); u.pu_y = tk_uniform(a.pu_y);
  return u;
}
TK_DEV MeWin uniform(const MeWin& w) {
  MeWin u;
  u.w32 = tk_uniform_ptr(w.w32); u.ox = tk_uniform(w.ox); u.oy = tk_uniform(w.oy); u.Ww = tk_uniform(w.Ww);
  u.Wh = tk_uniform(w.Wh); u.pitch = tk_uniform(w.pitch); u.on = tk_uniform(w.on);
  return u;
}
}  // namespace tk
