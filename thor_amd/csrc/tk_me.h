// tk_me.h - motion search for one prediction unit, team-cooperative.
// Specification followed: enc/encode_block.c:517-711 (motion_estimate, encoder_speed 0 path:
// telescope 32/16/8/4, per-SB candidate list with the 5-offset "widesad" for 16x16 CBs, hexagon
// refinement, 8 half-pel + 8 quarter-pel positions), :467-515 (quote_mv_bits), :417-453
// (sad_calc / widesad_calc), :69-82 (add_mvcandidate).  Every stage evaluates its candidates in
// parallel and then picks the winner by scanning costs in the reference's evaluation order with
// strict '<', which reproduces the sequential tie-breaking exactly.
#pragma once
// The parts below the searches, in dependency order (definition order inside namespace tk is the order of the code object); the
// searches themselves - me_stage_cb_window, motion_estimate, motion_estimate_bi - follow here.
#include "tk_me_seg.h"
#include "tk_me_lanes.h"
#include "tk_me_fastsub.h"

namespace tk {

// Stage ONE window for the coding block at (cb_x, cb_y) of size cb in reference `ref_idx` (ref_cb = its co-located sample in the padded
// plane), centred on the rounded search centre mvc: the HOR / VER / QUAD searches of this reference (eight motion_estimate calls) all start
// from it and find their window in LDS (motion_estimate: use_cb_win).  No window (cwin_valid = 0) when it does not fit the wave's budget
// with a reach of at least kMeWinRmin or would leave the padded plane.  The caller clears cwin_valid before the transform workspace is
// used again.
template <typename PIX>
TK_DEV void me_stage_cb_window(const Team t, MeWs* w_, const PIX* ref_cb, int rstride, int cb_x, int cb_y, int cb, mv_t mvc, int sign, int fwidth,
                               int fheight, int ref_idx) {
  const auto w = ldsc(w_);
  const int S = (int)sizeof(PIX), s = sign ? -1 : 1;
  const int cap = TKU(w->win_cap);
  int R = kMeWinR;
  while (R >= kMeWinRmin && me_win_bytes(cb, cb, R, S) > cap) R -= 4;
  const mv_t mv_ref = mk_mv(((mvc.x + 2) >> 2) << 2, ((mvc.y + 2) >> 2) << 2);
  const int Ww = cb + 2 * R, Wh = cb + 2 * R, pitch = Ww * S + 4;
  const int ox = s * (mv_ref.x >> 2) - R, oy = s * (mv_ref.y >> 2) - R;
  const int ok = TKU(w->win != nullptr && R >= kMeWinRmin && cb_x + ox >= -kPadY && cb_x + ox + Ww <= fwidth + kPadY && cb_y + oy >= -kPadY &&
                     cb_y + oy + Wh <= fheight + kPadY);
  t.sync();
  if (ok) {
    const uint32_t* w32 = lds_ld(&w_->win);
    const int rowb = Ww * S, spr = (rowb + 15) >> 4, total = spr * Wh;
    for (int k0 = 0; k0 < total; k0 += t.size) {
      const int k = k0 + t.rank;
      if (k < total) {
        const int row = k / spr, sg = k - row * spr;
        const Seg16 v = seg_load<SP_GLOBAL, 16>((const char*)(ref_cb + (oy + row) * rstride + ox) + 16 * sg);
        const int d = (row * pitch + 16 * sg) >> 2;
        const int nd = tmin(4, (rowb - 16 * sg) >> 2);
#if TK_HOST
        for (int q = 0; q < nd; q++) ((uint32_t*)w32)[d + q] = v.d[q];
#else
        TK_LDS uint32_t* l = (TK_LDS uint32_t*)(uint32_t)(uintptr_t)w32 + d;
        l[0] = v.d[0];
        if (nd > 1) l[1] = v.d[1];
        if (nd > 2) l[2] = v.d[2];
        if (nd > 3) l[3] = v.d[3];
#endif
      }
    }
  }
  if (t.rank == 0) {
    w->cwin_valid = ok; w->cwin_ref = ref_idx; w->cwin_ax = cb_x + ox; w->cwin_ay = cb_y + oy; w->cwin_Ww = Ww; w->cwin_Wh = Wh; w->cwin_pitch = pitch;
  }
  t.sync();
}

// SP: address space of the original-sample block `org` (LDS copy for coding blocks up to kLdsBlk and their 2*org-pred
// blocks, frame plane / global scratch above); w always lives in LDS on the device.
template <typename PIX, int SP>
TK_DEVNI unsigned motion_estimate(const Team t, MeWs* w_, const PIX* org, const PIX* ref, const MeArgs& a_in, mv_t mvc,
                                mv_t mvp, int ref_idx, mv_t* mv_out) {
  TK_PROF_T0();
#if TK_PROF_ME
  const long long pme0_ = (long long)__builtin_readcyclecounter();
#endif
  const auto w = ldsc(w_);
  const auto lists = ldsc(lds_ld(&w_->lists));
  const auto orgs = spc<SP>(org);
  auto cmv_get = [&](int c) -> mv_t { return mk_mv(w->cmv[c].x, w->cmv[c].y); };
  auto cmv_set = [&](int c, mv_t m) { w->cmv[c].x = m.x; w->cmv[c].y = m.y; };
  const MeArgs a = uniform(a_in);
  mvc = uniform(mvc);
  mvp = uniform(mvp);
  ref_idx = tk_uniform(ref_idx);
  const int s = a.sign ? -1 : 1;
  const int sh = a.bitdepth - 8;
  unsigned min_sad = kCostInit;
  mv_t mv_opt = mk_mv(0, 0);
  mv_t mv_ref = mk_mv(((mvc.x + 2) >> 2) << 2, ((mvc.y + 2) >> 2) << 2);
  // (rate: the vector's rate term, formed with the candidate - before its samples are waited for - not after the SAD)
  struct FP { mv_t mv; const PIX* p; int dx, dy; unsigned rate; };
  // (A table in LDS for the rate term - it is a function of a small bit count and of a per-frame constant - was measured SLOWER by 13 % per
  // call, tools/ubench_me.cpp / profiles/r05_ubench_me.md: the range check is a wave vote + branch per candidate, which serialises the four
  // candidate sets of an evaluator iteration; the double-precision chain pipelines across them.)
  auto rate_of = [&](mv_t m) -> unsigned { return mv_cost(a.lam, m.y - mvp.y, m.x - mvp.x); };
  auto fp_cost = [&](const FP& x, int sad) -> unsigned { return ((unsigned)sad >> sh) + x.rate; };
  // clip_mv leaves every vector within +-R quarter-pels of `ctr` alone when the block displaced by any of them stays inside
  // the padded area (one wave-uniform test per pass instead of four clamps per candidate; conservative for the
  // truncating division of clip_mv)
  auto clip_free = [&](mv_t ctr, int R) -> int {
    const int ext = kPadY - 16, cy = s * ctr.y, cx = s * ctr.x;
    return a.ypos + ((cy - R) >> 2) >= -ext && a.ypos + ((cy + R + 3) >> 2) + a.cb_size <= a.fheight + ext &&
           a.xpos + ((cx - R) >> 2) >= -ext && a.xpos + ((cx + R + 3) >> 2) + a.cb_size <= a.fwidth + ext;
  };
  auto mk_fp = [&](mv_t mv, int noclip) -> FP {
    FP x;
    x.mv = noclip ? mv : clip_mv(mv, a.ypos, a.xpos, a.fwidth, a.fheight, a.cb_size, a.cb_size, a.sign);
    x.dx = s * (x.mv.x >> 2);
    x.dy = s * (x.mv.y >> 2);
    x.p = ref + mul24(x.dy, a.rstride) + x.dx;
    x.rate = rate_of(x.mv);
    return x;
  };
#if TK_PROF_MACROS
  long long pq_ = (long long)__builtin_readcyclecounter();
  if (t.rank == 0) w->prof[11] += 1;
#endif
  // --- stage the search window in LDS (see MeWin): Wh rows of Ww bytes around the search centre with 16-byte row loads.  Only
  // when the whole window lies inside the padded reference plane (otherwise every pass of this search reads the plane).
  MeWin win;
  win.on = 0; win.w32 = nullptr; win.ox = win.oy = win.Ww = win.Wh = win.pitch = 0;
  const int use_cb_win = TKU(w->cwin_valid && w->cwin_ref == ref_idx && a.speed == 0);
  if (use_cb_win) {   // the block's window is already in LDS (me_stage_cb_window): this PU's view of it
    win.Ww = TKU(w->cwin_Ww); win.Wh = TKU(w->cwin_Wh); win.pitch = TKU(w->cwin_pitch);
    win.ox = TKU(w->cwin_ax) - a.pu_x; win.oy = TKU(w->cwin_ay) - a.pu_y;
    win.w32 = lds_ld(&w_->win);
    win.on = 1;
  } else {
    const int S = (int)sizeof(PIX);
    const int cap = TKU(w->win_cap);
    int R = kMeWinR;
    while (R >= kMeWinRmin && me_win_bytes(a.width, a.height, R, S) > cap) R -= 4;   // wave-uniform
    if (w->win && R >= kMeWinRmin && a.speed == 0) {
      win.Ww = a.width + 2 * R; win.Wh = a.height + 2 * R; win.pitch = win.Ww * S + 4;
      win.ox = s * (mv_ref.x >> 2) - R; win.oy = s * (mv_ref.y >> 2) - R;
      win.w32 = lds_ld(&w_->win);
      win.on = TKU(a.pu_x + win.ox >= -kPadY && a.pu_x + win.ox + win.Ww <= a.fwidth + kPadY && a.pu_y + win.oy >= -kPadY &&
                   a.pu_y + win.oy + win.Wh <= a.fheight + kPadY);
    }
    if (win.on) {
      const int rowb = win.Ww * S;   // a multiple of 4
      const int spr = (rowb + 15) >> 4, total = spr * win.Wh;   // 16-byte segments per row; the last one may read past the row (inside the plane's allocation)
      t.sync();
      for (int k0 = 0; k0 < total; k0 += t.size) {
        const int k = k0 + t.rank;
        if (k < total) {
          const int row = k / spr, sg = k - row * spr;
          const Seg16 v = seg_load<SP_GLOBAL, 16>((const char*)(ref + (win.oy + row) * a.rstride + win.ox) + 16 * sg);
          const int d = (row * win.pitch + 16 * sg) >> 2;
          const int nd = tmin(4, (rowb - 16 * sg) >> 2);   // dwords of this segment that belong to the row
#if TK_HOST
          for (int q = 0; q < nd; q++) ((uint32_t*)win.w32)[d + q] = v.d[q];
#else
          TK_LDS uint32_t* l = (TK_LDS uint32_t*)(uint32_t)(uintptr_t)win.w32 + d;
          l[0] = v.d[0];
          if (nd > 1) l[1] = v.d[1];
          if (nd > 2) l[2] = v.d[2];
          if (nd > 3) l[3] = v.d[3];
#endif
        }
      }
      t.sync();
    }
  }
  // 5-offset "widesad" evaluation of the clipped candidates w->cmv[0..n) (encode_block.c:430-453): per
  // candidate the offset with the smallest SAD (ties -> leftmost), then the usual cost with the adjusted
  // mv (written back to w->cmv).  Returns the best (cost << 32 | index).
  auto eval_wide = [&](int n) -> unsigned long long {
    unsigned long long bestk = ~0ull;
    for (int base = 0; base < n; base += kMeWideChunk) {
      const int m = n - base < kMeWideChunk ? n - base : kMeWideChunk;
      auto widepel = [&](int c5) -> FP {
        int c = mul24(c5, 13) >> 6, o = c5 - c - (c << 2);   // c5 / 5 for c5 < 60
        int off = o == 0 ? -3 : o == 1 ? -1 : o == 2 ? 0 : o == 3 ? 1 : 3;
        FP x;
        x.mv = cmv_get(base + c);
        x.dx = s * (x.mv.x >> 2) + off;
        x.dy = s * (x.mv.y >> 2);
        x.p = ref + mul24(x.dy, a.rstride) + x.dx;
        x.rate = 0;
        return x;
      };
      {
        const auto sadl = ldsc(w_->sad);
        seg_sads<SP>(t, m * 5, org, a.ostride, a.rstride, a.width, a.height, win, widepel, [&](int c5, const FP&, int sad, int mine) { if (mine) sadl[c5] = sad; });
      }
      t.sync();
      unsigned long long k = ~0ull;
      for (int lc = t.rank; lc < m; lc += t.size) {
        const int c = base + lc;
        mv_t mm = cmv_get(c);
        int x = 0;
        unsigned best = 1u << 31;
        for (int o = 0; o < 5; o++) {
          unsigned v = (unsigned)w->sad[lc * 5 + o];
          if (v < best) { best = v; x = o == 0 ? -3 : o == 1 ? -1 : o == 2 ? 0 : o == 3 ? 1 : 3; }
        }
        mm.x = (int16_t)(mm.x + ((s * x) << 2));
        cmv_set(c, mm);  // adjusted mv, looked up again if this candidate wins
        unsigned long long kk = ((unsigned long long)((best >> sh) + mv_cost(a.lam, mm.y - mvp.y, mm.x - mvp.x)) << 32) | (unsigned)c;   // (lanes diverge here: no table)
        k = kk < k ? kk : k;
      }
      t.sync();
      k = TKU64(team_min64(t, k));
      bestk = k < bestk ? k : bestk;
    }
    return bestk;
  };
  // Vectors this search has already evaluated cannot win a later pass: every pass keeps a candidate only on a strict '<'
  // against min_sad, the minimum over everything evaluated so far with the same cost function (same block, same mvp; a
  // vector is clipped the same way whenever it comes up).  The 5x5 grid of a telescope step (spacing `step`) shares its
  // points with even offsets with the previous step's grid (spacing 2*step) - up to 8 of 24; by induction the previous
  // grid is the only one that needs checking.  Passes of PUs that need more than one evaluator iteration for 24 candidates
  // leave those points out (encoder_speed 0; exact: the surviving candidates keep their relative order, so ties resolve the
  // same way); a hexagon refinement that starts on the centre of the last grid would only revisit it and is skipped.
  mv_t g_ctr = mk_mv(0, 0);
  int g_step = 0;   // spacing of the last telescope grid evaluated (0: none)
  // all four grids, for candidates that are not grid points themselves (the per-SB candidate list): a list entry that lies on
  // any of them has been evaluated
  mv_t gc32 = mk_mv(0, 0), gc16 = mk_mv(0, 0), gc8 = mk_mv(0, 0);   // centres of the grids of step 32, 16, 8 (step 4: g_ctr); named
                                                                      // scalars, not an array: nothing here is indexed at run time
  auto on_grid_of = [&](mv_t m, mv_t ctr, int gs) -> int {
    const int dx = m.x - ctr.x, dy = m.y - ctr.y;
    return !((dx | dy) & (gs - 1)) && iabs(dx) <= 2 * gs && iabs(dy) <= 2 * gs;
  };
  auto on_any_grid = [&](mv_t m) -> int {
    // g_step == 4: the telescope has run (all four steps, encoder_speed 0) - the four centres are this search's
    return g_step == 4 && (on_grid_of(m, gc32, 32) | on_grid_of(m, gc16, 16) | on_grid_of(m, gc8, 8) | on_grid_of(m, g_ctr, 4));
  };
  auto on_grid = [&](mv_t m) -> int {
    const int dx = m.x - g_ctr.x, dy = m.y - g_ctr.y;
    return g_step && !((dx | dy) & (g_step - 1)) && iabs(dx) <= 2 * g_step && iabs(dy) <= 2 * g_step;
  };
  const int lw_ = (a.width < 16 / (int)sizeof(PIX)) ? a.width : 16 / (int)sizeof(PIX);   // samples per row segment (seg_sads)
  const int dedup = a.speed == 0 && a.height * (a.width / lw_) >= 16;
  // PUs of up to 32x32 samples, encoder_speed 0: the one-lane-per-candidate full-pel search (me_cand_fullpel; 16-bit samples since round 6) - same passes, same result
  int small_done = 0;
  {
    // (rows of 64 and 128 samples keep the 64-lane evaluator: a lane walking 256+ row segments of the plane by itself measured 2x slower, profiles/r05_ubench_me.md)
    if (TKU(a.speed == 0 && t.size == 64 && a.width <= 32 && a.height <= 32)) {
#ifndef TK_ME_NO_SMALL
      unsigned long long fr;
#define TK_ME_FP_ARGS t, w_, org, ref, a.cb_size, a.ostride, a.width, a.height, a.rstride, a.sign, a.fwidth, a.fheight, a.xpos, a.ypos, a.lam, win.w32, win.ox, win.oy, win.Ww, win.Wh, win.pitch, win.on, mvc, mvp, ref_idx, sh
      const int rowb = a.width * (int)sizeof(PIX);   // bytes per row: the segment size
      if (rowb == 4) { if constexpr (sizeof(PIX) == 1) fr = me_cand_fullpel<PIX, 4, SP>(TK_ME_FP_ARGS); else fr = 0; }
      else if (rowb == 8) fr = me_cand_fullpel<PIX, 8, SP>(TK_ME_FP_ARGS);
      else fr = me_cand_fullpel<PIX, 16, SP>(TK_ME_FP_ARGS);
#undef TK_ME_FP_ARGS
      min_sad = (unsigned)(fr >> 32);
      mv_opt = mk_mv((int16_t)(uint16_t)(fr >> 16), (int16_t)(uint16_t)fr);
      mv_ref = mv_opt;
      small_done = 1;
#endif
    }
  }
#ifdef TK_ME_CROSSCHECK   // test builds: run the generic passes as well and stop the kernel when the two searches disagree
  const int xs_have = small_done;
  const unsigned xs_min = min_sad;
  const mv_t xs_mv = mv_opt;
  if (small_done) { small_done = 0; min_sad = kCostInit; mv_opt = mk_mv(0, 0); mv_ref = mk_mv(((mvc.x + 2) >> 2) << 2, ((mvc.y + 2) >> 2) << 2); }
#endif
  if (!small_done) {
  // --- telescope (encode_block.c:529-561); encoder_speed > 0 keeps it only for 16x16 CBs with bipred on
  if ((a.cb_size == 16 && a.enable_bipred) || a.speed == 0)
  for (int step = 32; step >= 4; step >>= 1) {
    const int n = step < 32 ? 24 : 25;
    const mv_t centre = mv_ref;
    const int noclip = TKU(clip_free(centre, 2 * step));
    auto tele_mv = [&](int c) -> mv_t {
      int idx = (step < 32 && c >= 12) ? c + 1 : c;  // centre skipped after the first step
      int q = mul24(idx, 13) >> 6;                     // idx / 5 for idx < 25 (24-bit multiplies: full rate, v_mul_lo_u32 is a quarter)
      return mk_mv(centre.x + mul24(idx - q - (q << 2) - 2, step), centre.y + mul24(q - 2, step));
    };
    auto tele = [&](int c) -> FP { return mk_fp(tele_mv(c), noclip); };
    if (dedup && g_step) {
      // compact list of the grid points not evaluated before (clipped) in w->cmv, in grid order
      t.sync();
      int cnt = 0;
      for (int c0 = 0; c0 < n; c0 += t.size) {
        const int c = c0 + t.rank;
        const mv_t m = tele_mv(c < n ? c : 0);
        const int keep = c < n && !on_grid(m);
        const unsigned long long mask = team_ballot(t, keep);
        if (keep) cmv_set(cnt + __builtin_popcountll(mask & ((1ull << t.rank) - 1ull)), mk_fp(m, noclip).mv);
        cnt += __builtin_popcountll(mask);
      }
      t.sync();
      cnt = TKU(cnt);
      auto cl = [&](int c) -> FP { return mk_fp(cmv_get(c), 1); };
      unsigned long long k = eval_fullpel<SP>(t, cnt, org, a.ostride, a.rstride, a.width, a.height, win, cl, fp_cost);
      if ((unsigned)(k >> 32) < min_sad) { min_sad = (unsigned)(k >> 32); mv_opt = cmv_get((int)(unsigned)k); }
      t.sync();
    } else
    if (step == 32 && a.cb_size == 16 && a.speed == 1) {  // first ring by widesad at encoder_speed 1
      t.sync();
      for (int c = t.rank; c < n; c += t.size) cmv_set(c, tele(c).mv);
      t.sync();
      unsigned long long k = eval_wide(n);
      if ((unsigned)(k >> 32) < min_sad) { min_sad = (unsigned)(k >> 32); mv_opt = cmv_get((int)(unsigned)k); }
      t.sync();
    } else {
      unsigned long long k = eval_fullpel<SP>(t, n, org, a.ostride, a.rstride, a.width, a.height, win, tele, fp_cost);
      if ((unsigned)(k >> 32) < min_sad) { min_sad = (unsigned)(k >> 32); mv_opt = tele((int)(unsigned)k).mv; }
    }
    g_ctr = centre; g_step = a.speed == 0 ? step : 0;
    if (step == 32) gc32 = centre; else if (step == 16) gc16 = centre; else if (step == 8) gc8 = centre;
    mv_ref = mv_opt;
  }

#if TK_PROF_MACROS
  if (t.rank == 0) w->prof[13] += (long long)__builtin_readcyclecounter() - pq_;
  pq_ = (long long)__builtin_readcyclecounter();
#endif
  // --- candidate list (encode_block.c:564-581)
  {
    const int n = TKU(lists->mvcand_num[ref_idx]);
    if (n > 0) {
      const int wide = a.cb_size == 16;
      for (int c = t.rank; c < n; c += t.size) {
        const mv_t m = mk_mv(lists->mvcand[ref_idx][c].x, lists->mvcand[ref_idx][c].y);
        cmv_set(c, clip_mv(mk_mv(m.x << 2, m.y << 2), a.ypos, a.xpos, a.fwidth, a.fheight, a.cb_size, a.cb_size, a.sign));
      }
      t.sync();
      if (wide) {
        unsigned long long bestk = eval_wide(n);
        if ((unsigned)(bestk >> 32) < min_sad) { min_sad = (unsigned)(bestk >> 32); mv_opt = cmv_get((int)(unsigned)bestk); }
        t.sync();
      } else {
        // Entries that lie on one of the telescope grids have been evaluated (a clipped vector that coincides with a grid point
        // was evaluated as itself: clip_mv is idempotent): the list - previous results of this superblock, clustered around the
        // motion the telescope has just walked to - is compacted in place to the others, in list order (45-56 % go on the test
        // content); nothing left: no pass.
        int cnt = n;
        if (a.speed == 0) {
          cnt = 0;
          for (int c0 = 0; c0 < n; c0 += t.size) {
            const int c = c0 + t.rank;
            const mv_t m = cmv_get(c < n ? c : 0);
            const int keep = c < n && !on_any_grid(m);
            const unsigned long long mask = team_ballot(t, keep);
            t.sync();   // every lane holds its entry before lower slots are rewritten
            if (keep) cmv_set(cnt + __builtin_popcountll(mask & ((1ull << t.rank) - 1ull)), m);
            cnt += __builtin_popcountll(mask);
          }
          t.sync();
          cnt = TKU(cnt);
        }
        if (cnt > 0) {
          auto cl = [&](int c) -> FP { return mk_fp(cmv_get(c), 1); };  // cmv already clipped (clip_mv is idempotent)
          unsigned long long k = eval_fullpel<SP>(t, cnt, org, a.ostride, a.rstride, a.width, a.height, win, cl, fp_cost);
          if ((unsigned)(k >> 32) < min_sad) { min_sad = (unsigned)(k >> 32); mv_opt = cmv_get((int)(unsigned)k); }
        }
        t.sync();
      }
    }
    mv_ref = mv_opt;
  }

#if TK_PROF_MACROS
  if (t.rank == 0) w->prof[14] += (long long)__builtin_readcyclecounter() - pq_;
  pq_ = (long long)__builtin_readcyclecounter();
#endif
  // --- hexagon refinement (encode_block.c:583-616): up to 5 rounds; skipped for CBs > 16 at encoder_speed > 0
  {
    int start = 0, end = 5;
    // all six points around the centre of the last telescope grid (spacing one sample) belong to that grid: nothing to find
    const int revisit = TKU(g_step == 4 && mv_ref.x == g_ctr.x && mv_ref.y == g_ctr.y);
    const int maxsteps = revisit ? 0 : (a.cb_size <= 16 || a.speed == 0) ? 6 : 0;
    for (int step = 1; step < maxsteps; step++) {
      const int n = (end - start + 6) % 6 + 1;  // 6 in the first round, 3 afterwards
      const mv_t centre = mv_ref;
      const int noclip = TKU(clip_free(centre, 8));
      auto hex = [&](int c) -> FP {
        int dir = (start + c) % 6;
        int ox = dir == 0 ? 1 : dir == 1 ? 2 : dir == 2 ? 1 : dir == 3 ? -1 : dir == 4 ? -2 : -1;  // "diy" -> x
        int oy = dir == 0 ? -1 : dir == 1 ? 0 : dir == 2 ? 1 : dir == 3 ? 1 : dir == 4 ? 0 : -1;  // "dix" -> y
        return mk_fp(mk_mv(centre.x + ox * 4, centre.y + oy * 4), noclip);
      };
      int which = -1;
      unsigned long long k = eval_fullpel<SP>(t, n, org, a.ostride, a.rstride, a.width, a.height, win, hex, fp_cost);
      if ((unsigned)(k >> 32) < min_sad) { min_sad = (unsigned)(k >> 32); which = (int)(unsigned)k; mv_opt = hex(which).mv; }
      int best_dir = which < 0 ? -1 : (start + which) % 6;
      mv_ref = mv_opt;
      start = best_dir ? best_dir - 1 : 5;
      end = start + 2;
      end -= (end >= 6) * 6;
      if (best_dir < 0) break;
    }
  }

#if TK_PROF_MACROS
  if (t.rank == 0) w->prof[15] += (long long)__builtin_readcyclecounter() - pq_;
#endif
  }   // !small_done
#ifdef TK_ME_CROSSCHECK
  if (xs_have && (xs_min != min_sad || xs_mv.x != mv_opt.x || xs_mv.y != mv_opt.y)) {
#if TK_HOST
    fprintf(stderr, "me_small8_fullpel disagrees with motion_estimate: %u (%d,%d) vs %u (%d,%d)\n", xs_min, xs_mv.x, xs_mv.y, min_sad, mv_opt.x, mv_opt.y);
    abort();
#else
    __builtin_trap();
#endif
  }
#endif
  TK_PROF_ADD(w, 2);
  // --- half-pel then quarter-pel (encode_block.c:628-663)
#if TK_PROF_MACROS
  pt0_ = (long long)__builtin_readcyclecounter();
#endif
  unsigned cmin = min_sad;
#ifdef TK_ME_NO_SUBPEL   // tools/ubench_me.cpp: the full-pel part alone
  if (false) {
#else
  {
#endif
  if (a.speed == 0)
  for (int pass = 0; pass < 2; pass++) {
    const int d = pass == 0 ? 2 : 1;
    const mv_t base = pass == 0 ? mv_ref : mv_opt;
#ifdef TK_ME_CROSSCHECK
    unsigned xs_sub = ~0u;   // result of me_cand8_subpel for this pass (test builds compare it with the generic pass)
#endif
    // order: (0,-d) (-d,0) (d,0) (0,d) (-d,-d) (-d,d) (d,-d) (d,d) as (y,x)
    struct SPc { mv_t mv; SubPel sp; };
    auto sub_prep = [&](int c) -> SPc {
      int oy = c == 0 ? 0 : c == 1 ? -d : c == 2 ? d : c == 3 ? 0 : c == 4 ? -d : c == 5 ? -d : d;
      int ox = c == 0 ? -d : c == 1 ? 0 : c == 2 ? 0 : c == 3 ? d : c == 4 ? -d : c == 5 ? d : c == 6 ? -d : d;
      SPc x;
      x.mv = mk_mv(base.x + ox, base.y + oy);
      x.sp = luma_setup(x.mv, a.sign, a.width, a.height, a.fwidth, a.fheight, a.xpos, a.ypos, a.enable_bipred);
      return x;
    };
    const Pow2 dw = mk_pow2(a.width);
    auto sub_item = [&](const SPc& x, int r) -> int {
      int i, j;
      split2(dw, r, i, j);
      return iabs((int)orgs[i * a.ostride + j] - luma_sample(ref, a.rstride, i, j, x.sp, a.enable_bipred, a.bitdepth));
    };
    auto sub_cost = [&](int, const SPc& x, int sad) -> unsigned {
      return ((unsigned)sad >> sh) + mv_cost(a.lam, x.mv.y - mvp.y, x.mv.x - mvp.x);
    };
    // PUs of up to 16x16 samples whose interpolation windows lie in the staged window: eight lanes per candidate (me_cand8_subpel; 16-bit samples since
    // round 6: me_cand16_subpel)
    {
#ifndef TK_ME_NO_SMALL
      if (TKU(a.width * a.height <= 256 && t.size == 64)) {   // (32x32: the 64-lane strip form below is faster - tools/ubench_me.cpp)
        unsigned k32;
        if constexpr (sizeof(PIX) == 1)
          k32 = me_cand8_subpel<SP>(t, org, a.ostride, a.width, a.height, a.sign, a.fwidth, a.fheight, a.xpos, a.ypos, a.enable_bipred, a.lam, win.w32, win.ox, win.oy,
                                    win.Ww, win.Wh, win.pitch, win.on, base, d, mvp);
        else
          k32 = me_cand16_subpel<SP>(t, org, a.ostride, a.width, a.height, a.sign, a.fwidth, a.fheight, a.xpos, a.ypos, a.enable_bipred, a.lam, win.w32, win.ox, win.oy,
                                     win.Ww, win.Wh, win.pitch, win.on, base, d, mvp, a.bitdepth);
        if (k32 != 0xffffffffu) {
#ifdef TK_ME_CROSSCHECK
          xs_sub = k32;
#else
          mv_t bestv = base;
          if ((k32 >> 8) < cmin) {
            cmin = k32 >> 8;
            const int c = (int)(k32 & 0xffu);
            const int oy = c == 0 ? 0 : c == 1 ? -d : c == 2 ? d : c == 3 ? 0 : c == 4 ? -d : c == 5 ? -d : d;
            const int ox = c == 0 ? -d : c == 1 ? 0 : c == 2 ? 0 : c == 3 ? d : c == 4 ? -d : c == 5 ? d : c == 6 ? -d : d;
            bestv = mk_mv(base.x + ox, base.y + oy);
          }
          mv_opt = mk_mv(mv_opt.x + (bestv.x - base.x), mv_opt.y + (bestv.y - base.y));
          continue;
#endif
        }
      }
#endif
    }
    // Fast path: all eight candidates read from the 8x8 window around the centre's integer position (always,
    // except when luma_setup's frame-edge clamps pull a candidate further away).
    TK_PROF_MARK(ps0_);
    SPc cand[8];
    const SubPel ctr = luma_setup(base, a.sign, a.width, a.height, a.fwidth, a.fheight, a.xpos, a.ypos, a.enable_bipred);
    int in_window = 1;
    for (int c = 0; c < 8; c++) {
      cand[c] = sub_prep(c);
      const int dy = cand[c].sp.ver_int - ctr.ver_int + 1, dx = cand[c].sp.hor_int - ctr.hor_int + 1;
      if (dy < 0 || dy > 2 || dx < 0 || dx > 2) in_window = 0;
    }
    unsigned long long k;
    (void)0;
    TK_PROF_MARK(ps1_);
#if TK_PROF_SUBPEL   // tools/ubench_me.cpp: set-up / sample loop / reduction of a sub-pel pass
    if (t.rank == 0) w->prof[6] += ps1_ - ps0_;
#endif
    if (in_window) {
      int sad8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      // per-candidate parameters are identical in every lane: scalar registers
      SubK8 k8[8];
      for (int c = 0; c < 8; c++) {
        SubPel usp = cand[c].sp;   // (subk8_make reads the packed taps and the fractions only)
        usp.ph = tk_uniform64(usp.ph); usp.pv = tk_uniform64(usp.pv);
        usp.ver_frac = tk_uniform(usp.ver_frac); usp.hor_frac = tk_uniform(usp.hor_frac);
        k8[c] = subk8_make(usp, tk_uniform(cand[c].sp.ver_int - ctr.ver_int + 1), tk_uniform(cand[c].sp.hor_int - ctr.hor_int + 1), a.enable_bipred);
      }
      const int sub_in_win = TKU(win.on && ctr.hor_int - 3 >= win.ox && ctr.hor_int + a.width + 5 <= win.ox + win.Ww &&
                                 ctr.ver_int - 3 >= win.oy && ctr.ver_int + a.height + 5 <= win.oy + win.Wh);
      if (sizeof(PIX) == 1 && a.width * a.height >= 512) {
        // large PUs: a lane takes a vertical strip of eight samples of one column (tk_pred.h:subk8_strip)
        if constexpr (sizeof(PIX) == 1) {
          for (int r = t.rank; r < a.width * (a.height >> 3); r += t.size) {
            int st, j;
            split2(dw, r, st, j);
            const int i0 = st << 3;
            const PIX* p0 = ref + (i0 + ctr.ver_int - 3) * a.rstride + (j + ctr.hor_int - 3);
            unsigned long long wb[15];
            if (sub_in_win) {   // the rows come out of the staged window
              const int woff = (i0 + ctr.ver_int - 3 - win.oy) * win.pitch + (j + ctr.hor_int - 3 - win.ox);
              TK_UNROLL
              for (int q = 0; q < 15; q++) { const Seg16 sg = win_seg<8>(win.w32, woff + q * win.pitch); wb[q] = (((unsigned long long)sg.d[1] << 32) | sg.d[0]) ^ 0x8080808080808080ull; }
            } else {
              TK_UNROLL
              for (int q = 0; q < 15; q++) wb[q] = gload64(p0 + q * a.rstride) ^ 0x8080808080808080ull;
            }
            int o8[8];
            TK_UNROLL
            for (int q = 0; q < 8; q++) o8[q] = (int)orgs[(i0 + q) * a.ostride + j];
            TK_UNROLL
            for (int c = 0; c < 8; c++) sad8[c] = subk8_strip(wb, k8[c], o8, sad8[c]);
          }
        }
      } else if (sizeof(PIX) == 2) {
        // 16-bit samples: eight window rows of eight samples per prediction sample (window or plane), candidates by v_dot2 (tk_pred.h:SubK16)
        if constexpr (sizeof(PIX) == 2) {
          SubK16 k16[8];
          for (int c = 0; c < 8; c++) {
            SubPel usp = cand[c].sp;
            for (int m = 0; m < 6; m++) { usp.tv[m] = tk_uniform(usp.tv[m]); usp.th[m] = tk_uniform(usp.th[m]); }
            usp.ver_frac = tk_uniform(usp.ver_frac); usp.hor_frac = tk_uniform(usp.hor_frac);
            k16[c] = subk16_make(usp, tk_uniform(cand[c].sp.ver_int - ctr.ver_int + 1), tk_uniform(cand[c].sp.hor_int - ctr.hor_int + 1), a.enable_bipred);
          }
          if (a.width * a.height >= 512) {
            // large PUs: a lane takes a vertical strip of eight samples of one column (tk_pred.h:subk16_strip)
            for (int r = t.rank; r < a.width * (a.height >> 3); r += t.size) {
              int st, j;
              split2(dw, r, st, j);
              const int i0 = st << 3;
              uint32_t wb[15][4];
              if (sub_in_win) {
                const int woff = (i0 + ctr.ver_int - 3 - win.oy) * win.pitch + (j + ctr.hor_int - 3 - win.ox) * 2;
                TK_UNROLL
                for (int q = 0; q < 15; q++) { const Seg16 sg = win_seg<16>(win.w32, woff + q * win.pitch); wb[q][0] = sg.d[0]; wb[q][1] = sg.d[1]; wb[q][2] = sg.d[2]; wb[q][3] = sg.d[3]; }
              } else {
                const PIX* p0 = ref + (i0 + ctr.ver_int - 3) * a.rstride + (j + ctr.hor_int - 3);
                TK_UNROLL
                for (int q = 0; q < 15; q++) { const Seg16 sg = seg_load<SP_GLOBAL, 16>(p0 + q * a.rstride); wb[q][0] = sg.d[0]; wb[q][1] = sg.d[1]; wb[q][2] = sg.d[2]; wb[q][3] = sg.d[3]; }
              }
              int o8[8];
              TK_UNROLL
              for (int q = 0; q < 8; q++) o8[q] = (int)orgs[(i0 + q) * a.ostride + j];
              TK_UNROLL
              for (int c = 0; c < 8; c++) sad8[c] = subk16_strip(wb, k16[c], o8, sad8[c], a.bitdepth);
            }
          } else
          for (int r = t.rank; r < a.width * a.height; r += t.size) {
            int i, j;
            split2(dw, r, i, j);
            uint32_t rows[8][4];
            if (sub_in_win) {
              const int woff = (i + ctr.ver_int - 3 - win.oy) * win.pitch + (j + ctr.hor_int - 3 - win.ox) * 2;
              TK_UNROLL
              for (int q = 0; q < 8; q++) { const Seg16 sg = win_seg<16>(win.w32, woff + q * win.pitch); rows[q][0] = sg.d[0]; rows[q][1] = sg.d[1]; rows[q][2] = sg.d[2]; rows[q][3] = sg.d[3]; }
            } else {
              const PIX* p0 = ref + (i + ctr.ver_int - 3) * a.rstride + (j + ctr.hor_int - 3);
              TK_UNROLL
              for (int q = 0; q < 8; q++) { const Seg16 sg = seg_load<SP_GLOBAL, 16>(p0 + q * a.rstride); rows[q][0] = sg.d[0]; rows[q][1] = sg.d[1]; rows[q][2] = sg.d[2]; rows[q][3] = sg.d[3]; }
            }
            const int o = (int)orgs[i * a.ostride + j];
            TK_UNROLL
            for (int c = 0; c < 8; c++) sad8[c] += iabs(o - subk16_sample(rows, k16[c], a.bitdepth));
          }
        }
      } else
      for (int r = t.rank; r < a.width * a.height; r += t.size) {
        int i, j;
        split2(dw, r, i, j);
        const PIX* p0 = ref + (i + ctr.ver_int - 3) * a.rstride + (j + ctr.hor_int - 3);
        WinRow<PIX> wr[8];
        if (sub_in_win) {   // the (PU + 8)^2 samples around the centre are inside the staged window
          if constexpr (sizeof(PIX) == 1) {
            const int woff = (i + ctr.ver_int - 3 - win.oy) * win.pitch + (j + ctr.hor_int - 3 - win.ox);
            TK_UNROLL
            for (int q = 0; q < 8; q++) { const Seg16 sg = win_seg<8>(win.w32, woff + q * win.pitch); wr[q].a = ((unsigned long long)sg.d[1] << 32) | sg.d[0]; }
          }
        } else
          for (int q = 0; q < 8; q++) win_load(p0 + q * a.rstride, wr[q]);
        const int o = (int)orgs[i * a.ostride + j];
        if constexpr (sizeof(PIX) == 1) {
          unsigned long long wb[8];
          for (int q = 0; q < 8; q++) wb[q] = wr[q].a ^ 0x8080808080808080ull;   // samples - 128 as int8 lanes
          TK_UNROLL
          for (int c = 0; c < 8; c++) {
            const unsigned pr = (unsigned)subk8_sample(wb, k8[c]), uo = (unsigned)o;
            sad8[c] += (int)((uo > pr ? uo : pr) - (uo < pr ? uo : pr));
          }
        } else {
          for (int c = 0; c < 8; c++) {
            const int dy = cand[c].sp.ver_int - ctr.ver_int + 1, dx = cand[c].sp.hor_int - ctr.hor_int + 1;
            WinRow<PIX> rows[6];
            for (int m = 0; m < 6; m++) rows[m] = win_pick(wr[m], wr[m + 1], wr[m + 2], dy, dx);
            sad8[c] += iabs(o - luma_sample_win<PIX>(rows, cand[c].sp, a.enable_bipred, a.bitdepth));
          }
        }
      }
      TK_PROF_ACC(w, 10, ps1_);
      TK_PROF_MARK(ps2_);
      k = ~0ull;
      for (int c = 0; c < 8; c++) {
        const int tot = team_sum(t, sad8[c]);
        const unsigned long long kk = ((unsigned long long)sub_cost(c, cand[c], tot) << 32) | (unsigned)c;
        k = kk < k ? kk : k;
      }
#if TK_PROF_SUBPEL
      TK_PROF_ACC(w, 7, ps2_);
#endif
    } else
      k = eval_min(t, 8, a.width * a.height, sub_prep, sub_item, sub_cost);
#ifdef TK_ME_CROSSCHECK
    if (xs_sub != ~0u && ((xs_sub >> 8) != (unsigned)(k >> 32) || (xs_sub & 0xffu) != ((unsigned)k & 0xffu))) {
#if TK_HOST
      abort();
#else
      __builtin_trap();
#endif
    }
#endif
    mv_t best = base;
    if ((unsigned)(k >> 32) < cmin) { cmin = (unsigned)(k >> 32); best = sub_prep((int)(unsigned)k).mv; }
    // mv_opt += delta of the winning position (none => unchanged)
    mv_opt = mk_mv(mv_opt.x + (best.x - base.x), mv_opt.y + (best.y - base.y));
  }
  else {
    // bilinear approximation (encode_block.c:664-707).  NB the reference folds the sign into mv_ref before
    // pricing the half-pel vector, so for a backward reference the rate term sees the negated vector.
    mv_t mr = mk_mv(mv_ref.x * s, mv_ref.y * s);
    int spx = 0, spy = 0, xd_hp = 0, yd_hp = 0, xd_qp = 0, yd_qp = 0;
    unsigned sad = fast_halfpel<SP>(t, org, ref + (mr.y >> 2) * a.rstride + (mr.x >> 2), a.ostride, a.rstride, a.width, a.height, &spx, &spy) >> sh;
    sad += mv_cost(a.lam, mr.y + s * spy - mvp.y, mr.x + s * spx - mvp.x);
    if (sad < cmin) { cmin = sad; xd_hp = s * spx; yd_hp = s * spy; }
    spx = xd_hp; spy = yd_hp;
    mr = mk_mv(mv_opt.x + s * spx, mv_opt.y + s * spy);
    mv_opt = mk_mv(mv_opt.x + xd_hp, mv_opt.y + yd_hp);
    sad = fast_quarterpel<SP>(t, org, ref + (s * (mr.y >> 2)) * a.rstride + s * (mr.x >> 2), a.ostride, a.rstride, a.width, a.height, &spx, &spy) >> sh;
    sad += mv_cost(a.lam, mr.y + s * spy - mvp.y, mr.x + s * spx - mvp.x);
    if (sad < cmin) { cmin = sad; xd_qp = s * spx; yd_qp = s * spy; }
    mv_opt = mk_mv(mv_opt.x + xd_qp, mv_opt.y + yd_qp);
  }
  }
  TK_PROF_ADD(w, 3);
#if TK_PROF_ME
  // whole-call cycles and call counts by coding-block size (this build's code_tu does not use slots 16..25)
  if (t.rank == 0) {
    const int cls = a.cb_size <= 8 ? 0 : a.cb_size == 16 ? 1 : a.cb_size == 32 ? 2 : a.cb_size == 64 ? 3 : 4;
    w->prof[16 + cls] += (long long)__builtin_readcyclecounter() - pme0_;
    w->prof[21 + cls] += 1;
  }
#endif
  *mv_out = mv_opt;
  return cmin < min_sad ? cmin : min_sad;
}


// motion_estimate_bi (enc/encode_block.c:798-914): joint search of ONE vector used as +mv on ref0 and
// -mv on ref1 (B frames, encoder_speed 0).  3x3 telescope from 8 px down to 1/4 px around the rounded
// centre, then six "extra" candidates read from the per-SB candidate list of r_idx0 - including the
// reference's side effect on that list (slots [num..3] zero-filled, slots 4 and 5 overwritten with mvp
// and (0,0) without touching the count) and its use of the list's full-pel entries
// as quarter-pel vectors.  The vector is clipped for ref0's sign and then AGAIN for ref1's sign; ref0 is
// predicted with the once-clipped vector, ref1 and the cost use the twice-clipped one.
// The search has two phases: the telescope (phase bit 1), which depends only on the block, the two reference planes, mvc and mvp,
// and the six extra candidates (phase bit 2), which read - and clobber - the candidate list as it stands after the bi-prediction
// search of the block.  The block decision of a B frame runs the telescope early on another wavefront (tk_block_queue.h:md_bijoint_telescope) and
// hands its result (min_sad_in, *mv_out) to the second phase; phase 3 = both, back to back.
template <typename PIX, int SP>
TK_DEVNI unsigned motion_estimate_bi(const Team t, MeWs* w_, const PIX* org_, const PIX* ref0, const PIX* ref1, const MeArgs& a,
                                    mv_t mvc, mv_t mvp, int r_idx0, mv_t* mv_out, int phase = 3, unsigned min_sad_in = kCostInit) {
  const auto org = spc<SP>(org_);
  const auto lists = ldsc(lds_ld(&w_->lists));
  const int sh = a.bitdepth - 8;
  const int size = a.cb_size;
  unsigned min_sad = (phase & 1) ? (unsigned)kCostInit : min_sad_in;
  mv_t mv_opt = (phase & 1) ? mk_mv(0, 0) : *mv_out;
  mv_t mv_ref = mk_mv(((mvc.x + 2) >> 2) << 2, ((mvc.y + 2) >> 2) << 2);
  struct BI { mv_t mv; SubPel s0, s1; };
  auto mk_bi = [&](mv_t mv) -> BI {
    BI x;
    mv_t m0 = clip_mv(mv, a.ypos, a.xpos, a.fwidth, a.fheight, size, size, a.sign);
    mv_t m1 = clip_mv(m0, a.ypos, a.xpos, a.fwidth, a.fheight, size, size, 1 - a.sign);
    x.mv = m1;
    x.s0 = luma_setup(m0, a.sign, size, size, a.fwidth, a.fheight, a.xpos, a.ypos, a.enable_bipred);
    x.s1 = luma_setup(m1, 1 - a.sign, size, size, a.fwidth, a.fheight, a.xpos, a.ypos, a.enable_bipred);
    return x;
  };
  const Pow2 dw = mk_pow2(size);
  auto bi_item = [&](const BI& x, int r) -> int {
    int i, j;
    split2(dw, r, i, j);
    int p0 = luma_sample(ref0, a.rstride, i, j, x.s0, a.enable_bipred, a.bitdepth);
    int p1 = luma_sample(ref1, a.rstride, i, j, x.s1, a.enable_bipred, a.bitdepth);
    return iabs((int)org[i * a.ostride + j] - ((p0 + p1) >> 1));
  };
  auto bi_cost = [&](int, const BI& x, int sad) -> unsigned {
    return ((unsigned)sad >> sh) + mv_cost(a.lam, (int16_t)(x.mv.y - mvp.y), (int16_t)(x.mv.x - mvp.x));
  };
  for (int step = (phase & 1) ? 32 : 0; step > 0; step >>= 1) {
    // candidate list of this step in the reference's (k outer = y, l inner = x) order
    int ox[9], oy[9], n = 0;
    const int vf = mv_ref.y & 3, hf = mv_ref.x & 3;
    for (int k = -step; k <= step; k += step)
      for (int l = -step; l <= step; l += step) {
        if (step < 32 && k == 0 && l == 0) continue;
        if (step == 1) {
          int skip;
          if (vf == 0 && hf == 0) skip = iabs(k) != iabs(l);
          else if (vf == 2 && hf == 2) skip = 1;
          else skip = iabs(k) == iabs(l);
          if (skip) continue;
        }
        ox[n] = l; oy[n] = k; n++;
      }
    if (n > 0) {
      const mv_t centre = mv_ref;
      auto cand = [&](int c) -> BI {
        int x = 0, y = 0;
        for (int q = 0; q < 9; q++) if (q == c) { x = ox[q]; y = oy[q]; }
        return mk_bi(mk_mv(centre.x + x, centre.y + y));
      };
      // A step whose candidates all sit on integer positions in both references (every step of 4 quarter-pels and more, unless a
      // frame-edge clamp of luma_setup interferes) predicts by copying: the SAD against the truncating average of the two displaced
      // blocks runs on the row-segment evaluator of the uni-directional search (16 bytes of each reference per lane and memory
      // instruction) instead of one sample per lane and step.
      // (the steps of 2 and 1 quarter-pels move off the integer grid: no need to build their candidates twice to find that out)
      int all_int = step >= 4;
      for (int c = 0; c < n && all_int; c++) { const BI x = cand(c); all_int = all_int && !(x.s0.ver_frac | x.s0.hor_frac | x.s1.ver_frac | x.s1.hor_frac); }
      unsigned long long k;
      if (TKU(all_int)) {
        struct FB { mv_t mv; const PIX* p; const PIX* p2; int dx, dy; };
        auto cand_fp = [&](int c) -> FB {
          const BI x = cand(c);
          FB f;
          f.mv = x.mv; f.dx = f.dy = 0;
          f.p = ref0 + x.s0.ver_int * a.rstride + x.s0.hor_int;
          f.p2 = ref1 + x.s1.ver_int * a.rstride + x.s1.hor_int;
          return f;
        };
        MeWin nowin;
        nowin.on = 0; nowin.w32 = nullptr; nowin.ox = nowin.oy = nowin.Ww = nowin.Wh = nowin.pitch = 0;
        k = eval_fullpel<SP>(t, n, org_, a.ostride, a.rstride, size, size, nowin, cand_fp,
                             [&](const FB& x, int sad) -> unsigned { return ((unsigned)sad >> sh) + mv_cost(a.lam, (int16_t)(x.mv.y - mvp.y), (int16_t)(x.mv.x - mvp.x)); });
      } else
        k = eval_min(t, n, size * size, cand, bi_item, bi_cost);
      if ((unsigned)(k >> 32) < min_sad) { min_sad = (unsigned)(k >> 32); mv_opt = cand((int)(unsigned)k).mv; }
    }
    mv_ref = mv_opt;
  }
  if (!(phase & 2)) { *mv_out = mv_opt; return min_sad; }
  // extra candidates (+ side effect on the shared list)
  t.sync();
  if (t.rank == 0) {
    for (int idx = lists->mvcand_num[r_idx0]; idx < 4; idx++) { lists->mvcand[r_idx0][idx].x = 0; lists->mvcand[r_idx0][idx].y = 0; }
    lists->mvcand[r_idx0][4].x = mvp.x; lists->mvcand[r_idx0][4].y = mvp.y;
    lists->mvcand[r_idx0][5].x = 0; lists->mvcand[r_idx0][5].y = 0;
  }
  t.sync();
  {
    auto cand = [&](int c) -> BI { return mk_bi(mk_mv(lists->mvcand[r_idx0][c].x, lists->mvcand[r_idx0][c].y)); };
    unsigned long long k = eval_min(t, 6, size * size, cand, bi_item, bi_cost);
    if ((unsigned)(k >> 32) < min_sad) { min_sad = (unsigned)(k >> 32); mv_opt = cand((int)(unsigned)k).mv; }
  }
  t.sync();
  *mv_out = mv_opt;
  return min_sad;
}

}  // namespace tk
