// tk_me_fastsub.h - bilinear sub-pel approximations of encoder_speed > 0: fast_halfpel, fast_quarterpel.
#pragma once
#include "tk_me_seg.h"

namespace tk {
// Bilinear sub-pel approximations of encoder_speed > 0 (sad_calc_fasthalf enc/encode_block.c:174-283 ==
// sad_calc_fasthalf_simd enc_kernels.c:330, sad_calc_fastquarter :286-415): the SADs of the 8 half-
// (quarter-) pel neighbours of the centre built from rounding (avg) and truncating (rdavg) byte averages;
// returns the smallest of them and its offset.  Lanes split the samples, 8 shuffle reductions.
template <int SP, typename PIX> TK_DEV unsigned fast_halfpel(const Team t, const PIX* a_, const PIX* b, int as, int bs, int width, int height, int* bx, int* by) {
  const auto a = spc<SP>(a_);
  int tl = 0, tr = 0, br = 0, bl = 0, top = 0, right = 0, down = 0, left = 0;
  const Pow2 dw = mk_pow2(width);
  for (int r = t.rank; r < width * height; r += t.size) {
    int i, j;
    split2(dw, r, i, j);
    const PIX* c = b + i * bs + j;
    auto B = [&](int dy, int dx) -> int { return (int)c[dy * bs + dx]; };
    auto av = [](int x, int y) { return (x + y + 1) >> 1; };
    auto rd = [](int x, int y) { return (x + y) >> 1; };
    const int o = (int)a[i * as + j];
    const int h_l = av(B(0, -1), B(0, 0)), h_r = av(B(0, 0), B(0, 1));
    const int v4 = av(B(-2, 0), B(1, 0));          // column j,   rows -2 / +1
    const int v4b = av(B(-1, 0), B(2, 0));         // column j,   rows -1 / +2
    const int t6 = av(B(0, -2), B(0, 1));          // row 0, cols -2 / +1
    const int t7 = av(B(0, -1), B(0, 2));          // row 0, cols -1 / +2
    const int ptl = rd(rd(rd(av(B(-2, -1), B(1, -1)), v4), rd(av(B(-1, -2), B(-1, 1)), t6)), rd(av(B(-1, -1), B(-1, 0)), h_l));
    const int ptr = rd(rd(rd(v4, av(B(-2, 1), B(1, 1))), rd(t7, av(B(-1, -1), B(-1, 2)))), rd(av(B(-1, 0), B(-1, 1)), h_r));
    const int pbl = rd(rd(rd(v4b, av(B(-1, -1), B(2, -1))), rd(t6, av(B(1, -2), B(1, 1)))), rd(av(B(1, -1), B(1, 0)), h_l));
    const int pbr = rd(rd(rd(v4b, av(B(-1, 1), B(2, 1))), rd(t7, av(B(1, -1), B(1, 2)))), rd(h_r, av(B(1, 0), B(1, 1))));
    left += iabs(o - h_l); right += iabs(o - h_r);
    down += iabs(o - av(B(0, 0), B(1, 0))); top += iabs(o - av(B(0, 0), B(-1, 0)));
    tl += iabs(o - ptl); tr += iabs(o - ptr); br += iabs(o - pbr); bl += iabs(o - pbl);
  }
  unsigned utop = (unsigned)team_sum(t, top), uright = (unsigned)team_sum(t, right), udown = (unsigned)team_sum(t, down), uleft = (unsigned)team_sum(t, left);
  unsigned utl = (unsigned)team_sum(t, tl), utr = (unsigned)team_sum(t, tr), ubr = (unsigned)team_sum(t, br), ubl = (unsigned)team_sum(t, bl);
  int x = 0, y = -2;
  if (udown < utop) { y = 2; utop = udown; }
  if (uright < utop) { x = 2; y = 0; utop = uright; }
  if (uleft < utop) { x = -2; y = 0; utop = uleft; }
  if (utl < utop) { x = -2; y = -2; utop = utl; }
  if (utr < utop) { x = 2; y = -2; utop = utr; }
  if (ubr < utop) { x = 2; y = 2; utop = ubr; }
  if (ubl < utop) { x = -2; y = 2; utop = ubl; }
  *bx = x; *by = y;
  return utop;
}

template <int SP, typename PIX> TK_DEV unsigned fast_quarterpel(const Team t, const PIX* o__, const PIX* r_, int os, int rs, int width, int height, int* bx, int* by) {
  const auto o_ = spc<SP>(o__);
  int tl = 0, tr = 0, br = 0, bl = 0, top = 0, right = 0, down = 0, left = 0;
  const int hx = *bx, hy = *by;  // half-pel offset chosen before (0 or +-2): selects the interpolation pattern
  const Pow2 dw = mk_pow2(width);
  for (int q = t.rank; q < width * height; q += t.size) {
    int i, j;
    split2(dw, q, i, j);
    const PIX* c = r_ + i * rs + j;
    auto av = [](int x, int y) { return (x + y + 1) >> 1; };
    const int o = (int)o_[i * os + j];
    const int a = c[0], d = c[1], f = c[rs];
    int p_tl, p_top, p_tr, p_left, p_right, p_bl, p_down, p_br;
    if (hx & hy) {
      const int e = c[rs + 1];
      const int ad = av(a, d), de = av(d, e), af = av(a, f), fe = av(f, e);
      p_tl = (ad + af) >> 1; p_top = (de + a) >> 1; p_tr = (ad + de) >> 1; p_left = (ad + f) >> 1; p_right = (ad + e) >> 1;
      p_bl = (af + fe) >> 1; p_down = (de + f) >> 1; p_br = (de + fe) >> 1;
    } else if (hx) {
      const int b = c[-rs], cc = c[-rs + 1], e = c[rs + 1];
      const int ad = av(a, d), de = av(d, e), dc = av(d, cc), af = av(a, f), ab = av(a, b);
      p_tl = (ad + ab) >> 1; p_top = (dc + a) >> 1; p_tr = (ad + dc) >> 1; p_left = (ad + a) >> 1; p_right = (ad + d) >> 1;
      p_bl = (ad + af) >> 1; p_down = (af + d) >> 1; p_br = (ad + de) >> 1;
    } else if (hy) {
      const int e = c[rs + 1], g = c[rs - 1], h = c[-1];
      const int ad = av(a, d), af = av(a, f), fe = av(f, e), ah = av(a, h), gf = av(g, f);
      p_tl = (ah + af) >> 1; p_top = (af + a) >> 1; p_tr = (ad + af) >> 1; p_left = (gf + a) >> 1; p_right = (ad + f) >> 1;
      p_bl = (af + gf) >> 1; p_down = (af + f) >> 1; p_br = (af + fe) >> 1;
    } else {
      const int b = c[-rs], h = c[-1];
      const int ad = av(a, d), af = av(a, f), ah = av(a, h), ab = av(a, b);
      p_tl = (ah + ab) >> 1; p_top = (ab + a) >> 1; p_tr = (ad + ab) >> 1; p_left = (ah + a) >> 1; p_right = (ad + a) >> 1;
      p_bl = (ah + af) >> 1; p_down = (af + a) >> 1; p_br = (af + ad) >> 1;
    }
    tl += iabs(o - p_tl); top += iabs(o - p_top); tr += iabs(o - p_tr); left += iabs(o - p_left); right += iabs(o - p_right);
    bl += iabs(o - p_bl); down += iabs(o - p_down); br += iabs(o - p_br);
  }
  unsigned utop = (unsigned)team_sum(t, top), uright = (unsigned)team_sum(t, right), udown = (unsigned)team_sum(t, down), uleft = (unsigned)team_sum(t, left);
  unsigned utl = (unsigned)team_sum(t, tl), utr = (unsigned)team_sum(t, tr), ubr = (unsigned)team_sum(t, br), ubl = (unsigned)team_sum(t, bl);
  int x = 0, y = -1;
  if (utl < utop) { x = -1; utop = utl; }
  if (utr < utop) { x = 1; utop = utr; }
  if (uleft < utop) { x = -1; y = 0; utop = uleft; }
  if (uright < utop) { x = 1; y = 0; utop = uright; }
  if (ubl < utop) { x = -1; y = 1; utop = ubl; }
  if (udown < utop) { x = 0; y = 1; utop = udown; }
  if (ubr < utop) { x = 1; y = 1; utop = ubr; }
  *bx = x; *by = y;
  return utop;
}
}  // namespace tk
