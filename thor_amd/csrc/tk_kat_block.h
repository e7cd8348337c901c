// tk_kat_block.h - one known-answer item of the block decision's neighbour context (tk_block_ctx.h) and the parameter rows / host-side argument checks of
// thor_hip_kat_block_ctx, thor_hip_kat_block_cost, thor_hip_kat_intra_search and thor_hip_kat_build_org8, shared by the device kernels (hip_kat_block.h) and the host build (tests/hostsim/kat_host_ctx.cpp).
// The expected answers are the reference's own (tests/golden/gen_kat11.py -> kat11.npz).
#pragma once
#include "tk_block_search.h"

namespace tk {
// par[kKatCtxPar * i ..]: ypos, xpos, size, frame width, frame height, superblock size
// out[kKatCtxOut * i ..]: get_mv_pred x, y | get_mv_cands count | candidate 0 and 1: mv0.x, mv0.y, mv1.x, mv1.y, ref0, ref1, dir (zeros for a candidate not
// returned) | find_contexts ctx_cbp, ctx_index with enable = 0, then with enable = 1 | upright_avail, downleft_avail
enum { kKatCtxPar = 6, kKatCtxOut = 23 };
TK_DEV void kat_ctx_item(const DbCell* cells, int cs, const int* q, int* o) {
  const int ypos = q[0], xpos = q[1], size = q[2], fw = q[3], fh = q[4], sb = q[5];
  const mv_t p = get_mv_pred(cells, cs, ypos, xpos, fw, fh, size, sb);
  InterPred c[2];
  c[0] = zero_pred(); c[1] = zero_pred();
  const int n = get_mv_cands(cells, cs, ypos, xpos, fw, fh, size, sb, c);
  o[0] = p.x; o[1] = p.y; o[2] = n;
  for (int k = 0; k < 2; k++) {
    const InterPred z = k < n ? c[k] : zero_pred();
    int* r = o + 3 + 7 * k;
    r[0] = z.mv0.x; r[1] = z.mv0.y; r[2] = z.mv1.x; r[3] = z.mv1.y; r[4] = z.ref0; r[5] = z.ref1; r[6] = z.dir;
  }
  for (int enable = 0; enable < 2; enable++) {
    SynCtx s;
    find_contexts(cells, cs, ypos, xpos, fh, fw, size, enable, &s);
    o[17 + 2 * enable] = s.ctx_cbp; o[18 + 2 * enable] = s.ctx_index;
  }
  o[21] = upright_avail(ypos, xpos, size, size, fw, sb);
  o[22] = downleft_avail(ypos, xpos, size, size, fh, sb);
}
// Host-side check of one item: 0 when every cell index the functions above can form - bi - cs - 1 (up-left) .. bi + cs * size / 4 - 1 (down-left) - lies inside a
// grid of `ncells` cells that is preceded by one row and one column (cs + 1 cells) of padding.
// (The up-right index bi - cs + size / 4 lies between the two: above bi - cs - 1, and - a row holds cs >= 2 cells - below bi + cs * size / 4; at the last
// column it is the first cell of the block's own row, inside the grid like every index that merely wraps into the next row.)
static inline int kat_ctx_check(const int* q, long long ncells) {
  const int ypos = q[0], xpos = q[1], size = q[2], fw = q[3], fh = q[4], sb = q[5];
  if ((sb != 64 && sb != 128) || size < 8 || size > sb || (size & (size - 1)) || fw < 8 || fh < 8 || fw > 8192 || fh > 8192 || fw % 8 || fh % 8) return 1;
  if (ypos < 0 || xpos < 0 || ypos >= fh || xpos >= fw || ypos % size || xpos % size) return 1;
  const long long cs = fw / 4, bi = (long long)(ypos / 4) * cs + xpos / 4;
  return bi + cs * (size / 4) <= ncells ? 0 : 2;
}

// thor_hip_kat_block_cost.  par[kKatCostPar * i ..]: size, bw, bh, nbits, off (first sample of the item's compact block in the org / rec pools: Y size x size,
// U, V (size / 2)^2, stride = size; a multiple of 16), skew (bytes from a 16-byte boundary to the original's first luma sample; chroma: half of it, rounded
// down to a whole sample), stride (of the original's luma rows, in samples; chroma: half).
// out[kKatCostOut * i ..] (64 bit): luma SSD from the SP_GLOBAL instance | from the SP_LDS instance (all ones where the block is wider than kLdsBlk) | rd_cost |
// rd_cost with the luma SSD passed in
enum { kKatCostPar = 7, kKatCostOut = 4 };
static inline int kat_cost_check(const int* q, double lambda, long long nsamp, int sample_bytes) {
  const int size = q[0], bw = q[1], bh = q[2], nbits = q[3], off = q[4], skew = q[5], stride = q[6];
  if (size < 8 || size > kMaxSb || (size & (size - 1)) || bw < 8 || bh < 8 || bw > size || bh > size || bw % 8 || bh % 8) return 1;
  if (nbits < 0 || nbits > (1 << 20) || !(lambda >= 0.0 && lambda <= 1e6)) return 1;
  if (skew < 0 || skew >= 16 || skew % sample_bytes || stride < bw || stride > 4096 || stride % 2) return 1;
  if (off < 0 || off % 16 || (long long)off + size * size * 3 / 2 > nsamp) return 2;
  return 0;
}

// thor_hip_kat_intra_search.  par[kKatIntraPar * i ..]: ypos, xpos, size, superblock size, num_intra_modes, off (first sample of the item's compact original
// block in the pool, stride = size; a multiple of 16).  The reconstructed plane is fw x fh samples with stride fw.  out[2 * i ..]: intra mode, SAD.
// The search reads the plane at row ypos - 1, columns xpos - 1 .. xpos + size (the last one only where up-right is available: xpos + size < fw), and at column
// xpos - 1, rows ypos .. ypos + size (the last one only where down-left is available: ypos + size < fh): inside the plane for every block inside the frame.
enum { kKatIntraPar = 6, kKatIntraOut = 2 };
static inline int kat_intra_check(const int* q, int fw, int fh, long long nsamp) {
  const int ypos = q[0], xpos = q[1], size = q[2], sb = q[3], nm = q[4], off = q[5];
  if ((sb != 64 && sb != 128) || size < 8 || size > 64 || (size & (size - 1)) || (nm != 4 && nm != 10)) return 1;
  if (ypos < 0 || xpos < 0 || ypos % size || xpos % size || ypos + size > fh || xpos + size > fw) return 2;
  if (off < 0 || off % 16 || (long long)off + size * size > nsamp) return 2;
  return 0;
}
// thor_hip_kat_build_org8.  par[kKatOrg8Par * i ..]: size, off (first sample of the item's compact blocks - original, prediction - in the two pools, and of
// its two output blocks; a multiple of 16), skew (bytes from a 16-byte boundary to the original's first sample, a whole number of samples), stride (of the
// original's rows in samples, at least size).
enum { kKatOrg8Par = 4 };
static inline int kat_org8_check(const int* q, long long nsamp, int sample_bytes) {
  const int size = q[0], off = q[1], skew = q[2], stride = q[3];
  if (size < 8 || size > kMaxSb || (size & (size - 1)) || skew < 0 || skew >= 16 || skew % sample_bytes || stride < size || stride > 4096) return 1;
  if (off < 0 || off % 16 || (long long)off + size * size > nsamp) return 2;
  return 0;
}
}  // namespace tk
