// tk_filters.h - frame-level in-loop filters and reference-frame creation, work-item parallel.
// Specification followed: common/common_frame.c:47-352 (deblock_frame_y, MODIFIED_DEBLOCK_TEST /
// NEW_MV_TEST / NEW_DEBLOCK_FILTER variants as compiled), :354-433 (deblock_frame_uv), :657-763
// (pad_yuv_frame / create_reference_frame).  Every 8-sample edge segment is independent inside
// one pass (it touches only rows/cols within +-2 of its own edge and reads its decision pixels
// before writing), so a pass is a flat parallel loop; vertical edges complete before horizontal.
#pragma once
#include "tk_common.h"

namespace tk {

struct DbParams {
  int width, height, bitdepth;
  int beta, tc_y, tc_c;
  const DbCell* cells;
  int cs;
};

TK_DEV int cell_mvbig(const DbCell& c) {
  return iabs(c.mv0.y) >= 4 || iabs(c.mv0.x) >= 4 || iabs(c.mv1.y) >= 4 || iabs(c.mv1.x) >= 4;
}

// One luma edge segment. dir 0: vertical edge at x = 8*bj (bj >= 1), rows 8*bi..+7;
// dir 1: horizontal edge at y = 8*bi (bi >= 1), cols 8*bj..+7.
template <typename PIX>
TK_DEV void deblock_y_segment(PIX* rec, int stride, const DbParams& P, int bi, int bj, int dir) {
  const int i = bi * 8, j = bj * 8;
  // step along the edge (a) and across it (x)
  const int sa = dir == 0 ? stride : 1;
  const int sx = dir == 0 ? 1 : stride;
  PIX* e = rec + i * stride + j;  // q0 of line 0
  auto dline = [&](int l) -> int {
    const PIX* p = e + l * sa;
    return iabs((int)p[-2 * sx] - (int)p[-sx]) + iabs((int)p[sx] - (int)p[0]);
  };
  const int d15 = dline(1) + dline(5);
  const int d26 = dline(2) + dline(6);
  for (int m = 0; m < 8; m += 4) {
    const int qi = dir == 0 ? ((i + m) / 4) * P.cs + j / 4 : (i / 4) * P.cs + (j + m) / 4;
    const int pi = dir == 0 ? qi - 1 : qi - P.cs;
    const DbCell& q = P.cells[qi];
    const DbCell& p = P.cells[pi];
    int q_size = q.size;
    const int tbs = q.tbpb & 1, pb = q.tbpb >> 1;
    if ((tbs || pb == (dir == 0 ? P_VER : P_HOR) || pb == P_QUAD) && q_size > kMinBlk) q_size /= 2;
    const int mv = cell_mvbig(p) || cell_mvbig(q);
    const int cbp = (p.cbp & 1) || (q.cbp & 1);
    const int mode = p.mode == M_INTRA || q.mode == M_INTRA;
    const int interior = ((dir == 0 ? j : i) % q_size) > 0;
    if (interior || !(mv || cbp || mode)) continue;
    for (int k = m; k < m + 4; k++) {
      const int d = (k & 1) ? d26 : d15;
      if (d >= P.beta) continue;
      PIX* l = e + k * sa;
      const int p1 = l[-2 * sx], p0 = l[-sx], q0 = l[0], q1 = l[sx];
      int delta = (18 * (q0 - p0) - 6 * (q1 - p1) + 16) >> 5;
      delta = clampi(delta, -P.tc_y, P.tc_y);
      l[-2 * sx] = (PIX)sat_pix(p1 + delta / 2, P.bitdepth);
      l[-sx] = (PIX)sat_pix(p0 + delta, P.bitdepth);
      l[0] = (PIX)sat_pix(q0 - delta, P.bitdepth);
      l[sx] = (PIX)sat_pix(q1 - delta / 2, P.bitdepth);
    }
  }
}

// One chroma edge segment (4 chroma samples) of plane `rec` (4:2:0), same (bi,bj,dir) grid as luma.
template <typename PIX>
TK_DEV void deblock_c_segment(PIX* rec, int stride, const DbParams& P, int bi, int bj, int dir) {
  const int i = bi * 8, j = bj * 8;
  const int qi = (i / 4) * P.cs + j / 4;
  const int pi = dir == 0 ? qi - 1 : qi - P.cs;
  const DbCell& q = P.cells[qi];
  const DbCell& p = P.cells[pi];
  const int mode = p.mode == M_INTRA || q.mode == M_INTRA;
  const int interior = ((dir == 0 ? j : i) % (int)q.size) > 0;
  if (interior || !mode) return;
  const int sa = dir == 0 ? stride : 1;
  const int sx = dir == 0 ? 1 : stride;
  PIX* e = rec + (i >> 1) * stride + (j >> 1);
  for (int k = 0; k < 4; k++) {
    PIX* l = e + k * sa;
    const int p1 = l[-2 * sx], p0 = l[-sx], q0 = l[0], q1 = l[sx];
    int delta = (4 * (q0 - p0) + (p1 - q1) + 4) >> 3;
    delta = clampi(delta, -P.tc_c, P.tc_c);
    l[-sx] = (PIX)sat_pix(p0 + delta, P.bitdepth);
    l[0] = (PIX)sat_pix(q0 - delta, P.bitdepth);
  }
}

// pass: 0 = Y vertical, 1 = Y horizontal, 2 = UV vertical, 3 = UV horizontal.
template <typename PIX>
TK_DEV void deblock_pass(const Plane3<PIX>& rec, const DbParams& P, int pass, int gid, int gsize) {
  const int nbi = P.height / 8, nbj = P.width / 8;
  const int dir = pass & 1;
  const int n = nbi * nbj;
  for (int it = gid; it < n; it += gsize) {
    const int bi = it / nbj, bj = it - bi * nbj;
    if (dir == 0 && bj == 0) continue;
    if (dir == 1 && bi == 0) continue;
    if (pass < 2) deblock_y_segment(rec.y, rec.sy, P, bi, bj, dir);
    else {
      deblock_c_segment(rec.u, rec.sc, P, bi, bj, dir);
      deblock_c_segment(rec.v, rec.sc, P, bi, bj, dir);
    }
  }
}

// create_reference_frame: copy + replicate-pad (pad luma 160, chroma 80).
// One work item per padded row (Y rows, then U, then V); `lane`/`nlanes` stride along the row.
template <typename PIX>
TK_DEV void make_ref_rows(const Plane3<PIX>& rec, const Plane3<PIX>& ref, int width, int height, int gid, int gsize,
                          int lane, int nlanes) {
  const int py = kPadY, pc = kPadY / 2;
  const int hy = height + 2 * py, hc = height / 2 + 2 * pc;
  const int total = hy + 2 * hc;
  for (int it = gid; it < total; it += gsize) {
    const PIX* src;
    PIX* dst;
    int w, h, pad, ss, ds, row;
    if (it < hy) { row = it - py; src = rec.y; dst = ref.y; w = width; h = height; pad = py; ss = rec.sy; ds = ref.sy; }
    else if (it < hy + hc) { row = it - hy - pc; src = rec.u; dst = ref.u; w = width / 2; h = height / 2; pad = pc; ss = rec.sc; ds = ref.sc; }
    else { row = it - hy - hc - pc; src = rec.v; dst = ref.v; w = width / 2; h = height / 2; pad = pc; ss = rec.sc; ds = ref.sc; }
    const int sr = clampi(row, 0, h - 1);
    const PIX* s = src + sr * ss;
    PIX* d = dst + row * ds;
    for (int x = -pad + lane; x < w + pad; x += nlanes) d[x] = s[clampi(x, 0, w - 1)];
  }
}

// Sum of squared differences between the original and the final reconstruction, per plane (the sums snr_yuv, common/snr.c:32-99,
// turns into PSNR; bitdepth == input_bitdepth, so no shifts).  One work item per row (Y rows, then U, then V) like make_ref_rows;
// `lane`/`nlanes` stride along the row in vectors of 16 bytes, the tail (chroma widths are multiples of 4, not of 16 bytes) in
// vectors of 4 samples.  Rows must start 16-byte aligned (DevFrame strides are multiples of 16 samples).  Adds into acc[plane]:
// exact 64-bit sums (at 12 bits one square is up to 4095^2, a 32-bit sum of a row would overflow after 257 samples).
template <typename PIX>
TK_DEV void frame_sse_rows(const Plane3<PIX>& org, const Plane3<PIX>& rec, int width, int height, int gid, int gsize, int lane, int nlanes,
                           unsigned long long acc[3]) {
  constexpr int kV = 16 / (int)sizeof(PIX);
  struct alignas(16) V16 { PIX v[kV]; };
  struct alignas(4 * sizeof(PIX)) V4 { PIX v[4]; };
  const int total = height + height;  // Y rows + U rows + V rows
  for (int it = gid; it < total; it += gsize) {
    const PIX* a;
    const PIX* b;
    int w, pl;
    if (it < height) { a = org.y + (size_t)it * org.sy; b = rec.y + (size_t)it * rec.sy; w = width; pl = 0; }
    else if (it < height + height / 2) { const int r = it - height; a = org.u + (size_t)r * org.sc; b = rec.u + (size_t)r * rec.sc; w = width / 2; pl = 1; }
    else { const int r = it - height - height / 2; a = org.v + (size_t)r * org.sc; b = rec.v + (size_t)r * rec.sc; w = width / 2; pl = 2; }
    const int nv = w / kV;
    unsigned long long s = 0;
    for (int i = lane; i < nv; i += nlanes) {
      const V16 va = ((const V16*)a)[i], vb = ((const V16*)b)[i];
      unsigned int q = 0;  // at most 8 squares of 4095^2 < 2^28
      for (int k = 0; k < kV; k++) { const int d = (int)va.v[k] - (int)vb.v[k]; q += (unsigned int)(d * d); }
      s += q;
    }
    for (int i = nv * (kV / 4) + lane; i < w / 4; i += nlanes) {
      const V4 va = ((const V4*)a)[i], vb = ((const V4*)b)[i];
      unsigned int q = 0;
      for (int k = 0; k < 4; k++) { const int d = (int)va.v[k] - (int)vb.v[k]; q += (unsigned int)(d * d); }
      s += q;
    }
    acc[0] += pl == 0 ? s : 0;  // constant indices: acc stays in registers on the device
    acc[1] += pl == 1 ? s : 0;
    acc[2] += pl == 2 ? s : 0;
  }
}

}  // namespace tk
