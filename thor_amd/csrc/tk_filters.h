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

// ---- input at a lower bit depth than the engine's (shift = bitdepth - input_bitdepth > 0) --------------------------------
// The frame enters widened and leaves rounded back, as the reference reads and writes it (common/common_frame.c:484-545, :549-650), and its
// distortion is measured at the input depth (common/snr.c:39-61).  A packed frame is Y, U, V one after the other without row padding; its
// rows are only as aligned as the geometry guarantees (widths are multiples of 8 samples, chroma widths of 4), so a packed luma row moves in
// vectors of 8 samples and a chroma row in vectors of 4.  The frame itself must start on a 16-byte boundary.  One work item per row (Y rows,
// then U, then V) like make_ref_rows; `lane`/`nlanes` stride along the row in those vectors.
template <typename T, int N> struct alignas(N * sizeof(T)) DepthVec { T v[N]; };

// write_yuv_frame / snr_yuv: saturate((v + round) >> shift, input_bitdepth).  Live: 1023 at 10 bits rounds to 256 at 8.
TK_DEV int depth_round(int v, int shift, int maxv) {
  const int r = (v + (1 << (shift - 1))) >> shift;
  return r > maxv ? maxv : r;
}

// Row `it` of a 4:2:0 frame of `planes` against the packed frame `packed`: the plane row, the packed row, the width in samples.
template <typename PIX, typename PK>
TK_DEV void depth_row(const Plane3<PIX>& planes, PK* packed, int width, int height, int it, PIX*& prow, PK*& krow, int& w) {
  const size_t ny = (size_t)width * height, nc = (size_t)(width / 2) * (height / 2);
  if (it < height) { prow = planes.y + (size_t)it * planes.sy; krow = packed + (size_t)it * width; w = width; }
  else if (it < height + height / 2) { const int r = it - height; prow = planes.u + (size_t)r * planes.sc; krow = packed + ny + (size_t)r * (width / 2); w = width / 2; }
  else { const int r = it - height - height / 2; prow = planes.v + (size_t)r * planes.sc; krow = packed + ny + nc + (size_t)r * (width / 2); w = width / 2; }
}

// read_yuv_frame: packed input-depth samples (SRC = uint8_t for depth 8, uint16_t otherwise) -> the engine's planes, v << shift.
template <typename SRC>
TK_DEV void depth_up_rows(const SRC* src, const Plane3<uint16_t>& dst, int width, int height, int shift, int gid, int gsize, int lane, int nlanes) {
  const int total = height + height;  // Y rows + U rows + V rows
  for (int it = gid; it < total; it += gsize) {
    uint16_t* d;
    const SRC* s;
    int w;
    depth_row(dst, src, width, height, it, d, s, w);
    if (it < height)
      for (int i = lane; i < w / 8; i += nlanes) {
        const DepthVec<SRC, 8> a = ((const DepthVec<SRC, 8>*)s)[i];
        DepthVec<uint16_t, 8> o;
        for (int k = 0; k < 8; k++) o.v[k] = (uint16_t)((int)a.v[k] << shift);
        ((DepthVec<uint16_t, 8>*)d)[i] = o;
      }
    else
      for (int i = lane; i < w / 4; i += nlanes) {
        const DepthVec<SRC, 4> a = ((const DepthVec<SRC, 4>*)s)[i];
        DepthVec<uint16_t, 4> o;
        for (int k = 0; k < 4; k++) o.v[k] = (uint16_t)((int)a.v[k] << shift);
        ((DepthVec<uint16_t, 4>*)d)[i] = o;
      }
  }
}

// write_yuv_frame: the engine's planes -> packed input-depth samples (DST = uint8_t for depth 8, uint16_t otherwise), rounded and saturated.
template <typename DST>
TK_DEV void depth_down_rows(const Plane3<uint16_t>& src, DST* dst, int width, int height, int shift, int input_bitdepth, int gid, int gsize, int lane,
                            int nlanes) {
  const int maxv = (1 << input_bitdepth) - 1;
  const int total = height + height;
  for (int it = gid; it < total; it += gsize) {
    uint16_t* s;
    DST* d;
    int w;
    depth_row(src, dst, width, height, it, s, d, w);
    if (it < height)
      for (int i = lane; i < w / 8; i += nlanes) {
        const DepthVec<uint16_t, 8> a = ((const DepthVec<uint16_t, 8>*)s)[i];
        DepthVec<DST, 8> o;
        for (int k = 0; k < 8; k++) o.v[k] = (DST)depth_round(a.v[k], shift, maxv);
        ((DepthVec<DST, 8>*)d)[i] = o;
      }
    else
      for (int i = lane; i < w / 4; i += nlanes) {
        const DepthVec<uint16_t, 4> a = ((const DepthVec<uint16_t, 4>*)s)[i];
        DepthVec<DST, 4> o;
        for (int k = 0; k < 4; k++) o.v[k] = (DST)depth_round(a.v[k], shift, maxv);
        ((DepthVec<DST, 4>*)d)[i] = o;
      }
  }
}

// frame_sse_rows at the input depth, the sum snr_yuv forms: both frames go through the round-and-saturate step before they are subtracted.
// Same work split and exact 64-bit sums; every row, luma too, is read in vectors of 4 samples (8 bytes), which divide every row width, so there is
// no tail loop (a frame's worth of this is ~20 us at 1920x1080: the wider luma vectors of frame_sse_rows would buy nothing).
TK_DEV void frame_sse_depth_rows(const Plane3<uint16_t>& org, const Plane3<uint16_t>& rec, int width, int height, int shift, int input_bitdepth, int gid,
                                 int gsize, int lane, int nlanes, unsigned long long acc[3]) {
  const int maxv = (1 << input_bitdepth) - 1;
  const int total = height + height;
  for (int it = gid; it < total; it += gsize) {
    const int pl = it < height ? 0 : it < height + height / 2 ? 1 : 2;
    const int r = pl == 0 ? it : pl == 1 ? it - height : it - height - height / 2;
    const int w = pl == 0 ? width : width / 2;
    const uint16_t* a = pl == 0 ? org.y + (size_t)r * org.sy : (pl == 1 ? org.u : org.v) + (size_t)r * org.sc;
    const uint16_t* b = pl == 0 ? rec.y + (size_t)r * rec.sy : (pl == 1 ? rec.u : rec.v) + (size_t)r * rec.sc;
    unsigned long long s = 0;
    for (int i = lane; i < w / 4; i += nlanes) {   // 4 samples = 8 bytes: divides every row
      const DepthVec<uint16_t, 4> va = ((const DepthVec<uint16_t, 4>*)a)[i], vb = ((const DepthVec<uint16_t, 4>*)b)[i];
      unsigned int q = 0;  // 4 squares of at most 1023^2
      for (int k = 0; k < 4; k++) { const int d = depth_round(va.v[k], shift, maxv) - depth_round(vb.v[k], shift, maxv); q += (unsigned int)(d * d); }
      s += q;
    }
    acc[0] += pl == 0 ? s : 0;  // constant indices: acc stays in registers on the device
    acc[1] += pl == 1 ? s : 0;
    acc[2] += pl == 2 ? s : 0;
  }
}

// ---- frames in a caller's layout: semi-planar chroma, a row pitch, samples in the high bits (include/thor_hip.h: thor_hip_frame_layout) ------
// What decoders, capture cards and GPU pipelines hand over: NV12 / NV21 for 8 bits, P010 / P012 / P016 above.  The same pass applies the depth
// conversion of the section above, so such a frame becomes the engine's planes, or the reconstruction such a frame, with one read and one write of
// every sample.  Bytes of a row beyond the picture and bytes between planes are neither read nor written.
struct PixLayout {  // a layout resolved against a picture (resolve_layout): no zero left that means "tight", everything in bytes
  int chroma;       // 0: U and V planes, 1: one plane U0 V0 U1 V1 ..., 2: V0 U0 V1 U1 ...
  int msb;          // samples are value << msb (16 - input_bitdepth for P010 / P012 / P016, else 0)
  size_t pitch_y, pitch_c, off_u, off_v;
  size_t bytes;     // from the base to the end of the last row's pitch: what a buffer in this layout holds
};

// The caller's description (0 = tight / adjacent) against a width x height 4:2:0 picture of input_bitdepth samples.  false: the layout is refused.
static inline bool resolve_layout(int chroma, int msb_aligned, long long pitch_y, long long pitch_c, size_t off_u, size_t off_v, int width, int height,
                                  int input_bitdepth, PixLayout& L) {
  const size_t B = input_bitdepth > 8 ? 2 : 1;
  if (chroma < 0 || chroma > 2 || msb_aligned < 0 || msb_aligned > 1 || (msb_aligned && input_bitdepth <= 8)) return false;
  const size_t row_y = (size_t)width * B, row_c = chroma == 0 ? row_y / 2 : row_y;
  if (pitch_y < 0 || pitch_c < 0) return false;
  L.chroma = chroma;
  L.msb = msb_aligned ? 16 - input_bitdepth : 0;
  L.pitch_y = pitch_y ? (size_t)pitch_y : row_y;
  L.pitch_c = pitch_c ? (size_t)pitch_c : row_c;
  if (L.pitch_y < row_y || L.pitch_c < row_c || L.pitch_y % B || L.pitch_c % B || off_u % B || off_v % B) return false;
  const size_t rows_c = (size_t)height / 2;
  L.off_u = off_u ? off_u : L.pitch_y * height;
  L.off_v = chroma == 0 ? (off_v ? off_v : L.off_u + L.pitch_c * rows_c) : 0;
  L.bytes = L.pitch_y * height;
  if (L.off_u + L.pitch_c * rows_c > L.bytes) L.bytes = L.off_u + L.pitch_c * rows_c;
  if (chroma == 0 && L.off_v + L.pitch_c * rows_c > L.bytes) L.bytes = L.off_v + L.pitch_c * rows_c;
  return true;
}

// N samples moved as one: 16 bytes on the layout side (one dwordx4), as much as that makes on the plane side.
template <typename T, int N> struct alignas(N * sizeof(T) < 16 ? N * sizeof(T) : 16) LayoutVec { T v[N]; };

template <typename SRC, typename PIX> TK_DEV PIX layout_in_sample(SRC s, int msb, int up) { return (PIX)((((int)s) >> msb) << up); }
template <typename PIX, typename DST> TK_DEV DST layout_out_sample(PIX v, int shift, int maxv, int msb) {
  const int r = shift > 0 ? depth_round((int)v, shift, maxv) : (int)v;
  return (DST)(r << msb);
}

// One row of n samples, layout -> plane.  vec: `s` and its pitch are 16-byte aligned (plane rows always are); whole vectors first, the rest of
// the row (n is a multiple of 4 only) sample by sample.
template <typename SRC, typename PIX> TK_DEV void layout_in_run(const SRC* s, PIX* d, int n, int msb, int up, bool vec, int lane, int nlanes) {
  constexpr int N = 16 / (int)sizeof(SRC);
  const int nv = vec ? n / N : 0;
  for (int i = lane; i < nv; i += nlanes) {
    const LayoutVec<SRC, N> a = ((const LayoutVec<SRC, N>*)s)[i];
    LayoutVec<PIX, N> o;
    for (int k = 0; k < N; k++) o.v[k] = layout_in_sample<SRC, PIX>(a.v[k], msb, up);
    ((LayoutVec<PIX, N>*)d)[i] = o;
  }
  for (int i = nv * N + lane; i < n; i += nlanes) d[i] = layout_in_sample<SRC, PIX>(s[i], msb, up);
}
// One row of n interleaved pairs -> rows d0 (first of each pair) and d1: a vector of pairs in, two half-width vectors out.
template <typename SRC, typename PIX> TK_DEV void layout_in_pairs(const SRC* s, PIX* d0, PIX* d1, int n, int msb, int up, bool vec, int lane, int nlanes) {
  constexpr int N = 8 / (int)sizeof(SRC);
  const int nv = vec ? n / N : 0;
  for (int i = lane; i < nv; i += nlanes) {
    const LayoutVec<SRC, 2 * N> a = ((const LayoutVec<SRC, 2 * N>*)s)[i];
    LayoutVec<PIX, N> o0, o1;
    for (int k = 0; k < N; k++) { o0.v[k] = layout_in_sample<SRC, PIX>(a.v[2 * k], msb, up); o1.v[k] = layout_in_sample<SRC, PIX>(a.v[2 * k + 1], msb, up); }
    ((LayoutVec<PIX, N>*)d0)[i] = o0;
    ((LayoutVec<PIX, N>*)d1)[i] = o1;
  }
  for (int i = nv * N + lane; i < n; i += nlanes) { d0[i] = layout_in_sample<SRC, PIX>(s[2 * i], msb, up); d1[i] = layout_in_sample<SRC, PIX>(s[2 * i + 1], msb, up); }
}
// The two above the other way: plane -> layout, rounded back to the input depth when shift > 0.
template <typename PIX, typename DST>
TK_DEV void layout_out_run(const PIX* s, DST* d, int n, int shift, int maxv, int msb, bool vec, int lane, int nlanes) {
  constexpr int N = 16 / (int)sizeof(DST);
  const int nv = vec ? n / N : 0;
  for (int i = lane; i < nv; i += nlanes) {
    const LayoutVec<PIX, N> a = ((const LayoutVec<PIX, N>*)s)[i];
    LayoutVec<DST, N> o;
    for (int k = 0; k < N; k++) o.v[k] = layout_out_sample<PIX, DST>(a.v[k], shift, maxv, msb);
    ((LayoutVec<DST, N>*)d)[i] = o;
  }
  for (int i = nv * N + lane; i < n; i += nlanes) d[i] = layout_out_sample<PIX, DST>(s[i], shift, maxv, msb);
}
template <typename PIX, typename DST>
TK_DEV void layout_out_pairs(const PIX* s0, const PIX* s1, DST* d, int n, int shift, int maxv, int msb, bool vec, int lane, int nlanes) {
  constexpr int N = 8 / (int)sizeof(DST);
  const int nv = vec ? n / N : 0;
  for (int i = lane; i < nv; i += nlanes) {
    const LayoutVec<PIX, N> a0 = ((const LayoutVec<PIX, N>*)s0)[i], a1 = ((const LayoutVec<PIX, N>*)s1)[i];
    LayoutVec<DST, 2 * N> o;
    for (int k = 0; k < N; k++) { o.v[2 * k] = layout_out_sample<PIX, DST>(a0.v[k], shift, maxv, msb); o.v[2 * k + 1] = layout_out_sample<PIX, DST>(a1.v[k], shift, maxv, msb); }
    ((LayoutVec<DST, 2 * N>*)d)[i] = o;
  }
  for (int i = nv * N + lane; i < n; i += nlanes) { d[2 * i] = layout_out_sample<PIX, DST>(s0[i], shift, maxv, msb); d[2 * i + 1] = layout_out_sample<PIX, DST>(s1[i], shift, maxv, msb); }
}

// Whether the rows that start at base + off and follow each other at `pitch` all lie on 16-byte boundaries.
TK_DEV bool layout_rows_aligned(const void* base, size_t off, size_t pitch) { return ((((uintptr_t)base + off) | pitch) & 15) == 0; }

// A frame at `base` in layout L (SRC = uint8_t for input depth 8, uint16_t otherwise) -> the engine's planes: x = s >> L.msb, plane sample x << up
// (up = bitdepth - input_bitdepth, depth_up_rows' widening).  One work item per luma row, then one per chroma row (its U and its V samples);
// `lane`/`nlanes` stride along the row.
template <typename SRC, typename PIX>
TK_DEV void layout_in_rows(const void* base, const PixLayout& L, const Plane3<PIX>& dst, int width, int height, int up, int gid, int gsize, int lane,
                           int nlanes) {
  const uint8_t* b = (const uint8_t*)base;
  const bool vy = layout_rows_aligned(b, 0, L.pitch_y);
  const bool vc = layout_rows_aligned(b, L.off_u, L.pitch_c) && (L.chroma != 0 || layout_rows_aligned(b, L.off_v, L.pitch_c));
  const int total = height + height / 2;
  for (int it = gid; it < total; it += gsize) {
    if (it < height) {
      layout_in_run((const SRC*)(b + (size_t)it * L.pitch_y), dst.y + (size_t)it * dst.sy, width, L.msb, up, vy, lane, nlanes);
      continue;
    }
    const size_t r = (size_t)(it - height);
    PIX* du = dst.u + r * dst.sc;
    PIX* dv = dst.v + r * dst.sc;
    const SRC* su = (const SRC*)(b + L.off_u + r * L.pitch_c);
    if (L.chroma == 0) {
      layout_in_run(su, du, width / 2, L.msb, up, vc, lane, nlanes);
      layout_in_run((const SRC*)(b + L.off_v + r * L.pitch_c), dv, width / 2, L.msb, up, vc, lane, nlanes);
    } else
      layout_in_pairs(su, L.chroma == 1 ? du : dv, L.chroma == 1 ? dv : du, width / 2, L.msb, up, vc, lane, nlanes);
  }
}

// The engine's planes -> a frame at `base` in layout L (DST = uint8_t for input depth 8, uint16_t otherwise): r = depth_round(v, shift, max) when
// shift = bitdepth - input_bitdepth > 0, else v; written r << L.msb.  Same work split.
template <typename PIX, typename DST>
TK_DEV void layout_out_rows(const Plane3<PIX>& src, void* base, const PixLayout& L, int width, int height, int shift, int input_bitdepth, int gid, int gsize,
                            int lane, int nlanes) {
  uint8_t* b = (uint8_t*)base;
  const int maxv = (1 << input_bitdepth) - 1;
  const bool vy = layout_rows_aligned(b, 0, L.pitch_y);
  const bool vc = layout_rows_aligned(b, L.off_u, L.pitch_c) && (L.chroma != 0 || layout_rows_aligned(b, L.off_v, L.pitch_c));
  const int total = height + height / 2;
  for (int it = gid; it < total; it += gsize) {
    if (it < height) {
      layout_out_run(src.y + (size_t)it * src.sy, (DST*)(b + (size_t)it * L.pitch_y), width, shift, maxv, L.msb, vy, lane, nlanes);
      continue;
    }
    const size_t r = (size_t)(it - height);
    const PIX* su = src.u + r * src.sc;
    const PIX* sv = src.v + r * src.sc;
    DST* du = (DST*)(b + L.off_u + r * L.pitch_c);
    if (L.chroma == 0) {
      layout_out_run(su, du, width / 2, shift, maxv, L.msb, vc, lane, nlanes);
      layout_out_run(sv, (DST*)(b + L.off_v + r * L.pitch_c), width / 2, shift, maxv, L.msb, vc, lane, nlanes);
    } else
      layout_out_pairs(L.chroma == 1 ? su : sv, L.chroma == 1 ? sv : su, du, width / 2, shift, maxv, L.msb, vc, lane, nlanes);
  }
}

}  // namespace tk
