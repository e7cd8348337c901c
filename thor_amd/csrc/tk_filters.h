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

// ---- RGB frames: colour conversion and 4:2:0 downsampling at the boundary (include/thor_hip.h: thor_hip_rgb_format) -------------------------------
// What screen capture, renderers and tensor pipelines hold.  Staging an RGB frame is converting it to a planar 4:2:0 frame of input_bitdepth
// samples and staging that; fetching is the inverse of the reconstruction rounded back to input_bitdepth.  Integers only; the coefficients are
// derived once per (format, input_bitdepth) on the host (resolve_rgb) and travel by value.  The formulas are spelled out in include/thor_hip.h.
enum { RGB_FWD_BITS = 24, RGB_INV_BITS = 20 };
struct RgbFormat {  // a thor_hip_rgb_format resolved against a picture and an input depth
  int kind;         // 0: four samples per pixel, 1: three samples per pixel, 2: three planes R, G, B
  int lead;         // four samples per pixel: 1 when the unused one comes first (ARGB / ABGR)
  int swap;         // packed: 1 when blue comes before red (BGRA / ABGR / BGR)
  int sbytes;       // bytes per sample of the RGB side: 1 (depth 8) or 2
  int msb;          // samples are value << msb (16 - depth when msb_aligned, else 0)
  int maxv;         // 2^depth - 1
  int site;         // 0: chroma at the centre of its 2x2 quad, 1: at the left column ([1 2 1] / 4 horizontally, left edge replicated)
  size_t pitch, plane, bytes;   // bytes between rows, between planes (kind 2), from the base to the end of the frame
  int oy, oc, maxo;             // luma offset, chroma offset, 2^input_bitdepth - 1
  int yr, yg, yb, ur, ug, ub, vr, vg, vb;  // RGB -> Y'CbCr, RGB_FWD_BITS fractional bits; ur + ug + ub == vr + vg + vb == 0
  int iy, rv, gu, gv, bu;                  // Y'CbCr -> RGB, RGB_INV_BITS fractional bits
};

// round(a / b) for a >= 0, b > 0, halves up
static inline long long rgb_rdiv(long long a, long long b) { return (2 * a + b) / (2 * b); }

// The caller's description against a width x height picture whose 4:2:0 samples have input_bitdepth bits.  false: the format is refused.
static inline bool resolve_rgb(int order, int depth, int msb_aligned, int matrix, int full_range, int chroma_site, long long pitch, size_t plane_stride,
                               int width, int height, int input_bitdepth, RgbFormat& R) {
  static const int K[3][2] = {{2990, 1140}, {2126, 722}, {2627, 593}};  // Kr, Kb over 10000: BT.601, BT.709, BT.2020 (Kg = 10000 - Kr - Kb)
  if (order < 0 || order > 6 || (depth != 8 && depth != 10 && depth != 12 && depth != 16)) return false;
  if (msb_aligned < 0 || msb_aligned > 1 || (msb_aligned && depth != 10 && depth != 12)) return false;
  if (matrix < 0 || matrix > 2 || full_range < 0 || full_range > 1 || chroma_site < 0 || chroma_site > 1 || pitch < 0) return false;
  if (width < 16 || height < 16 || width % 8 || height % 8 || (input_bitdepth != 8 && input_bitdepth != 10 && input_bitdepth != 12)) return false;
  R.kind = order < 4 ? 0 : order < 6 ? 1 : 2;
  R.lead = order == 2 || order == 3;
  R.swap = order == 1 || order == 3 || order == 5;
  R.sbytes = depth > 8 ? 2 : 1;
  R.msb = msb_aligned ? 16 - depth : 0;
  R.maxv = (1 << depth) - 1;
  R.site = chroma_site;
  const size_t row = (size_t)width * R.sbytes * (R.kind == 0 ? 4 : R.kind == 1 ? 3 : 1);
  R.pitch = pitch ? (size_t)pitch : row;
  if (R.pitch < row || R.pitch % R.sbytes || plane_stride % R.sbytes || (plane_stride && R.kind != 2)) return false;
  R.plane = R.kind == 2 ? (plane_stride ? plane_stride : R.pitch * height) : 0;
  if (R.kind == 2 && R.plane < R.pitch * height) return false;
  R.bytes = R.kind == 2 ? 2 * R.plane + R.pitch * height : R.pitch * height;
  const int n = input_bitdepth;
  const long long M = R.maxv, kr = K[matrix][0], kb = K[matrix][1], kg = 10000 - kr - kb;
  const long long SY = full_range ? (1 << n) - 1 : 219 << (n - 8), SC = full_range ? (1 << n) - 1 : 224 << (n - 8);
  R.oy = full_range ? 0 : 16 << (n - 8);
  R.oc = 1 << (n - 1);
  R.maxo = (1 << n) - 1;
  const int F = RGB_FWD_BITS, G = RGB_INV_BITS;
  R.yr = (int)rgb_rdiv((kr * SY) << F, 10000 * M);
  R.yb = (int)rgb_rdiv((kb * SY) << F, 10000 * M);
  R.yg = (int)rgb_rdiv(SY << F, M) - R.yr - R.yb;
  R.ub = (int)rgb_rdiv(SC << F, 2 * M);
  R.ur = -(int)rgb_rdiv((kr * SC) << F, 2 * (10000 - kb) * M);
  R.ug = -R.ub - R.ur;
  R.vr = (int)rgb_rdiv(SC << F, 2 * M);
  R.vb = -(int)rgb_rdiv((kb * SC) << F, 2 * (10000 - kr) * M);
  R.vg = -R.vr - R.vb;
  R.iy = (int)rgb_rdiv(M << G, SY);
  R.rv = (int)rgb_rdiv((2 * (10000 - kr) * M) << G, 10000 * SC);
  R.bu = (int)rgb_rdiv((2 * (10000 - kb) * M) << G, 10000 * SC);
  R.gu = -(int)rgb_rdiv((2 * kb * (10000 - kb) * M) << G, 10000 * kg * SC);
  R.gv = -(int)rgb_rdiv((2 * kr * (10000 - kr) * M) << G, 10000 * kg * SC);
  return true;
}

TK_DEV int rgb_clamp(long long v, int maxv) { return v < 0 ? 0 : v > maxv ? maxv : (int)v; }
TK_DEV int rgb_luma(const RgbFormat& R, int r, int g, int b) {
  const long long a = (long long)R.yr * r + (long long)R.yg * g + (long long)R.yb * b + ((long long)R.oy << RGB_FWD_BITS) + (1ll << (RGB_FWD_BITS - 1));
  return rgb_clamp(a >> RGB_FWD_BITS, R.maxo);
}
// tr, tg, tb: the sums over the chroma sample's taps (weights adding up to 1 << taps_log2): one rounding for the whole sum
TK_DEV int rgb_chroma(const RgbFormat& R, int cr, int cg, int cb, int tr, int tg, int tb, int taps_log2) {
  const int sh = RGB_FWD_BITS + taps_log2;
  const long long a = (long long)cr * tr + (long long)cg * tg + (long long)cb * tb + ((long long)R.oc << sh) + (1ll << (sh - 1));
  return rgb_clamp(a >> sh, R.maxo);
}
TK_DEV void rgb_inverse(const RgbFormat& R, int y, int u, int v, int& r, int& g, int& b) {
  const long long l = (long long)R.iy * (y - R.oy) + (1ll << (RGB_INV_BITS - 1));
  r = rgb_clamp((l + (long long)R.rv * (v - R.oc)) >> RGB_INV_BITS, R.maxv);
  g = rgb_clamp((l + (long long)R.gu * (u - R.oc) + (long long)R.gv * (v - R.oc)) >> RGB_INV_BITS, R.maxv);
  b = rgb_clamp((l + (long long)R.bu * (u - R.oc)) >> RGB_INV_BITS, R.maxv);
}

// Pixel x of the row at `row`, sample by sample.
template <typename SRC> TK_DEV void rgb_load_px(const uint8_t* row, const RgbFormat& R, int x, int& r, int& g, int& b) {
  if (R.kind == 2) {
    r = ((const SRC*)row)[x] >> R.msb; g = ((const SRC*)(row + R.plane))[x] >> R.msb; b = ((const SRC*)(row + 2 * R.plane))[x] >> R.msb;
    return;
  }
  const SRC* p = (const SRC*)row + (size_t)x * (R.kind == 0 ? 4 : 3) + R.lead;
  const int c0 = p[0] >> R.msb, c2 = p[2] >> R.msb;
  r = R.swap ? c2 : c0; g = p[1] >> R.msb; b = R.swap ? c0 : c2;
}
template <typename DST> TK_DEV void rgb_store_px(uint8_t* row, const RgbFormat& R, int x, int r, int g, int b) {
  if (R.kind == 2) {
    ((DST*)row)[x] = (DST)(r << R.msb); ((DST*)(row + R.plane))[x] = (DST)(g << R.msb); ((DST*)(row + 2 * R.plane))[x] = (DST)(b << R.msb);
    return;
  }
  DST* p = (DST*)row + (size_t)x * (R.kind == 0 ? 4 : 3);
  if (R.kind == 0) p[R.lead ? 0 : 3] = (DST)(R.maxv << R.msb);
  p += R.lead;
  p[0] = (DST)((R.swap ? b : r) << R.msb); p[1] = (DST)(g << R.msb); p[2] = (DST)((R.swap ? r : b) << R.msb);
}

// Pixels per lane step.  With whole vectors: 16 bytes of a four-sample row (4 pixels of bytes, 2 of 16-bit words), the three dwords that hold as many
// pixels of a three-sample row, 16 bytes of each plane of a planar frame; sample by sample: one 2x2 quad.
template <typename S, int KIND, bool VEC> struct RgbRun { static constexpr int P = !VEC ? 2 : KIND == 2 ? 16 / (int)sizeof(S) : 4 / (int)sizeof(S); };

// Sample j of the 3 * P samples that three dwords hold (little-endian).
template <typename S> TK_DEV int rgb_dword_sample(const uint32_t* w, int j) {
  constexpr int per = 4 / (int)sizeof(S);
  return (int)((w[j / per] >> (8 * (int)sizeof(S) * (j % per))) & (sizeof(S) == 1 ? 0xffu : 0xffffu));
}

// Luma rows 2 * crow and 2 * crow + 1, pixels x0 .. x0 + P - 1, with their P / 2 chroma samples: RGB -> planes.  x0 is a multiple of P.
template <typename SRC, typename PIX, int KIND, bool VEC>
TK_DEV void rgb_in_span(const uint8_t* base, const RgbFormat& R, const Plane3<PIX>& dst, int up, int crow, int x0) {
  constexpr int P = RgbRun<SRC, KIND, VEC>::P;
  int r[2][P], g[2][P], b[2][P], lr[2] = {0, 0}, lg[2] = {0, 0}, lb[2] = {0, 0};
  for (int q = 0; q < 2; q++) {
    const uint8_t* row = base + (size_t)(2 * crow + q) * R.pitch;
    if constexpr (!VEC) {
      for (int k = 0; k < P; k++) rgb_load_px<SRC>(row, R, x0 + k, r[q][k], g[q][k], b[q][k]);
    } else if constexpr (KIND == 0) {
      const LayoutVec<SRC, 4 * P> a = *(const LayoutVec<SRC, 4 * P>*)(row + (size_t)x0 * 4 * sizeof(SRC));
      for (int k = 0; k < P; k++) {
        const int c0 = (R.lead ? a.v[4 * k + 1] : a.v[4 * k]) >> R.msb, c2 = (R.lead ? a.v[4 * k + 3] : a.v[4 * k + 2]) >> R.msb;
        r[q][k] = R.swap ? c2 : c0; g[q][k] = (R.lead ? a.v[4 * k + 2] : a.v[4 * k + 1]) >> R.msb; b[q][k] = R.swap ? c0 : c2;
      }
    } else if constexpr (KIND == 1) {
      const uint32_t* wp = (const uint32_t*)(row + (size_t)x0 * 3 * sizeof(SRC));
      const uint32_t w[3] = {wp[0], wp[1], wp[2]};
      for (int k = 0; k < P; k++) {
        const int c0 = rgb_dword_sample<SRC>(w, 3 * k) >> R.msb, c2 = rgb_dword_sample<SRC>(w, 3 * k + 2) >> R.msb;
        r[q][k] = R.swap ? c2 : c0; g[q][k] = rgb_dword_sample<SRC>(w, 3 * k + 1) >> R.msb; b[q][k] = R.swap ? c0 : c2;
      }
    } else {
      const LayoutVec<SRC, P> ar = *(const LayoutVec<SRC, P>*)(row + (size_t)x0 * sizeof(SRC));
      const LayoutVec<SRC, P> ag = *(const LayoutVec<SRC, P>*)(row + R.plane + (size_t)x0 * sizeof(SRC));
      const LayoutVec<SRC, P> ab = *(const LayoutVec<SRC, P>*)(row + 2 * R.plane + (size_t)x0 * sizeof(SRC));
      for (int k = 0; k < P; k++) { r[q][k] = ar.v[k] >> R.msb; g[q][k] = ag.v[k] >> R.msb; b[q][k] = ab.v[k] >> R.msb; }
    }
    if (R.site) rgb_load_px<SRC>(row, R, x0 ? x0 - 1 : 0, lr[q], lg[q], lb[q]);  // the tap one column back, within the same rows
  }
  PIX yo[2][P], uo[P / 2], vo[P / 2];
  for (int q = 0; q < 2; q++)
    for (int k = 0; k < P; k++) yo[q][k] = (PIX)(rgb_luma(R, r[q][k], g[q][k], b[q][k]) << up);
  for (int j = 0; j < P / 2; j++) {
    int tr = 0, tg = 0, tb = 0;
    for (int q = 0; q < 2; q++) {
      if (R.site) {
        tr += (j ? r[q][2 * j - 1] : lr[q]) + 2 * r[q][2 * j] + r[q][2 * j + 1];
        tg += (j ? g[q][2 * j - 1] : lg[q]) + 2 * g[q][2 * j] + g[q][2 * j + 1];
        tb += (j ? b[q][2 * j - 1] : lb[q]) + 2 * b[q][2 * j] + b[q][2 * j + 1];
      } else {
        tr += r[q][2 * j] + r[q][2 * j + 1]; tg += g[q][2 * j] + g[q][2 * j + 1]; tb += b[q][2 * j] + b[q][2 * j + 1];
      }
    }
    uo[j] = (PIX)(rgb_chroma(R, R.ur, R.ug, R.ub, tr, tg, tb, R.site ? 3 : 2) << up);
    vo[j] = (PIX)(rgb_chroma(R, R.vr, R.vg, R.vb, tr, tg, tb, R.site ? 3 : 2) << up);
  }
  PIX* dy = dst.y + (size_t)(2 * crow) * dst.sy + x0;
  PIX* du = dst.u + (size_t)crow * dst.sc + x0 / 2;
  PIX* dv = dst.v + (size_t)crow * dst.sc + x0 / 2;
  if constexpr (VEC) {  // plane rows are 16-byte aligned and x0 is a multiple of P
    LayoutVec<PIX, P> o0, o1;
    LayoutVec<PIX, P / 2> ou, ov;
    for (int k = 0; k < P; k++) { o0.v[k] = yo[0][k]; o1.v[k] = yo[1][k]; }
    for (int j = 0; j < P / 2; j++) { ou.v[j] = uo[j]; ov.v[j] = vo[j]; }
    *(LayoutVec<PIX, P>*)dy = o0; *(LayoutVec<PIX, P>*)(dy + dst.sy) = o1;
    *(LayoutVec<PIX, P / 2>*)du = ou; *(LayoutVec<PIX, P / 2>*)dv = ov;
  } else {
    for (int k = 0; k < P; k++) { dy[k] = yo[0][k]; dy[dst.sy + k] = yo[1][k]; }
    for (int j = 0; j < P / 2; j++) { du[j] = uo[j]; dv[j] = vo[j]; }
  }
}

// The same span the other way: planes -> RGB, chroma replicated over its quad, the reconstruction rounded back to the input depth first.
template <typename PIX, typename DST, int KIND, bool VEC>
TK_DEV void rgb_out_span(const Plane3<PIX>& src, uint8_t* base, const RgbFormat& R, int shift, int crow, int x0) {
  constexpr int P = RgbRun<DST, KIND, VEC>::P;
  int y[2][P], u[P / 2], v[P / 2];
  const PIX* sy = src.y + (size_t)(2 * crow) * src.sy + x0;
  const PIX* su = src.u + (size_t)crow * src.sc + x0 / 2;
  const PIX* sv = src.v + (size_t)crow * src.sc + x0 / 2;
  if constexpr (VEC) {
    const LayoutVec<PIX, P> a0 = *(const LayoutVec<PIX, P>*)sy, a1 = *(const LayoutVec<PIX, P>*)(sy + src.sy);
    const LayoutVec<PIX, P / 2> au = *(const LayoutVec<PIX, P / 2>*)su, av = *(const LayoutVec<PIX, P / 2>*)sv;
    for (int k = 0; k < P; k++) { y[0][k] = a0.v[k]; y[1][k] = a1.v[k]; }
    for (int j = 0; j < P / 2; j++) { u[j] = au.v[j]; v[j] = av.v[j]; }
  } else {
    for (int k = 0; k < P; k++) { y[0][k] = sy[k]; y[1][k] = sy[src.sy + k]; }
    for (int j = 0; j < P / 2; j++) { u[j] = su[j]; v[j] = sv[j]; }
  }
  if (shift > 0) {
    for (int k = 0; k < P; k++) { y[0][k] = depth_round(y[0][k], shift, R.maxo); y[1][k] = depth_round(y[1][k], shift, R.maxo); }
    for (int j = 0; j < P / 2; j++) { u[j] = depth_round(u[j], shift, R.maxo); v[j] = depth_round(v[j], shift, R.maxo); }
  }
  for (int q = 0; q < 2; q++) {
    uint8_t* row = base + (size_t)(2 * crow + q) * R.pitch;
    int r[P], g[P], b[P];
    for (int k = 0; k < P; k++) rgb_inverse(R, y[q][k], u[k / 2], v[k / 2], r[k], g[k], b[k]);
    if constexpr (!VEC) {
      for (int k = 0; k < P; k++) rgb_store_px<DST>(row, R, x0 + k, r[k], g[k], b[k]);
    } else if constexpr (KIND == 0) {
      LayoutVec<DST, 4 * P> o;
      const int one = R.maxv << R.msb;
      for (int k = 0; k < P; k++) {
        const int c0 = (R.swap ? b[k] : r[k]) << R.msb, c1 = g[k] << R.msb, c2 = (R.swap ? r[k] : b[k]) << R.msb;
        o.v[4 * k] = (DST)(R.lead ? one : c0); o.v[4 * k + 1] = (DST)(R.lead ? c0 : c1);
        o.v[4 * k + 2] = (DST)(R.lead ? c1 : c2); o.v[4 * k + 3] = (DST)(R.lead ? c2 : one);
      }
      *(LayoutVec<DST, 4 * P>*)(row + (size_t)x0 * 4 * sizeof(DST)) = o;
    } else if constexpr (KIND == 1) {
      constexpr int per = 4 / (int)sizeof(DST);
      uint32_t w[3] = {0, 0, 0};
      for (int k = 0; k < P; k++) {
        const int c[3] = {(R.swap ? b[k] : r[k]) << R.msb, g[k] << R.msb, (R.swap ? r[k] : b[k]) << R.msb};
        for (int i = 0; i < 3; i++) w[(3 * k + i) / per] |= (uint32_t)c[i] << (8 * (int)sizeof(DST) * ((3 * k + i) % per));
      }
      uint32_t* wp = (uint32_t*)(row + (size_t)x0 * 3 * sizeof(DST));
      wp[0] = w[0]; wp[1] = w[1]; wp[2] = w[2];
    } else {
      LayoutVec<DST, P> orr, og, ob;
      for (int k = 0; k < P; k++) { orr.v[k] = (DST)(r[k] << R.msb); og.v[k] = (DST)(g[k] << R.msb); ob.v[k] = (DST)(b[k] << R.msb); }
      *(LayoutVec<DST, P>*)(row + (size_t)x0 * sizeof(DST)) = orr;
      *(LayoutVec<DST, P>*)(row + R.plane + (size_t)x0 * sizeof(DST)) = og;
      *(LayoutVec<DST, P>*)(row + 2 * R.plane + (size_t)x0 * sizeof(DST)) = ob;
    }
  }
}

// Whether the rows of the RGB side take whole vectors: 16-byte aligned rows (and planes) for four samples per pixel and for planes, 4-byte aligned
// rows for three samples per pixel.
TK_DEV bool rgb_rows_aligned(const void* base, const RgbFormat& R) {
  return ((((uintptr_t)base) | R.pitch | R.plane) & (R.kind == 1 ? 3 : 15)) == 0;
}

// An RGB frame at `base` (SRC = uint8_t for depth 8, uint16_t otherwise) -> the engine's planes, input_bitdepth samples << up.  One work item per
// pair of luma rows with its chroma row; `lane`/`nlanes` stride along it in runs of RgbRun::P pixels, what is left of the row quad by quad.
template <typename SRC, typename PIX, int KIND>
TK_DEV void rgb_in_kind(const uint8_t* b, const RgbFormat& R, const Plane3<PIX>& dst, int width, int height, int up, int gid, int gsize, int lane, int nlanes) {
  constexpr int P = RgbRun<SRC, KIND, true>::P;
  const int nv = rgb_rows_aligned(b, R) ? width / P : 0;
  for (int it = gid; it < height / 2; it += gsize) {
    for (int i = lane; i < nv; i += nlanes) rgb_in_span<SRC, PIX, KIND, true>(b, R, dst, up, it, i * P);
    for (int x = nv * P + 2 * lane; x < width; x += 2 * nlanes) rgb_in_span<SRC, PIX, KIND, false>(b, R, dst, up, it, x);
  }
}
template <typename SRC, typename PIX>
TK_DEV void rgb_in_rows(const void* base, const RgbFormat& R, const Plane3<PIX>& dst, int width, int height, int up, int gid, int gsize, int lane, int nlanes) {
  const uint8_t* b = (const uint8_t*)base;
  if (R.kind == 0) rgb_in_kind<SRC, PIX, 0>(b, R, dst, width, height, up, gid, gsize, lane, nlanes);
  else if (R.kind == 1) rgb_in_kind<SRC, PIX, 1>(b, R, dst, width, height, up, gid, gsize, lane, nlanes);
  else rgb_in_kind<SRC, PIX, 2>(b, R, dst, width, height, up, gid, gsize, lane, nlanes);
}

// The engine's planes -> an RGB frame at `base` (DST = uint8_t for depth 8, uint16_t otherwise); shift = bitdepth - input_bitdepth.  Same work split.
template <typename PIX, typename DST, int KIND>
TK_DEV void rgb_out_kind(const Plane3<PIX>& src, uint8_t* b, const RgbFormat& R, int width, int height, int shift, int gid, int gsize, int lane, int nlanes) {
  constexpr int P = RgbRun<DST, KIND, true>::P;
  const int nv = rgb_rows_aligned(b, R) ? width / P : 0;
  for (int it = gid; it < height / 2; it += gsize) {
    for (int i = lane; i < nv; i += nlanes) rgb_out_span<PIX, DST, KIND, true>(src, b, R, shift, it, i * P);
    for (int x = nv * P + 2 * lane; x < width; x += 2 * nlanes) rgb_out_span<PIX, DST, KIND, false>(src, b, R, shift, it, x);
  }
}
template <typename PIX, typename DST>
TK_DEV void rgb_out_rows(const Plane3<PIX>& src, void* base, const RgbFormat& R, int width, int height, int shift, int gid, int gsize, int lane, int nlanes) {
  uint8_t* b = (uint8_t*)base;
  if (R.kind == 0) rgb_out_kind<PIX, DST, 0>(src, b, R, width, height, shift, gid, gsize, lane, nlanes);
  else if (R.kind == 1) rgb_out_kind<PIX, DST, 1>(src, b, R, width, height, shift, gid, gsize, lane, nlanes);
  else rgb_out_kind<PIX, DST, 2>(src, b, R, width, height, shift, gid, gsize, lane, nlanes);
}

}  // namespace tk
