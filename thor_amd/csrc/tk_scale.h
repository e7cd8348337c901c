// tk_scale.h - frames of another size at the boundary: separable polyphase resampling into the staging slot.
// A source frame (4:2:0, input_bitdepth samples, src_w x src_h, in any PixLayout) becomes the engine's planes at width x height: each plane is
// filtered horizontally, then vertically, with integer tap tables built once per geometry on the host (resolve_scale; 64-bit integers, no floating
// point), and the result is widened like any staged frame.  include/thor_hip.h (thor_hip_scale) holds the arithmetic to the bit; the functions
// below are that text.  The sample arithmetic is TK_DEV: k_scale_in (hip_kernels.h) and the host build (scale_in_host) run the same pieces.
#pragma once
#include <vector>
#include "tk_filters.h"

namespace tk {

enum { SCALE_BILINEAR = 0, SCALE_BICUBIC = 1 };
enum {
  SCALE_COEF_BITS = 14,   // every tap set sums to 1 << 14
  SCALE_GUARD = 2,        // bits the horizontal intermediate keeps below the sample
  SCALE_MAX_TAPS = 33,    // ratio 8, bicubic
  SCALE_MAX_ABS = 26214,  // sum |c| of a tap set: the intermediate fits 16 bits and the vertical sum 32 at 12-bit samples
  SCALE_MIN = 16, SCALE_MAX = 8192, SCALE_MAX_RATIO = 8,
  // a workgroup's tile of destination samples, and what it needs of LDS at the worst ratio (8): the source samples of one row that 64 destination
  // samples reach, the horizontally filtered rows that 32 destination rows reach
  SCALE_TW = 64, SCALE_TH = 32,
  SCALE_ROWCAP = (SCALE_TW - 1) * SCALE_MAX_RATIO + SCALE_MAX_TAPS + 7,   // 544
  SCALE_VROWS = (SCALE_TH - 1) * SCALE_MAX_RATIO + SCALE_MAX_TAPS + 7,    // 288
  SCALE_WAVES = 4
};

// floor(a / b), b > 0
static inline long long scale_floordiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// The taps of destination index i on one axis (S source samples -> T): first source index (may be negative: the edge replicates) and the
// coefficients, which sum to 1 << 14.  Returns their count; 0: refused (lengths, ratio, filter, index, or more taps than `cap`).
static inline int scale_taps(int S, int T, int filter, int cosited, int i, int* first, int16_t* coef, int cap) {
  if (S < 1 || T < 1 || S > SCALE_MAX || T > SCALE_MAX || S > SCALE_MAX_RATIO * T || T > SCALE_MAX_RATIO * S) return 0;
  if (filter < 0 || filter > 1 || cosited < 0 || cosited > 1 || i < 0 || i >= T || !first || !coef) return 0;
  const long long D = 2ll * (S > T ? S : T), A = filter == SCALE_BICUBIC ? 2 : 1, lim = A * D;
  auto num = [&](long long k) { return cosited ? 2 * ((long long)i * S - k * T) : (2ll * i + 1) * S - (2 * k + 1) * T; };
  long long k = scale_floordiv((cosited ? 2ll * i * S : (2ll * i + 1) * S) - lim, 2ll * T) - 2;
  while (num(k) >= lim) k++;   // n(k) falls by 2T per step
  long long W[SCALE_MAX_TAPS + 1], sum = 0;
  int n = 0, best = 0;
  for (; num(k + n) > -lim; n++) {
    if (n >= SCALE_MAX_TAPS) return 0;
    const long long nn = num(k + n), a = nn < 0 ? -nn : nn;
    W[n] = filter == SCALE_BILINEAR ? D - a : a < D ? 3 * a * a * a - 5 * a * a * D + 2 * D * D * D : -a * a * a + 5 * a * a * D - 8 * a * D * D + 4 * D * D * D;
    sum += W[n];
    if (W[n] > W[best]) best = n;
  }
  if (n == 0 || n > cap || sum <= 0) return 0;
  long long total = 0;
  long long c[SCALE_MAX_TAPS];
  for (int j = 0; j < n; j++) { c[j] = scale_floordiv(2 * W[j] * (1 << SCALE_COEF_BITS) + sum, 2 * sum); total += c[j]; }
  c[best] += (1 << SCALE_COEF_BITS) - total;
  for (int j = 0; j < n; j++) {
    if (c[j] < -32768 || c[j] > 32767) return 0;
    coef[j] = (int16_t)c[j];
  }
  *first = (int)k;
  return n;
}

// One axis of a plan as the filters read it: `nt` coefficients per destination index (tap sets shorter than the longest are padded with zeros).
struct ScaleAxis {
  const int* first;
  const int16_t* coef;
  int nt, S, T;
};
struct ScaleTables { ScaleAxis a[4]; };   // luma horizontal, luma vertical, chroma horizontal, chroma vertical

// The tables of one axis on the host.
struct ScaleAxisTable {
  std::vector<int> first;
  std::vector<int16_t> coef;
  int nt = 0, S = 0, T = 0;
  int span = 0;   // the most source samples one tile reaches
  // false: a tap set is refused, sums above SCALE_MAX_ABS in magnitude, or a tile of `tile` destination samples reaches more than `cap` source samples
  bool build(int S_, int T_, int filter, int cosited, int tile, int cap) {
    S = S_; T = T_; nt = 0; span = 0;
    first.assign(T, 0);
    std::vector<int16_t> all((size_t)T * SCALE_MAX_TAPS, 0);
    std::vector<int> cnt(T);
    for (int i = 0; i < T; i++) {
      cnt[i] = scale_taps(S, T, filter, cosited, i, &first[i], &all[(size_t)i * SCALE_MAX_TAPS], SCALE_MAX_TAPS);
      if (!cnt[i]) return false;
      long long mag = 0;
      for (int j = 0; j < cnt[i]; j++) mag += all[(size_t)i * SCALE_MAX_TAPS + j] < 0 ? -all[(size_t)i * SCALE_MAX_TAPS + j] : all[(size_t)i * SCALE_MAX_TAPS + j];
      if (mag > SCALE_MAX_ABS) return false;
      if (i && first[i] < first[i - 1]) return false;
      if (cnt[i] > nt) nt = cnt[i];
    }
    coef.assign((size_t)T * nt, 0);
    for (int i = 0; i < T; i++)
      for (int j = 0; j < cnt[i]; j++) coef[(size_t)i * nt + j] = all[(size_t)i * SCALE_MAX_TAPS + j];
    for (int t0 = 0; t0 < T; t0 += tile) {
      const int t1 = (t0 + tile < T ? t0 + tile : T) - 1;
      if (first[t1] + nt - first[t0] > span) span = first[t1] + nt - first[t0];
    }
    return span <= cap;
  }
};

// A scaled staging resolved against the engine's picture: the source layout at the source size and the four tap tables.
struct ScalePlan {
  int src_w = 0, src_h = 0, width = 0, height = 0, filter = -1, site = -1;
  PixLayout L;               // of the source frame
  ScaleAxisTable t[4];       // luma horizontal, luma vertical, chroma horizontal, chroma vertical
  bool same_tables(int sw, int sh, int w, int h, int f, int s) const { return sw == src_w && sh == src_h && w == width && h == height && f == filter && s == site; }
  // the tables as one block of memory: four `first` arrays, then four coefficient arrays (each padded to 4 bytes); `at` = where that block lies
  size_t blob_bytes() const {
    size_t n = 0;
    for (int k = 0; k < 4; k++) n += t[k].first.size() * sizeof(int) + ((t[k].coef.size() + 1) & ~(size_t)1) * sizeof(int16_t);
    return n;
  }
  ScaleTables pack(uint8_t* host, const uint8_t* at) const {
    ScaleTables d;
    size_t off = 0;
    for (int k = 0; k < 4; k++) {
      memcpy(host + off, t[k].first.data(), t[k].first.size() * sizeof(int));
      d.a[k].first = (const int*)(at + off);
      off += t[k].first.size() * sizeof(int);
    }
    for (int k = 0; k < 4; k++) {
      memcpy(host + off, t[k].coef.data(), t[k].coef.size() * sizeof(int16_t));
      d.a[k].coef = (const int16_t*)(at + off);
      d.a[k].nt = t[k].nt; d.a[k].S = t[k].S; d.a[k].T = t[k].T;
      off += ((t[k].coef.size() + 1) & ~(size_t)1) * sizeof(int16_t);
    }
    return d;
  }
  ScaleTables host_tables() const {
    ScaleTables d;
    for (int k = 0; k < 4; k++) d.a[k] = ScaleAxis{t[k].first.data(), t[k].coef.data(), t[k].nt, t[k].S, t[k].T};
    return d;
  }
};

// The arguments alone: sizes, ratios, filter, site, and the source layout at the source size.  false: refused.  Builds no table.
static inline bool resolve_scale_args(int src_w, int src_h, int filter, int site, int chroma, int msb_aligned, long long pitch_y, long long pitch_c, size_t off_u,
                                      size_t off_v, int width, int height, int input_bitdepth, PixLayout& L) {
  if (src_w < SCALE_MIN || src_h < SCALE_MIN || src_w > SCALE_MAX || src_h > SCALE_MAX || (src_w & 1) || (src_h & 1)) return false;
  if (width < 16 || height < 16 || width % 8 || height % 8 || width > SCALE_MAX || height > SCALE_MAX) return false;
  if (src_w > SCALE_MAX_RATIO * width || width > SCALE_MAX_RATIO * src_w || src_h > SCALE_MAX_RATIO * height || height > SCALE_MAX_RATIO * src_h) return false;
  if (filter < 0 || filter > 1 || site < 0 || site > 1) return false;
  if (input_bitdepth != 8 && input_bitdepth != 10 && input_bitdepth != 12) return false;
  return resolve_layout(chroma, msb_aligned, pitch_y, pitch_c, off_u, off_v, src_w, src_h, input_bitdepth, L);
}

// The whole plan.  `P` may hold the tables of an earlier call: they are rebuilt only when the geometry, the filter or the site changed.
static inline bool resolve_scale(int src_w, int src_h, int filter, int site, int chroma, int msb_aligned, long long pitch_y, long long pitch_c, size_t off_u,
                                 size_t off_v, int width, int height, int input_bitdepth, ScalePlan& P, bool* rebuilt = nullptr) {
  PixLayout L;
  if (rebuilt) *rebuilt = false;
  if (!resolve_scale_args(src_w, src_h, filter, site, chroma, msb_aligned, pitch_y, pitch_c, off_u, off_v, width, height, input_bitdepth, L)) return false;
  if (!P.same_tables(src_w, src_h, width, height, filter, site)) {
    P.filter = -1;   // not valid until all four are built
    if (!P.t[0].build(src_w, width, filter, 0, SCALE_TW, SCALE_ROWCAP) || !P.t[1].build(src_h, height, filter, 0, SCALE_TH, SCALE_VROWS) ||
        !P.t[2].build(src_w / 2, width / 2, filter, site, SCALE_TW, SCALE_ROWCAP) || !P.t[3].build(src_h / 2, height / 2, filter, 0, SCALE_TH, SCALE_VROWS))
      return false;
    P.src_w = src_w; P.src_h = src_h; P.width = width; P.height = height; P.filter = filter; P.site = site;
    if (rebuilt) *rebuilt = true;
  }
  P.L = L;
  return true;
}

// ---- what a workgroup does for one tile (TK_DEV: the kernel and the host build share it) ---------------------------------------------------------

// One plane of the source as its rows are read: every `step`-th sample of a row of `len` samples, starting at `phase` (semi-planar chroma: 2, 0 / 1).
struct ScaleSrc {
  const uint8_t* base;   // first row
  size_t pitch;
  int step, phase, len;  // len: samples of the row that belong to the picture, all planes of it counted
  bool vec;              // rows on 16-byte boundaries
};
// A tile: destination samples [x0, x0 + tw) x [y0, y0 + th) of plane `plane`; the source samples [klo, khi] of the rows [r0, r0 + nrows) feed it.
struct ScaleTile {
  int plane, x0, y0, tw, th, klo, khi, r0, nrows;
};

TK_DEV int scale_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

TK_HD int scale_tiles(int w, int h) { return ((w + SCALE_TW - 1) / SCALE_TW) * ((h + SCALE_TH - 1) / SCALE_TH); }
TK_HD int scale_items(int width, int height) { return scale_tiles(width, height) + 2 * scale_tiles(width / 2, height / 2); }

// Tile number `item` of the frame: the luma tiles first, then those of U, then those of V.
TK_DEV ScaleTile scale_tile(int item, int width, int height, const ScaleAxis& H, const ScaleAxis& V) {
  ScaleTile t;
  const int nl = scale_tiles(width, height), nc = scale_tiles(width / 2, height / 2);
  t.plane = item < nl ? 0 : 1 + (item - nl) / nc;
  const int j = item < nl ? item : (item - nl) % nc;
  const int across = (H.T + SCALE_TW - 1) / SCALE_TW;
  t.x0 = (j % across) * SCALE_TW; t.y0 = (j / across) * SCALE_TH;
  t.tw = H.T - t.x0 < SCALE_TW ? H.T - t.x0 : SCALE_TW;
  t.th = V.T - t.y0 < SCALE_TH ? V.T - t.y0 : SCALE_TH;
  t.klo = scale_clampi(H.first[t.x0], 0, H.S - 1);
  t.khi = scale_clampi(H.first[t.x0 + t.tw - 1] + H.nt - 1, 0, H.S - 1);
  t.r0 = scale_clampi(V.first[t.y0], 0, V.S - 1);
  t.nrows = scale_clampi(V.first[t.y0 + t.th - 1] + V.nt - 1, 0, V.S - 1) - t.r0 + 1;
  return t;
}

TK_DEV ScaleSrc scale_src(const void* frame, const PixLayout& L, int plane, int src_w) {
  ScaleSrc s;
  const uint8_t* b = (const uint8_t*)frame;
  if (plane == 0) { s.base = b; s.pitch = L.pitch_y; s.step = 1; s.phase = 0; s.len = src_w; s.vec = layout_rows_aligned(b, 0, L.pitch_y); }
  else if (L.chroma == 0) {
    const size_t off = plane == 1 ? L.off_u : L.off_v;
    s.base = b + off; s.pitch = L.pitch_c; s.step = 1; s.phase = 0; s.len = src_w / 2; s.vec = layout_rows_aligned(b, off, L.pitch_c);
  } else {
    s.base = b + L.off_u; s.pitch = L.pitch_c; s.step = 2; s.phase = (plane == 1) == (L.chroma == 1) ? 0 : 1; s.len = src_w;
    s.vec = layout_rows_aligned(b, L.off_u, L.pitch_c);
  }
  return s;
}

// Samples klo .. khi of the plane's row `r` -> buf[0 .. khi - klo], x = s >> msb.  Whole 16-byte vectors where the rows are aligned and the vector
// lies inside the picture's row; what is left of the range sample by sample.  Nothing outside [klo, khi] of the row is stored, nothing outside the
// row is read.
template <typename SRC> TK_DEV void scale_load_row(const ScaleSrc& s, int msb, int r, int klo, int khi, int16_t* buf, int lane, int nlanes) {
  constexpr int N = 16 / (int)sizeof(SRC);
  const SRC* row = (const SRC*)(s.base + (size_t)r * s.pitch);
  const int e0 = klo * s.step + s.phase, e1 = khi * s.step + s.phase;   // elements of the row
  int v0 = 0, v1 = -1;                                                    // whole vectors
  if (s.vec) { v0 = e0 / N; v1 = e1 / N < s.len / N - 1 ? e1 / N : s.len / N - 1; }
  for (int vi = v0 + lane; vi <= v1; vi += nlanes) {
    const LayoutVec<SRC, N> a = ((const LayoutVec<SRC, N>*)row)[vi];
    TK_UNROLL
    for (int j = 0; j < N; j++) {
      const int e = vi * N + j;
      if (s.step == 2 && (j & 1) != s.phase) continue;
      const int k = s.step == 2 ? e >> 1 : e;
      if (k >= klo && k <= khi) buf[k - klo] = (int16_t)(((int)a.v[j]) >> msb);
    }
  }
  int ks = klo;                                                           // first sample the vectors did not bring
  if (v1 >= v0) { const int e = (v1 + 1) * N; ks = s.step == 2 ? (e + 1 - s.phase) >> 1 : e; if (ks < klo) ks = klo; }
  for (int k = ks + lane; k <= khi; k += nlanes) buf[k - klo] = (int16_t)(((int)row[k * s.step + s.phase]) >> msb);
}

// The horizontal pass of one source row for the tile's columns: out[c] = (sum coef * x + half) >> (14 - g).  `coef`: the tile's coefficients as
// [tap][SCALE_TW] (scale_stage_coef).
TK_DEV void scale_hfilter_row(const ScaleAxis& H, const ScaleTile& t, const int16_t* coef, const int16_t* buf, int16_t* out, int lane, int nlanes) {
  for (int c = lane; c < t.tw; c += nlanes) {
    const int f = H.first[t.x0 + c];
    int acc = 1 << (SCALE_COEF_BITS - 1 - SCALE_GUARD);
    for (int k = 0; k < H.nt; k++) acc += (int)coef[k * SCALE_TW + c] * (int)buf[scale_clampi(f + k, 0, H.S - 1) - t.klo];
    out[c] = (int16_t)(acc >> (SCALE_COEF_BITS - SCALE_GUARD));
  }
}
TK_DEV void scale_stage_coef(const ScaleAxis& H, const ScaleTile& t, int16_t* coef, int tid, int nthreads) {
  for (int i = tid; i < H.nt * t.tw; i += nthreads) { const int c = i / H.nt, k = i % H.nt; coef[k * SCALE_TW + c] = H.coef[(size_t)(t.x0 + c) * H.nt + k]; }
}

// The vertical pass over the tile: inter[row - r0][SCALE_TW] -> plane samples at the engine's depth.
template <typename PIX>
TK_DEV void scale_vfilter(const ScaleAxis& V, const ScaleTile& t, const int16_t* inter, PIX* plane, int stride, int maxv, int up, int tid, int nthreads) {
  for (int i = tid; i < t.th * SCALE_TW; i += nthreads) {
    const int y = i / SCALE_TW, c = i % SCALE_TW;
    if (c >= t.tw) continue;
    const int f = V.first[t.y0 + y];
    const int16_t* cf = V.coef + (size_t)(t.y0 + y) * V.nt;
    int acc = 1 << (SCALE_COEF_BITS - 1 + SCALE_GUARD);
    for (int k = 0; k < V.nt; k++) acc += (int)cf[k] * (int)inter[(scale_clampi(f + k, 0, V.S - 1) - t.r0) * SCALE_TW + c];
    plane[(size_t)(t.y0 + y) * stride + t.x0 + c] = (PIX)(scale_clampi(acc >> (SCALE_COEF_BITS + SCALE_GUARD), 0, maxv) << up);
  }
}

template <typename PIX> TK_DEV PIX* scale_plane(const Plane3<PIX>& p, int plane) { return plane == 0 ? p.y : plane == 1 ? p.u : p.v; }

#if TK_HOST
// The host build: every tile in turn, its phases in the kernel's order with `nwaves` x `nlanes` lanes taken one after the other.  The Engine runs it
// with one lane; tests/hostsim/unit_scale.cpp also as 4 x 64.
template <typename SRC, typename PIX>
static inline void scale_in_host(const void* frame, const PixLayout& L, const ScaleTables& tab, const Plane3<PIX>& dst, int src_w, int width, int height,
                                 int input_bitdepth, int up, int nwaves, int nlanes) {
  std::vector<int16_t> rowbuf((size_t)nwaves * SCALE_ROWCAP), coef((size_t)SCALE_MAX_TAPS * SCALE_TW), inter((size_t)SCALE_VROWS * SCALE_TW);
  const int nthreads = nwaves * nlanes, maxv = (1 << input_bitdepth) - 1;
  for (int item = 0; item < scale_items(width, height); item++) {
    const bool luma = item < scale_tiles(width, height);
    const ScaleAxis& H = tab.a[luma ? 0 : 2];
    const ScaleAxis& V = tab.a[luma ? 1 : 3];
    const ScaleTile t = scale_tile(item, width, height, H, V);
    const ScaleSrc s = scale_src(frame, L, t.plane, src_w);
    for (int tid = 0; tid < nthreads; tid++) scale_stage_coef(H, t, coef.data(), tid, nthreads);
    for (int r = 0; r < t.nrows; r += nwaves) {
      for (int w = 0; w < nwaves && r + w < t.nrows; w++)
        for (int l = 0; l < nlanes; l++) scale_load_row<SRC>(s, L.msb, t.r0 + r + w, t.klo, t.khi, &rowbuf[(size_t)w * SCALE_ROWCAP], l, nlanes);
      for (int w = 0; w < nwaves && r + w < t.nrows; w++)
        for (int l = 0; l < nlanes; l++) scale_hfilter_row(H, t, coef.data(), &rowbuf[(size_t)w * SCALE_ROWCAP], &inter[(size_t)(r + w) * SCALE_TW], l, nlanes);
    }
    for (int tid = 0; tid < nthreads; tid++)
      scale_vfilter<PIX>(V, t, inter.data(), scale_plane(dst, t.plane), t.plane ? dst.sc : dst.sy, maxv, up, tid, nthreads);
  }
}
#endif

}  // namespace tk
