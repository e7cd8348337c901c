// tk_tf.h - temporal noise filter of staged originals, motion-compensated (include/thor_hip.h: thor_hip_temporal_filter states the whole algorithm;
// tests/tf_model.py restates it in numpy).  Integers only.  Two steps per request:
//   search  per neighbour and 8x8 luma block the full-pel vector of [-8, 8]^2 with the least (SAD, rank), and the block weight wb from that SAD
//   blend   per sample the weighted mean of the current sample and its motion-compensated neighbours, luma and both chroma planes
// The block functions are TK_DEV: k_tf_search / k_tf_blend (hip_kernels.h) run them on LDS tiles with one lane per candidate and on the planes with one
// lane per four samples, the host twin tf_filter_frame with one lane.  The filter is not recursive: it reads originals and writes another frame.
#pragma once
#include "tk_common.h"

namespace tk {

constexpr int TF_BLK = 8;                                      // luma block; its chroma block is 4x4
constexpr int TF_RANGE = 8;                                    // vectors (dx, dy) in [-8, 8]^2
constexpr int TF_SPAN = 2 * TF_RANGE + 1;
constexpr int TF_CAND = TF_SPAN * TF_SPAN;                     // 289
constexpr int TF_TILE = 32;                                    // luma samples a workgroup owns per axis: 4 x 4 blocks
constexpr int TF_WIN = TF_TILE + 2 * TF_RANGE;                 // the neighbour's tile with its halo
constexpr int TF_MAX_REFS = 4;
constexpr int TF_MAX_STRENGTH = 16;
constexpr int TF_RANK_BITS = 9;                                // rank <= 289 < 2^9; SAD <= 64 * 4095 < 2^18: the key (SAD << 9 | rank) stays below 2^27
constexpr unsigned TF_NO_KEY = 0xffffffffu;

struct TfBlock {  // one block against one neighbour
  int8_t dx, dy;
  uint16_t wb;    // Q8, at most 192
};

template <typename PIX> struct TfJob {
  Plane3<PIX> cur, dst;            // rows start 16-byte aligned (staged frames do)
  Plane3<PIX> ref[TF_MAX_REFS];
  int dist[TF_MAX_REFS];           // 1 or 2
  int nrefs;                       // 0: dst becomes a copy of cur
  int width, height;               // multiples of 8
  int strength;                    // 1 .. 16
  int sh;                          // bitdepth - 8
  TfBlock* blk;                    // [neighbour][block, raster order]: (width / 8) * (height / 8) records per neighbour
};

TK_DEV int tf_rank(int dx, int dy) { return (dx | dy) == 0 ? 0 : 1 + (dy + TF_RANGE) * TF_SPAN + (dx + TF_RANGE); }
TK_DEV void tf_rank_vector(int rank, int& dx, int& dy) {
  dx = dy = 0;
  if (rank) { dy = (rank - 1) / TF_SPAN - TF_RANGE; dx = (rank - 1) % TF_SPAN - TF_RANGE; }
}

// SAD of the 8x8 block at b (rows start at addresses aligned to 8 samples) against the 8x8 samples at sample index ri of the array `ra` (4-byte aligned base,
// any index).  The device form is the motion search's packed one: v_sad_u8 on four 8-bit samples, v_sad_u16 on two 16-bit ones; the displaced row comes as
// aligned dwords, shifted into place with v_alignbyte (the dword after the row's last one is read: the window's array is padded for it).
template <typename PIX> TK_DEV unsigned tf_sad8x8(const PIX* b, int bs, const PIX* ra, int ri, int rs) {
  unsigned s = 0;
#if TK_HOST
  const PIX* r = ra + ri;
  for (int i = 0; i < TF_BLK; i++)
    for (int j = 0; j < TF_BLK; j++) s += (unsigned)iabs((int)b[i * bs + j] - (int)r[i * rs + j]);
#else
  constexpr int ND = 2 * (int)sizeof(PIX);   // dwords of a row of 8 samples
  TK_UNROLL
  for (int i = 0; i < TF_BLK; i++) {
    const uint32_t* bp = (const uint32_t*)(b + i * bs);
    const unsigned byte = (unsigned)(ri + i * rs) * (unsigned)sizeof(PIX);
    const uint32_t* rp = (const uint32_t*)ra + (byte >> 2);
    const unsigned off = byte & 3;
    uint32_t w[ND + 1];
    TK_UNROLL
    for (int k = 0; k <= ND; k++) w[k] = rp[k];
    TK_UNROLL
    for (int k = 0; k < ND; k++) {
      const uint32_t d = __builtin_amdgcn_alignbyte(w[k + 1], w[k], off);
      if constexpr (sizeof(PIX) == 1) s = __builtin_amdgcn_sad_u8(bp[k], d, s);
      else s = __builtin_amdgcn_sad_u16(bp[k], d, s);
    }
  }
#endif
  return s;
}

// Least key (SAD << 9 | rank) of the block at (x0, y0) of a pw x ph plane over this lane's share of the 289 vectors; sample ri of the array `ra` (4-byte aligned)
// is the neighbour's sample (x0, y0), rs samples per row.  A candidate whose block leaves the plane is skipped (no padding), the zero vector never is.  TF_NO_KEY: no candidate.
template <typename PIX> TK_DEV unsigned tf_block_search(const PIX* b, int bs, const PIX* ra, int ri, int rs, int x0, int y0, int pw, int ph, int lane, int nlanes) {
  unsigned best = TF_NO_KEY;
  for (int c = lane; c < TF_CAND; c += nlanes) {
    const int dy = c / TF_SPAN - TF_RANGE, dx = c % TF_SPAN - TF_RANGE;
    if (x0 + dx < 0 || x0 + dx + TF_BLK > pw || y0 + dy < 0 || y0 + dy + TF_BLK > ph) continue;
    const unsigned key = (tf_sad8x8(b, bs, ra, ri + dy * rs + dx, rs) << TF_RANK_BITS) | (unsigned)tf_rank(dx, dy);
    best = key < best ? key : best;
  }
  return best;
}

// The block's record from its least key: wb = B[dist] * max(0, Tb - m) / Tb with m = SAD >> sh, Tb = 128 * strength, B = 192 / 128 for dist 1 / 2.
// B * (Tb - m) <= 192 * 2048: 32 bits with room.
TK_DEV TfBlock tf_block_record(unsigned key, int sh, int strength, int dist) {
  TfBlock t;
  int dx, dy;
  tf_rank_vector((int)(key & ((1u << TF_RANK_BITS) - 1)), dx, dy);
  t.dx = (int8_t)dx; t.dy = (int8_t)dy;
  const int m = (int)((key >> TF_RANK_BITS) >> sh), Tb = 128 * strength;
  t.wb = (uint16_t)((dist == 1 ? 192 : 128) * (Tb - m > 0 ? Tb - m : 0) / Tb);
  return t;
}

// Four neighbouring samples (x .. x + 3, y) of plane `plane` (0: luma, 1: U, 2: V; chroma coordinates for 1 and 2), x a multiple of 4: they share one
// block, hence one vector and one wb per neighbour.  Per sample: w = wb * max(0, Ts - (|c - r| >> sh)), Ts = 4 * strength; out = (c * W0 + sum r * w +
// D / 2) / D with W0 = 256 * Ts and D = W0 + sum w.  W0 <= 2^14 and w <= 192 * 64 per neighbour, so D <= 2^16 and the numerator stays below 2^29.
template <typename PIX> TK_DEV void tf_blend_quad(const TfJob<PIX>& J, int plane, int x, int y) {
  struct alignas(4 * sizeof(PIX)) Quad { PIX v[4]; };
  const int lb = plane ? 2 : 3;                                   // log2 of the block size in this plane
  const int stride = plane ? J.cur.sc : J.cur.sy;
  const PIX* cp = (plane == 0 ? J.cur.y : plane == 1 ? J.cur.u : J.cur.v) + (size_t)y * stride + x;
  Quad c;
  __builtin_memcpy(&c, __builtin_assume_aligned(cp, sizeof(Quad)), sizeof(Quad));
  const unsigned Ts = 4u * (unsigned)J.strength, W0 = 256u * Ts;
  unsigned num[4], den[4];
  for (int j = 0; j < 4; j++) { num[j] = (unsigned)c.v[j] * W0; den[j] = W0; }
  const int nb = (J.width / TF_BLK) * (J.height / TF_BLK), bi = (y >> lb) * (J.width / TF_BLK) + (x >> lb);
  for (int k = 0; k < J.nrefs; k++) {
    const TfBlock t = J.blk[(size_t)k * nb + bi];
    if (!t.wb) continue;
    const int dx = plane ? t.dx >> 1 : t.dx, dy = plane ? t.dy >> 1 : t.dy;   // arithmetic shifts
    const int rstride = plane ? J.ref[k].sc : J.ref[k].sy;
    const PIX* rp = (plane == 0 ? J.ref[k].y : plane == 1 ? J.ref[k].u : J.ref[k].v) + (ptrdiff_t)(y + dy) * rstride + (x + dx);
    for (int j = 0; j < 4; j++) {
      const unsigned r = rp[j];
      const unsigned d = (unsigned)iabs((int)c.v[j] - (int)r) >> J.sh;
      const unsigned w = (unsigned)t.wb * (Ts > d ? Ts - d : 0u);
      num[j] += r * w;
      den[j] += w;
    }
  }
  Quad o;
  for (int j = 0; j < 4; j++) o.v[j] = (PIX)((num[j] + den[j] / 2) / den[j]);
  PIX* dp = (plane == 0 ? J.dst.y : plane == 1 ? J.dst.u : J.dst.v) + (size_t)y * (plane ? J.dst.sc : J.dst.sy) + x;
  __builtin_memcpy(__builtin_assume_aligned(dp, sizeof(Quad)), &o, sizeof(Quad));
}

// A request's arguments (thor_hip_tf_request) without a device: 0 when every field is in range.  Slots are checked by the caller.
static inline bool tf_strength_ok(int strength) { return strength >= 1 && strength <= TF_MAX_STRENGTH; }
struct TfRequest {
  int stream, dst_slot, slot, nrefs;
  int ref_slot[TF_MAX_REFS], ref_dist[TF_MAX_REFS];
};
// All requests of one call: true when each is in range, every source is staged (is_staged(stream, slot)), no destination is a source of any request of
// the call and no two requests share a destination.  Touches nothing.
template <typename F> static inline bool tf_requests_ok(const TfRequest* req, int n, int num_streams, F is_staged) {
  if (!req || n < 1) return false;
  for (int i = 0; i < n; i++) {
    const TfRequest& r = req[i];
    if (r.stream < 0 || r.stream >= num_streams || r.dst_slot < 0 || r.nrefs < 0 || r.nrefs > TF_MAX_REFS) return false;
    if (!is_staged(r.stream, r.slot)) return false;
    for (int k = 0; k < r.nrefs; k++)
      if ((r.ref_dist[k] != 1 && r.ref_dist[k] != 2) || !is_staged(r.stream, r.ref_slot[k])) return false;
  }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      if (req[i].stream != req[j].stream) continue;
      if (i != j && req[i].dst_slot == req[j].dst_slot) return false;
      if (req[i].dst_slot == req[j].slot) return false;
      for (int k = 0; k < req[j].nrefs; k++)
        if (req[i].dst_slot == req[j].ref_slot[k]) return false;
    }
  return true;
}

#if TK_HOST
// One request with one lane: what k_tf_search and k_tf_blend compute tile by tile.
template <typename PIX> static inline void tf_filter_frame(const TfJob<PIX>& J) {
  const int bw = J.width / TF_BLK, bh = J.height / TF_BLK;
  for (int k = 0; k < J.nrefs; k++)
    for (int by = 0; by < bh; by++)
      for (int bx = 0; bx < bw; bx++) {
        const int x0 = bx * TF_BLK, y0 = by * TF_BLK;
        const unsigned key = tf_block_search(J.cur.y + (size_t)y0 * J.cur.sy + x0, J.cur.sy, J.ref[k].y, y0 * J.ref[k].sy + x0, J.ref[k].sy, x0, y0, J.width, J.height,
                                             0, 1);
        J.blk[(size_t)k * bw * bh + by * bw + bx] = tf_block_record(key, J.sh, J.strength, J.dist[k]);
      }
  for (int y = 0; y < J.height; y++)
    for (int x = 0; x < J.width; x += 4) tf_blend_quad(J, 0, x, y);
  for (int plane = 1; plane < 3; plane++)
    for (int y = 0; y < J.height / 2; y++)
      for (int x = 0; x < J.width / 2; x += 4) tf_blend_quad(J, plane, x, y);
}
#endif

}  // namespace tk
