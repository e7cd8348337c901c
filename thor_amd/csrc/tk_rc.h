// tk_rc.h - rate control: a base QP per frame and stream from a frame analysis on the device (include/thor_hip.h: thor_hip_rate_control
// states the whole algorithm).  Two parts:
//   analysis    the half-size luma of the staged original, cut into 8x8 blocks: SAD against the block's rounded mean (intra cost) and the least SAD against
//               the previous half-size plane over the integer vectors of [-8, 8]^2 (inter cost).  The block functions are TK_DEV: k_rc_cost (hip_kernels.h)
//               runs them on LDS tiles with one lane per sample / per candidate, the host simulation on the planes with one lane (rc_cost_frame).
//   controller  host code, 64-bit integers only: virtual buffer, one bits-per-cost factor per frame class, the lowest base QP whose predicted bits fit.
// This is the project's own rate control, not the reference's (enc/rc.c changes the QP after every superblock in raster order, which the anti-diagonal
// wavefront of the superblock kernel cannot follow): every frame is coded at ONE QP and stays exactly what the block path produces at that QP.
#pragma once
#include "tk_common.h"
#if TK_HOST
#include <vector>
#endif

namespace tk {

// ---- analysis ------------------------------------------------------------------------------------------------------------------------------
constexpr int RC_BLK = 8;                                      // block of the half-size plane (4 wide / high at the right / bottom edge)
constexpr int RC_RANGE = 8;                                    // vectors (dx, dy) in [-8, 8]^2
constexpr int RC_SPAN = 2 * RC_RANGE + 1;
constexpr int RC_CAND = RC_SPAN * RC_SPAN;                     // 289
constexpr int RC_TILE = 32;                                    // half-size samples a workgroup owns per axis: 4 x 4 blocks
constexpr int RC_WIN = RC_TILE + 2 * RC_RANGE;                 // the previous plane's tile with its halo

template <typename PIX> struct RcJob {
  const PIX* y;             // luma of the staged original, at the engine's depth
  int sy;
  int hw, hh;               // size of the half-size plane (width / 2, height / 2: multiples of 4)
  PIX* cur;                 // half-size plane written by this analysis, hw samples per row
  const PIX* prev;          // the plane the previous analysis of the stream wrote; nullptr: none (inter cost = intra cost)
  unsigned long long* out;  // sum_intra, sum_best, n_intra: added to (cleared by the caller)
  // the variant that takes the previous frame as a full-size ORIGINAL (k_rc_cost<PIX, true>, thor_hip_scene_cost): halved while it is loaded; `cur` and `prev`
  // are not used then, and nothing is stored but the sums
  const PIX* prev_y = nullptr;   // luma of the previous original, 16-byte aligned like y; nullptr: none
  int prev_sy = 0;               // a multiple of 8 samples
};

// sample (x, r) of the half-size plane: (a + b + c + d + 2) >> 2 over the 2x2 quad
template <typename PIX> TK_DEV int rc_half_sample(const PIX* y, int sy, int x, int r) {
  const PIX* p = y + (size_t)(2 * r) * sy + 2 * x;
  return ((int)p[0] + (int)p[1] + (int)p[sy] + (int)p[sy + 1] + 2) >> 2;
}
// Four neighbouring samples (x .. x + 3, r) of the half-size plane at once, x a multiple of 4: two loads of 8 full-size samples (8 or 16 bytes each; the
// rows of a staged frame start 16-byte aligned and 2 * x is a multiple of 8), the same rounding as rc_half_sample.
template <typename PIX> TK_DEV void rc_half_quad(const PIX* y, int sy, int x, int r, PIX out[4]) {
  struct alignas(8 * sizeof(PIX)) Row { PIX v[8]; };
  const PIX* p = y + (size_t)(2 * r) * sy + 2 * x;
  Row a, b;
  __builtin_memcpy(&a, __builtin_assume_aligned(p, sizeof(Row)), sizeof(Row));
  __builtin_memcpy(&b, __builtin_assume_aligned(p + sy, sizeof(Row)), sizeof(Row));
  for (int k = 0; k < 4; k++) out[k] = (PIX)(((int)a.v[2 * k] + (int)a.v[2 * k + 1] + (int)b.v[2 * k] + (int)b.v[2 * k + 1] + 2) >> 2);
}
// The three block functions take a bw x bh block (bw, bh: 4 or 8) at b, bs samples per row, and return this lane's share: the caller adds the
// lanes' sums (rc_block_sum, rc_block_dev) or takes their minimum (rc_block_inter).  32-bit: 64 samples of 4095 do not fit 16 bits.
template <typename PIX> TK_DEV unsigned rc_block_sum(const PIX* b, int bs, int bw, int bh, int lane, int nlanes) {
  const int lw = bw == 8 ? 3 : 2;
  unsigned s = 0;
  for (int i = lane; i < bw * bh; i += nlanes) s += b[(i >> lw) * bs + (i & (bw - 1))];
  return s;
}
template <typename PIX> TK_DEV unsigned rc_block_dev(const PIX* b, int bs, int bw, int bh, int mean, int lane, int nlanes) {
  const int lw = bw == 8 ? 3 : 2;
  unsigned s = 0;
  for (int i = lane; i < bw * bh; i += nlanes) s += (unsigned)iabs((int)b[(i >> lw) * bs + (i & (bw - 1))] - mean);
  return s;
}
// Least SAD of the block at (x0, y0) of a pw x ph plane against the previous plane displaced by (dx, dy); `ref` points at the previous plane's sample
// (x0, y0), rs samples per row.  One candidate per lane and round; a candidate whose block leaves the plane is skipped (no padding), the zero vector
// never is.  0xffffffff when the lane had no candidate.
template <typename PIX> TK_DEV unsigned rc_block_inter(const PIX* b, int bs, const PIX* ref, int rs, int bw, int bh, int x0, int y0, int pw, int ph, int lane,
                                                       int nlanes) {
  unsigned best = 0xffffffffu;
  for (int c = lane; c < RC_CAND; c += nlanes) {
    const int dy = c / RC_SPAN - RC_RANGE, dx = c % RC_SPAN - RC_RANGE;
    if (x0 + dx < 0 || x0 + dx + bw > pw || y0 + dy < 0 || y0 + dy + bh > ph) continue;
    const PIX* r = ref + dy * rs + dx;
    unsigned s = 0;
    for (int i = 0; i < bh; i++)
      for (int j = 0; j < bw; j++) s += (unsigned)iabs((int)b[i * bs + j] - (int)r[i * rs + j]);
    best = s < best ? s : best;
  }
  return best;
}
// One block's share of the three sums, from its intra cost and its inter cost.
TK_DEV void rc_block_add(unsigned intra, unsigned inter, unsigned long long acc[3]) {
  acc[0] += intra;
  acc[1] += intra < inter ? intra : inter;
  acc[2] += intra < inter ? 1u : 0u;
}

#if TK_HOST
// The analysis of one frame with one lane: what k_rc_cost computes tile by tile.
// prev_orig (k_rc_cost<PIX, true>): the previous frame is J.prev_y, halved here four samples at a time as the kernel does; no plane is stored.
template <typename PIX> static inline void rc_cost_frame(const RcJob<PIX>& J0, bool prev_orig = false) {
  RcJob<PIX> J = J0;
  std::vector<PIX> hcur, hprev;
  if (prev_orig) {
    hcur.resize((size_t)J.hw * J.hh);
    J.cur = hcur.data(); J.prev = nullptr;
    if (J.prev_y) {
      hprev.resize((size_t)J.hw * J.hh);
      for (int r = 0; r < J.hh; r++)
        for (int x = 0; x < J.hw; x += 4) rc_half_quad(J.prev_y, J.prev_sy, x, r, hprev.data() + (size_t)r * J.hw + x);
      J.prev = hprev.data();
    }
  }
  for (int r = 0; r < J.hh; r++)
    for (int x = 0; x < J.hw; x++) J.cur[(size_t)r * J.hw + x] = (PIX)rc_half_sample(J.y, J.sy, x, r);
  unsigned long long acc[3] = {0, 0, 0};
  for (int y0 = 0; y0 < J.hh; y0 += RC_BLK)
    for (int x0 = 0; x0 < J.hw; x0 += RC_BLK) {
      const int bw = J.hw - x0 < RC_BLK ? J.hw - x0 : RC_BLK, bh = J.hh - y0 < RC_BLK ? J.hh - y0 : RC_BLK, n = bw * bh;
      const PIX* b = J.cur + (size_t)y0 * J.hw + x0;
      const int mean = (int)((rc_block_sum(b, J.hw, bw, bh, 0, 1) + (unsigned)(n / 2)) / (unsigned)n);
      const unsigned intra = rc_block_dev(b, J.hw, bw, bh, mean, 0, 1);
      const unsigned inter = J.prev ? rc_block_inter(b, J.hw, J.prev + (size_t)y0 * J.hw + x0, J.hw, bw, bh, x0, y0, J.hw, J.hh, 0, 1) : intra;
      rc_block_add(intra, inter, acc);
    }
  for (int k = 0; k < 3; k++) J.out[k] += acc[k];
}
#endif

// ---- controller (host) -----------------------------------------------------------------------------------------------------------------------
// 2^((qp - 4) / 6) in Q16, qp 0..51
static const long long kRcStepQ16[52] = {41285, 46341, 52016, 58386, 65536, 73562, 82570, 92682, 104032, 116772, 131072, 147123, 165140,
                                         185364, 208064, 233544, 262144, 294247, 330281, 370728, 416128, 467088, 524288, 588493, 660561, 741455,
                                         832255, 934175, 1048576, 1176987, 1321123, 1482910, 1664511, 1868350, 2097152, 2353974, 2642246, 2965821,
                                         3329021, 3736700, 4194304, 4707947, 5284492, 5931642, 6658043, 7473400, 8388608, 9415894, 10568984,
                                         11863283, 13316085, 14946800};
// Frame classes: I, P, B of level 0, 1, 2, 3 and deeper.
constexpr int RC_CLASSES = 6;
static inline int rc_class(int frame_type /* 0 I, 1 P, 2 B */, int b_level) { return frame_type == 0 ? 0 : frame_type == 1 ? 1 : 2 + (b_level < 3 ? b_level : 3); }
// Bits per unit of cost / step (Q16) a class starts with, fitted on host-simulation encodes of synthetic clips at qp 22 / 32 / 42.
static const long long kRcInitFactorQ16[RC_CLASSES] = {296000, 217000, 216000, 188000, 174000, 174000};
// Bounds that keep every product below 2^63: a factor is at most 2^26 (200 times the fitted ones: only a flat frame, whose cost is next to nothing, observes
// more) and a cost enters the controller as at most 2^36 (an 8192 x 8192 frame of 12-bit samples sums to under 2^36), so factor * cost <= 2^62; bits and T are
// ints, so bits * step < 2^31 * 2^24 and T * a[c] < 2^62.
constexpr long long kRcFactorMax = 1ll << 26;
constexpr long long kRcCostMax = 1ll << 36;
static inline long long rc_cost(long long cost) { return cost < 1 ? 1 : cost > kRcCostMax ? kRcCostMax : cost; }
constexpr int kRcIntraBudget = 4;    // a later I frame may take this many frame budgets; the buffer absorbs the rest
constexpr int kRcMinBudgetDiv = 8;   // no frame is asked to fit less than T / 8

struct RcConfig {  // thor_hip_rate_control, resolved: the QP ranges no longer hold a 0 / 0 that means 0..51
  int bitrate = 0, buffer_ms = 1000, min_qp = 0, max_qp = 51, min_qp_i = 0, max_qp_i = 51, initial_qp = 0;
  bool on() const { return bitrate > 0; }
};
// The caller's numbers -> c; false: refused (a negative value, min > max, a QP above 51) and c is untouched.  bitrate 0 gives a config that is off.
static inline bool rc_resolve(int bitrate, int buffer_ms, int min_qp, int max_qp, int min_qp_i, int max_qp_i, int initial_qp, RcConfig& c) {
  if (bitrate < 0 || buffer_ms < 0 || min_qp < 0 || max_qp < 0 || min_qp_i < 0 || max_qp_i < 0 || initial_qp < 0) return false;
  if (min_qp == 0 && max_qp == 0) max_qp = 51;
  if (min_qp_i == 0 && max_qp_i == 0) max_qp_i = 51;
  if (min_qp > max_qp || min_qp_i > max_qp_i || max_qp > 51 || max_qp_i > 51 || initial_qp > 51) return false;
  RcConfig r;
  r.bitrate = bitrate; r.buffer_ms = buffer_ms ? buffer_ms : 1000;
  r.min_qp = min_qp; r.max_qp = max_qp; r.min_qp_i = min_qp_i; r.max_qp_i = max_qp_i; r.initial_qp = initial_qp;
  c = r;
  return true;
}

struct RcState {
  long long T = 1, B = 1;                 // bits per frame, buffer size in bits
  long long F = 0;                        // virtual buffer fullness: += bits - T per frame, never below -B
  int overflows = 0;                      // frames that ended with F > B
  int frames = 0;                         // frames coded since the sequence began
  long long factor[RC_CLASSES] = {0};     // bits * step / cost in Q16, moving average of weight 1/2
  long long avg_bits[RC_CLASSES] = {0};   // bits of a frame of the class, moving average of weight 1/4
  int count[RC_CLASSES] = {0};            // frames of the class (all halved when their sum reaches 65536)
  void begin(const RcConfig& c, float frame_rate) {
    *this = RcState();
    T = (long long)((double)c.bitrate / (double)frame_rate);   // the one floating-point line
    if (T < 1) T = 1;
    B = (long long)c.bitrate * c.buffer_ms / 1000;
    if (B < 1) B = 1;
  }
};

static inline long long rc_tdiv(long long a, long long b) { return a >= 0 ? a / b : -((-a) / b); }   // rounds towards zero, stated for the restatement

// Bits the frame may take: T times the class's share of an average inter frame (I frames: kRcIntraBudget), less the fullness paid back over half the
// buffer, at least T / kRcMinBudgetDiv.
static inline long long rc_budget(const RcState& s, int cls) {
  long long budget = s.T;
  if (cls == 0) budget = s.T * kRcIntraBudget;
  else if (s.count[cls] > 0) {
    long long sum = 0, n = 0;
    for (int c = 1; c < RC_CLASSES; c++) { sum += (long long)s.count[c] * s.avg_bits[c]; n += s.count[c]; }
    const long long mean = sum / n > 1 ? sum / n : 1;
    budget = s.T * s.avg_bits[cls] / mean;
  }
  const long long span = s.B / (2 * s.T) > 1 ? s.B / (2 * s.T) : 1;
  budget -= rc_tdiv(s.F, span);
  return budget > s.T / kRcMinBudgetDiv ? budget : s.T / kRcMinBudgetDiv;
}
static inline long long rc_predict(const RcState& s, int cls, long long cost, int frame_qp) {
  const long long f = s.count[cls] > 0 ? s.factor[cls] : kRcInitFactorQ16[cls];
  return f * rc_cost(cost) / kRcStepQ16[frame_qp];
}
// The base QP of the next frame.  frame_qp[b]: the QP the frame is coded at when the base QP is b (GopScheduler::rule_qp).  cost: sum_intra for an I
// frame, else sum_best.
static inline int rc_decide(const RcConfig& c, const RcState& s, int cls, long long cost, const int frame_qp[52]) {
  if (s.frames == 0) return c.initial_qp;   // the caller put the parameter set's qp there when it was 0
  const int lo = cls == 0 ? c.min_qp_i : c.min_qp, hi = cls == 0 ? c.max_qp_i : c.max_qp;
  const long long budget = rc_budget(s, cls);
  for (int b = lo; b < hi; b++)
    if (rc_predict(s, cls, cost, frame_qp[b]) <= budget) return b;
  return hi;
}
// After the frame is coded at frame_qp with `bits` bits.
static inline void rc_update(RcState& s, int cls, long long cost, int frame_qp, long long bits) {
  long long obs = bits * kRcStepQ16[frame_qp] / rc_cost(cost);
  obs = obs < 1 ? 1 : obs > kRcFactorMax ? kRcFactorMax : obs;
  s.factor[cls] = s.count[cls] > 0 ? (s.factor[cls] + obs) / 2 : obs;
  s.avg_bits[cls] = s.count[cls] > 0 ? (3 * s.avg_bits[cls] + bits) / 4 : bits;
  s.count[cls]++;
  int total = 0;
  for (int k = 0; k < RC_CLASSES; k++) total += s.count[k];
  if (total >= 65536)
    for (int k = 0; k < RC_CLASSES; k++) s.count[k] = (s.count[k] + 1) / 2;
  s.F += bits - s.T;
  if (s.F < -s.B) s.F = -s.B;
  if (s.F > s.B) s.overflows++;
  s.frames++;
}

struct RcStat {  // one coded frame of a rate-controlled stream (thor_hip_frame_rc)
  int base_qp = 0, frame_class = 0, qp_rule = 0;   // qp_rule: how the frame's QP follows from base_qp (GopScheduler::rule_qp)
  unsigned long long sum_intra = 0, sum_best = 0, n_intra = 0;
  long long fullness = 0, buffer_bits = 0, target_bits = 0;
  int overflows = 0;
};

// ---- key frames (include/thor_hip.h: thor_hip_scene_cut states the rule) -----------------------------------------------------------------------
constexpr int kMaxKeyRequests = 64;   // pending thor_hip_force_key_frame requests per stream
enum { KEY_SCHEDULE = 0, KEY_FORCED = 1, KEY_SCENE_CUT = 2 };
struct ScConfig {  // thor_hip_scene_cut, resolved
  int percent = 0, min_interval = 0;
  bool on() const { return percent > 0; }
};
static inline bool sc_resolve(int percent, int min_interval, ScConfig& c) {
  if (percent < 0 || percent > 100 || min_interval < 0) return false;
  c.percent = percent; c.min_interval = min_interval;
  return true;
}
// Is the P frame frame_num of a stream whose last I frame was last_intra a scene cut?  had_prev: its analysis had a previous plane.  The sums are at most
// 2^36 (kRcCostMax: an 8192 x 8192 frame of 12-bit samples) and percent at most 100 < 2^7, so both products stay below 2^43.
static inline bool sc_is_cut(const ScConfig& c, bool had_prev, int frame_num, int last_intra, unsigned long long sum_intra, unsigned long long sum_best) {
  if (!c.on() || !had_prev) return false;
  if (frame_num - last_intra < (c.min_interval > 1 ? c.min_interval : 1)) return false;
  return sum_intra > 0 && sum_best * 100ull >= (unsigned long long)c.percent * sum_intra;
}

}  // namespace tk
