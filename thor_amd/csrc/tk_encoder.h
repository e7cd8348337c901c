// tk_encoder.h - host side of the engine: stream state in device memory, per-frame job set-up,
// superblock wavefront scheduling, bitstream assembly.  Shared by the HIP library (kernels in
// hip_kernels.h / tk_kernel.h, launched by hip_backend.h) and by the 1-lane host simulation used in CPU tests (hostsim.cpp); the two
// differ only in the `backend` functions declared below.
// Specification followed: enc/encode_frame.c:637-850 (encode_frame: lambda, header, SB raster
// order, deblock, CDEF, reference rotation), enc/write_bits.c:49-121 (sequence / frame header),
// enc/putbits.c:45-83 (frame framing), enc/mainenc.c:246-523 (low-delay GOP: frame types, QPs and
// reference lists).
#pragma once
#include <vector>
#include <string>
#include <thread>
#include <cstdio>
#include <cstring>
#include <cmath>
#include "tk_common.h"
#include "tk_tables.h"
#include "tk_cdef.h"
#include "tk_interp_dev.h"
#include "tk_clpf.h"
#include "tk_filters.h"
#include "tk_scale.h"
#include "tk_rc.h"
#include "tk_tf.h"
#include "tk_report.h"

namespace tk {

// ---- backend (device memory + launches) ------------------------------------------------
namespace backend {
void* dev_alloc(size_t n);
void dev_free(void* p);
void h2d(void* d, const void* h, size_t n);
void d2h(void* h, const void* d, size_t n);
void dev_memset(void* d, int v, size_t n);
void dev_sync();
size_t team_ws_bytes(int pix_bytes);
// jobs: device array of S FrameJob; hjobs: the same on the host.  ranges (host array of S, or nullptr = whole frames): the anti-diagonals
// t = l + 2k of the superblock grid, [lo, hi), that this launch codes of every stream (tk_sched.h; lo == hi: nothing).
struct SbRange { unsigned short lo, hi; };
template <typename PIX> void run_superblocks(const FrameJob<PIX>* jobs, const FrameJob<PIX>* hjobs, int S, const SbRange* ranges);
template <typename PIX> void run_clpf_stats(const ClpfJob<PIX>* jobs, const ClpfJob<PIX>* hjobs, int S);
template <typename PIX> void run_clpf_apply(const ClpfJob<PIX>* jobs, const ClpfJob<PIX>* hjobs, int S);  // copies rec -> src first
template <typename PIX> void run_deblock(const FrameJob<PIX>* jobs, const FrameJob<PIX>* hjobs, int S);
template <typename PIX> void run_make_ref(const FrameJob<PIX>* hjobs, const Plane3<PIX>* dst, int S);
// copies rec -> src, then runs the five CDEF passes; cjobs/hcjobs: device/host arrays of S CdefJob
template <typename PIX> void run_cdef(const CdefJob<PIX>* cjobs, const CdefJob<PIX>* hcjobs, int S);
// bit-level concatenation of per-SB bit strings: item i copies nbits[i] bits from src[i] to bit offset dst_bit[i] of dst
struct GatherItem { const uint32_t* src; int nbits; long long dst_bit; };
void run_gather(const GatherItem* d_items, int n, uint32_t* dst);
void release_superblocks(const void* jobs);  // frees the scheduler state run_superblocks keeps for this job array
// temporally interpolated reference frames of n streams (all phases: pyramid, block search per level, merge, upscale,
// motion compensation, padding); jobs/hjobs: device/host arrays of n idev::Job
template <typename PIX> void run_interp(const idev::Job<PIX>* jobs, const idev::Job<PIX>* hjobs, int n);
// the launch templates above for one sample type: each backend instantiates them for uint8_t and uint16_t
#define TK_BACKEND_INSTANTIATE(PIX)                                                                      \
  template void run_interp<PIX>(const idev::Job<PIX>*, const idev::Job<PIX>*, int);                      \
  template void run_superblocks<PIX>(const FrameJob<PIX>*, const FrameJob<PIX>*, int, const SbRange*);   \
  template void run_deblock<PIX>(const FrameJob<PIX>*, const FrameJob<PIX>*, int);                       \
  template void run_make_ref<PIX>(const FrameJob<PIX>*, const Plane3<PIX>*, int);                        \
  template void run_cdef<PIX>(const CdefJob<PIX>*, const CdefJob<PIX>*, int);                            \
  template void run_clpf_stats<PIX>(const ClpfJob<PIX>*, const ClpfJob<PIX>*, int);                      \
  template void run_clpf_apply<PIX>(const ClpfJob<PIX>*, const ClpfJob<PIX>*, int);
}  // namespace backend
#if !TK_HOST
// Per-plane sums of squared differences orig - rec of S streams into out[4 * s + plane] (added: the caller clears the slots), one launch
// (hip_kernels.h: k_frame_sse, launched by hip_backend.h).  The host build calls frame_sse_rows directly (Engine::finish_frames).
template <typename PIX> void launch_frame_sse(const FrameJob<PIX>* jobs, const FrameJob<PIX>* hjobs, int S, unsigned long long* out);
// Input at a lower bit depth than the engine's (bitdepth > input_bitdepth; tk_filters.h: depth_up_rows, depth_down_rows, frame_sse_depth_rows), one
// launch each on the library's stream.  `packed`: a packed planar 4:2:0 frame of input-depth samples in device memory.  The host build calls the row
// functions directly (Engine::widen / narrow / finish_frames).
void launch_depth_up(const void* packed, const Plane3<uint16_t>& dst, int width, int height, int bitdepth, int input_bitdepth);
void launch_depth_down(const Plane3<uint16_t>& src, void* packed, int width, int height, int bitdepth, int input_bitdepth);
void launch_frame_sse_depth(const FrameJob<uint16_t>* jobs, const FrameJob<uint16_t>* hjobs, int S, int bitdepth, int input_bitdepth, unsigned long long* out);
// A frame in a caller's layout (tk_filters.h: PixLayout, layout_in_rows, layout_out_rows) <-> planes at the engine's depth, one launch each on the
// library's stream.  `frame`: device memory.  The host build calls the row functions directly (Engine::layout_in / layout_out).
template <typename PIX> void launch_layout_in(const void* frame, const PixLayout& L, const Plane3<PIX>& dst, int width, int height, int bitdepth, int input_bitdepth);
template <typename PIX> void launch_layout_out(const Plane3<PIX>& src, void* frame, const PixLayout& L, int width, int height, int bitdepth, int input_bitdepth);
// An RGB frame (tk_filters.h: RgbFormat, rgb_in_rows, rgb_out_rows) <-> planes at the engine's depth, one launch each on the library's stream.
template <typename PIX> void launch_rgb_in(const void* frame, const RgbFormat& R, const Plane3<PIX>& dst, int width, int height, int bitdepth, int input_bitdepth);
template <typename PIX> void launch_rgb_out(const Plane3<PIX>& src, void* frame, const RgbFormat& R, int width, int height, int bitdepth, int input_bitdepth);
// A frame of another size (tk_scale.h: ScalePlan, k_scale_in) -> planes at the engine's depth, one launch on the library's stream.
template <typename PIX> void launch_scale_in(const void* frame, const PixLayout& L, const ScaleTables& tab, int vrows, const Plane3<PIX>& dst, int src_w, int width,
                                             int height, int bitdepth, int input_bitdepth);
// The frame analysis of rate control (tk_rc.h, k_rc_cost) of n streams, one launch on the library's stream.  jobs / hjobs: device / host arrays of n RcJob.
template <typename PIX> void launch_rc_cost(const RcJob<PIX>* jobs, const RcJob<PIX>* hjobs, int n);
// The same against previous originals (RcJob::prev_y): the kernel's other instantiation, which stores nothing but the sums.
template <typename PIX> void launch_rc_cost_orig(const RcJob<PIX>* jobs, const RcJob<PIX>* hjobs, int n);
// The temporal filter (tk_tf.h) of n requests: k_tf_search for every neighbour of every request, then k_tf_blend, two launches on the library's stream.
template <typename PIX> void launch_tf(const TfJob<PIX>* jobs, const TfJob<PIX>* hjobs, int n);
#endif

// ---- parameters -------------------------------------------------------------------------
struct SeqParams {  // the enc_params fields this path honours (enc/mainenc.h:35-112)
  int width = 0, height = 0, qp = 32;
  int bitdepth = 8, input_bitdepth = 8;
  float frame_rate = 30.f;
  float lambda_coeffI = 1.f, lambda_coeffP = 1.f, lambda_coeffB = 1.f, lambda_coeffB0 = 1.f, lambda_coeffB1 = 1.f, lambda_coeffB2 = 1.f, lambda_coeffB3 = 1.f;
  float early_skip_thr = 0.f;
  int enable_tb_split = 0, enable_pb_split = 0, max_num_ref = 1, HQperiod = 1;
  int num_reorder_pics = 0, dyadic_coding = 1, interp_ref = 0;
  int dqpP = 0, dqpI = 0, dqpB = 0, dqpB0 = 0, dqpB1 = 0, dqpB2 = 0, dqpB3 = 0;
  float mqpP = 1.f, mqpB = 1.f, mqpB0 = 1.f, mqpB1 = 1.f, mqpB2 = 1.f, mqpB3 = 1.f;
  int intra_period = 0, intra_rdo = 0, encoder_speed = 0;
  int deblocking = 1, cdef = 2, clpf = 0, max_clpf_strength = 4, use_block_contexts = 0, enable_bipred = 0;
  int cfl_intra = 1, cfl_inter = 0;
  int log2_sb_size = 7;
};

struct FrameParams {
  int frame_type = F_I, qp = 32, num_ref = 0, frame_num = 0, interp_ref = 0, num_intra_modes = 10;
  int ref_array[kMaxRefs] = {0, 0, 0, 0};  // indices into the sliding window (0 = most recent); -1 = interpolated frame
  int interp_src[2] = {0, 0};              // window indices the interpolated frame is built from (before pruning)
  double lambda_coeff = 1.0;
  int b_level = 0;
  int qp_rule = 0;                         // QR_*: how qp follows from the base QP (GopScheduler::rule_qp)
  int key_reason = 0;                      // KEY_*: why the frame is an I frame when the schedule alone would not have made it one (tk_rc.h)
};
enum { QR_BASE = 0, QR_I, QR_P, QR_B0, QR_B1, QR_B2, QR_B3, QR_B };

// Coding-order schedule of one stream: a resumable restatement of the frame loop of enc/mainenc.c:246-625
// (frame types, QPs, b_level, reference lists for low-delay and dyadic hierarchical-B GOPs, the fall-back
// to PPP coding for a tail that does not fill a sub-GOP, duplicate / pre-intra reference removal).
// frame numbers are relative to `skip` like encoder_info.frame_info.frame_num.
struct GopScheduler {
  SeqParams sp;             // HQperiod / num_reorder_pics mutate at the tail exactly like the reference's params
  int skip = 0, num_frames = 0, file_frames = 0;
  int frame_num0 = 0, k = 0, sub_gop = 1, num_encoded = 0, last_intra = 0, last_PorI = -1, min_interp_depth = 0;
  bool started = false;
  int key_req[kMaxKeyRequests];   // frame numbers a key frame was asked for (thor_hip_force_key_frame), low delay only; a request leaves when its frame is scheduled
  int n_key = 0;
  static int ilog2i(unsigned v) { int n = 0; while (v >>= 1) n++; return n; }
  static int code_to_display(int sub, int idx) {
    static const int cd1[1] = {0}, cd2[2] = {1, 0}, cd4[4] = {3, 1, 0, 2}, cd8[8] = {7, 3, 1, 5, 0, 2, 4, 6},
                     cd16[16] = {15, 7, 3, 11, 1, 5, 9, 13, 0, 2, 4, 6, 8, 10, 12, 14};
    const int* t[5] = {cd1, cd2, cd4, cd8, cd16};
    return t[ilog2i(sub)][idx];
  }
  static int display_to_code(int sub, int idx) {
    static const int dc1[2] = {-1, 0}, dc2[3] = {-2, 1, 0}, dc4[5] = {-4, 2, 1, 3, 0}, dc8[9] = {-8, 4, 2, 5, 1, 6, 3, 7, 0},
                     dc16[17] = {-16, 8, 4, 9, 2, 10, 5, 11, 1, 12, 6, 13, 3, 14, 7, 15, 0};
    const int* t[5] = {dc1, dc2, dc4, dc8, dc16};
    return t[ilog2i(sub)][idx];
  }
  void init(const SeqParams& p, int skip_, int nframes, int file_frames_) {
    sp = p; skip = skip_; num_frames = nframes; file_frames = file_frames_;
    sub_gop = p.num_reorder_pics + 1 > 1 ? p.num_reorder_pics + 1 : 1;
    min_interp_depth = ilog2i((unsigned)(p.num_reorder_pics + 1)) - 3;
    if (p.frame_rate > 30) min_interp_depth--;
    frame_num0 = skip; k = 0; num_encoded = 0; last_intra = 0; last_PorI = -1; started = true;
    n_key = 0;
  }
  // A key frame at chunk-relative frame frame_num; false: the set is full.  A frame asked for twice is held once.
  bool request_key(int frame_num) {
    for (int i = 0; i < n_key; i++)
      if (key_req[i] == frame_num) return true;
    if (n_key == kMaxKeyRequests) return false;
    key_req[n_key++] = frame_num;
    return true;
  }
  bool take_key(int frame_num) {
    for (int i = 0; i < n_key; i++)
      if (key_req[i] == frame_num) { key_req[i] = key_req[--n_key]; return true; }
    return false;
  }
  int intra_modes(int frame_type) const { return (sp.intra_rdo == 0 || (frame_type != F_I && sp.encoder_speed > 0)) ? 4 : 10; }
  // Make f the I frame intra_period would have made at its place: every I frame of next() passes here, and so does a frame next() returned as a P
  // frame that is promoted afterwards (a request for the frame already scheduled, a scene cut).  Nothing else of the schedule moves: num_encoded,
  // the HQperiod phase and last_PorI run on; later frames drop the references older than this frame (last_intra).
  void promote(FrameParams& f, int reason) {
    f.frame_type = F_I;
    f.qp_rule = QR_I;
    f.qp = rule_qp(sp, QR_I, sp.qp);
    f.num_ref = 0;
    for (int r = 0; r < kMaxRefs; r++) f.ref_array[r] = 0;
    f.num_intra_modes = intra_modes(F_I);
    f.lambda_coeff = sp.lambda_coeffI;
    f.key_reason = reason;
    last_intra = f.frame_num;
  }
  // The QP of a frame from the base QP (mainenc.c:281-314): which of the dqp / mqp pairs applies is the frame's qp_rule, set by next(); the base is the
  // parameter set's qp, or the rate control's choice for the frame (Engine::rate_control).
  static int rule_qp(const SeqParams& p, int rule, int base) {
    int q = base;
    if (rule == QR_I) q = base + p.dqpI;
    else if (rule == QR_P) q = (int)(p.mqpP * (float)base) + p.dqpP;
    else if (rule == QR_B0) q = (int)(p.mqpB0 * (float)base) + p.dqpB0;
    else if (rule == QR_B1) q = (int)(p.mqpB1 * (float)base) + p.dqpB1;
    else if (rule == QR_B2) q = (int)(p.mqpB2 * (float)base) + p.dqpB2;
    else if (rule == QR_B3) q = (int)(p.mqpB3 * (float)base) + p.dqpB3;
    else if (rule == QR_B) q = (int)(p.mqpB * (float)base) + p.dqpB;
    return q < 0 ? 0 : (q > 51 ? 51 : q);
  }
  // ring_frame_num(idx): frame_num of the reconstruction currently at sliding-window position idx.
  // Returns false when the sequence is finished; otherwise fills f and the absolute input frame index.
  template <class RingF> bool next(FrameParams& f, int& abs_frame, RingF ring_frame_num) {
    for (;;) {
      if (!(frame_num0 < skip + num_frames && frame_num0 + 1 <= file_frames)) return false;
      if (k >= sub_gop) {
        // end of a sub-GOP: tail fall-back (mainenc.c:615-623)
        if ((frame_num0 + sub_gop + 1 > file_frames || frame_num0 + sub_gop >= skip + num_frames) && sub_gop >= 2) {
          sp.HQperiod = sub_gop; sub_gop = 1; sp.num_reorder_pics = 0;
        }
        frame_num0 += sub_gop;  // the for-increment runs after the fall-back, i.e. with the NEW sub_gop
        k = 0;
        continue;
      }
      const int dyadic = sp.dyadic_coding;
      int frame_offset;
      if (dyadic && sub_gop > 1) frame_offset = code_to_display(sub_gop, k) - sub_gop + 1;
      else frame_offset = k == 0 ? 0 : k - sub_gop;
      const int frame_num_abs = frame_num0 + frame_offset;
      k++;
      if (frame_num_abs < skip) continue;
      f = FrameParams();
      f.frame_num = frame_num_abs - skip;
      abs_frame = frame_num_abs;
      if (sp.num_reorder_pics == 0) {
        if (sp.intra_period > 0) f.frame_type = (num_encoded % sp.intra_period) == 0 ? F_I : F_P;
        else f.frame_type = num_encoded == 0 ? F_I : F_P;
        if (n_key && take_key(f.frame_num) && f.frame_type != F_I) { f.frame_type = F_I; f.key_reason = KEY_FORCED; }
      } else {
        if (sp.intra_period > 0) f.frame_type = (f.frame_num % sp.intra_period) == 0 ? F_I : ((f.frame_num % sub_gop) == 0 ? F_P : F_B);
        else f.frame_type = f.frame_num == 0 ? F_I : ((f.frame_num % sub_gop) == 0 ? F_P : F_B);
      }
      const int coded_phase = (num_encoded + sub_gop - 2) % sub_gop + 1;
      const int b_level = ilog2i((unsigned)coded_phase);
      f.b_level = b_level;
      if (f.frame_type == F_I) {}   // an I frame's fields: promote(), below; it builds no reference list
      else if (sp.num_reorder_pics == 0) f.qp_rule = (num_encoded % sp.HQperiod) ? QR_P : QR_BASE;
      else if (f.frame_num % sub_gop) f.qp_rule = !dyadic ? QR_B : b_level == 0 ? QR_B0 : b_level == 1 ? QR_B1 : b_level == 2 ? QR_B2 : b_level == 3 ? QR_B3 : QR_B;
      else f.qp_rule = (f.frame_num % sp.HQperiod) ? QR_P : QR_BASE;
      f.qp = rule_qp(sp, f.qp_rule, sp.qp);
      f.num_ref = f.frame_type == F_I ? 0 : (num_encoded < sp.max_num_ref ? num_encoded : sp.max_num_ref);
      f.interp_ref = 0;
      int ra[kMaxRefs + 2] = {0, 0, 0, 0, 0, 0};
      auto imin = [](int a, int b) { return a < b ? a : b; };
      if (f.num_ref > 0) {
        if (sp.num_reorder_pics > 0) {
          if (dyadic) {
            if ((num_encoded - 1) % sub_gop == 0) {  // P frame: previous anchors
              ra[0] = num_encoded == 1 ? 0 : sub_gop - 1;
              if (f.num_ref > 1) ra[1] = imin(32, imin(num_encoded - 1, 2 * sub_gop - 1));
              for (int r = 2; r < f.num_ref; r++) ra[r] = r - 2;
            } else {
              const int display_phase = (f.frame_num - 1) % sub_gop;
              const int ref_offset = sub_gop >> (b_level + 1);
              if (b_level >= min_interp_depth && sp.interp_ref == 1) {
                if (f.num_ref == 2) f.num_ref++;
                f.interp_ref = sp.interp_ref;
                ra[1] = imin(num_encoded - 1, coded_phase - display_to_code(sub_gop, display_phase - ref_offset + 1) - 1);
                ra[2] = imin(num_encoded - 1, coded_phase - display_to_code(sub_gop, display_phase + ref_offset + 1) - 1);
                ra[0] = -1;
                f.interp_src[0] = ra[1]; f.interp_src[1] = ra[2];
                for (int r = 3; r < f.num_ref; r++) ra[r] = r - 3;
              } else {
                ra[0] = imin(num_encoded - 1, coded_phase - display_to_code(sub_gop, display_phase - ref_offset + 1) - 1);
                ra[1] = imin(num_encoded - 1, coded_phase - display_to_code(sub_gop, display_phase + ref_offset + 1) - 1);
                for (int r = 2; r < f.num_ref; r++) ra[r] = r - 2;
              }
            }
          } else {
            fprintf(stderr, "thor_hip: non-dyadic reordering is not implemented\n");
            abort();
          }
        } else {
          ra[0] = last_PorI;
          const int r1 = ((num_encoded + sp.HQperiod - 2) % sp.HQperiod) + 1;
          const int r2 = r1 == 1 ? 2 : 1;
          int r3 = r2 + 1;
          if (r3 == r1) r3 += 1;
          if (f.num_ref == 2) ra[1] = r1;
          else if (f.num_ref == 3) { ra[1] = r1; ra[2] = r2; }
          else if (f.num_ref == 4) { ra[1] = r1; ra[2] = r2; ra[3] = r3; }
        }
      }
      for (int r = f.num_ref - 1; r > 0; --r)
        for (int q = r - 1; q >= 0; --q)
          if (ra[q] == ra[r]) {
            for (int s2 = r; s2 < f.num_ref - 1; ++s2) ra[s2] = ra[s2 + 1];
            f.num_ref--;
            break;
          }
      if (f.frame_num > last_intra)
        for (int r = f.num_ref - 1; r >= 0; --r)
          if (ra[r] >= 0 && ring_frame_num(ra[r]) < last_intra) {
            for (int s2 = r; s2 < f.num_ref - 1; ++s2) ra[s2] = ra[s2 + 1];
            f.num_ref--;
          }
      for (int r = 0; r < kMaxRefs; r++) f.ref_array[r] = ra[r];
      f.num_intra_modes = intra_modes(f.frame_type);
      if (f.frame_type == F_I) promote(f, f.key_reason);
      else if (f.frame_type == F_P) f.lambda_coeff = sp.lambda_coeffP;
      else f.lambda_coeff = b_level == 0 ? sp.lambda_coeffB0 : b_level == 1 ? sp.lambda_coeffB1 : b_level == 2 ? sp.lambda_coeffB2
                                                                              : b_level == 3 ? sp.lambda_coeffB3 : sp.lambda_coeffB;
      return true;
    }
  }
  // call after the frame returned by next() has been encoded (mainenc.c:552, 611)
  void advance(const FrameParams& f) {
    num_encoded++;
    last_PorI = f.frame_type != F_B ? 0 : last_PorI + 1;
  }
};

// ---- host bit writer (MSB first) ---------------------------------------------------------
struct HostBits {
  std::vector<uint32_t> w;  // word i holds stream bits [32i, 32i+32), first bit in the MSB
  int nbits = 0;
  void put(int n, uint32_t v) {
    if (n <= 0) return;
    if (n < 32) v &= (1u << n) - 1u;
    const int off = nbits & 31, room = 32 - off;
    if (off == 0) w.push_back(0);
    if (n <= room) {
      w.back() |= v << (room - n);
    } else {
      const int lo = n - room;
      w.back() |= v >> lo;
      w.push_back(v << (32 - lo));
    }
    nbits += n;
  }
  // append nb bits taken MSB-first from 32-bit words (device BitSink layout)
  void append_words(const uint32_t* src, int nb) {
    int i = 0;
    for (; i + 32 <= nb; i += 32) put(32, src[i >> 5]);
    if (i < nb) put(nb - i, src[i >> 5] >> (32 - (nb - i)));
  }
  void overwrite(int pos, int n, uint32_t v) {  // header back-patching, bit by bit (tiny)
    for (int i = n - 1; i >= 0; i--, pos++) {
      const uint32_t m = 0x80000000u >> (pos & 31);
      if ((v >> i) & 1u) w[pos >> 5] |= m; else w[pos >> 5] &= ~m;
    }
  }
  int get(int pos) const { return (int)((w[pos >> 5] >> (31 - (pos & 31))) & 1u); }
  size_t num_bytes() const { return ((size_t)nbits + 7) / 8; }
  void to_bytes(std::vector<uint8_t>& out) const {  // big-endian words -> byte stream
    const size_t nb = num_bytes();
    for (size_t i = 0; i < nb; i++) out.push_back((uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3))));
  }
  void clear() { w.clear(); nbits = 0; }
};

inline void write_sequence_header(HostBits& b, const SeqParams& p) {  // write_bits.c:49-81 (4:2:0, no qmtx)
  b.put(16, p.width); b.put(16, p.height); b.put(3, p.log2_sb_size);
  b.put(1, p.enable_pb_split); b.put(1, p.enable_tb_split); b.put(2, p.max_num_ref - 1);
  b.put(2, p.interp_ref); b.put(1, 0 /*delta qp*/); b.put(1, p.deblocking); b.put(1, p.clpf ? 1 : 0);
  b.put(1, p.use_block_contexts); b.put(2, p.enable_bipred); b.put(1, 0 /*qmtx*/);
  b.put(2, 1 /*420*/); b.put(4, p.num_reorder_pics); b.put(1, p.cfl_intra); b.put(1, p.cfl_inter);
  b.put(1, p.bitdepth != 8);
  if (p.bitdepth != 8) b.put(1, p.bitdepth == 12);
  b.put(1, p.input_bitdepth != 8);
  if (p.input_bitdepth != 8) b.put(1, p.input_bitdepth == 12);
}

struct CdefHeader {
  int damping = 5, bits = 0;
  int strengths[8] = {0}, uv_strengths[8] = {0};
};
inline void write_cdef_params(HostBits& b, int pos_or_minus1, int cdef_on, const CdefHeader& h, int phase = 0) {  // write_bits.c:83-97
  HostBits tmp;
  if (cdef_on) {
    tmp.put(2, h.damping - 3); tmp.put(2, h.bits);
    for (int i = 0; i < (1 << h.bits); i++) { tmp.put(7, h.strengths[i]); tmp.put(7, h.uv_strengths[i]); }
  } else tmp.put(18, 0);
  if (pos_or_minus1 < 0) {
    for (int i = 0; i < tmp.nbits; i++) b.put(1, (uint32_t)tmp.get(i));
  } else {
    // Back-patch as the reference's stream writer performs it (enc/putbits.c:130-144): write_stream_pos()
    // back to the saved header position, rewrite, write_stream_pos() forward again.  The forward move restores
    // the saved 32-bit accumulator of the CURRENT position, so patched bits that fall into the stream's last,
    // not yet flushed word are lost and the originally written bits stay (visible on tiny frames).
    // `phase`: bit position (mod 32) of b's bit 0 in the stream the reference would be writing to (0 unless the bits
    // are appended to a caller's stream that already holds unflushed bits - drop-in seam, frame 0 after the sequence header).
    const int unflushed = (((b.nbits + phase) >> 5) << 5) - phase;
    for (int i = 0; i < tmp.nbits; i++)
      if (pos_or_minus1 + i < unflushed) b.overwrite(pos_or_minus1 + i, 1, (uint32_t)tmp.get(i));
  }
}

// ---- per-stream device state ---------------------------------------------------------------
template <typename PIX> struct DevFrame {
  PIX* base_y = nullptr;
  PIX* base_c = nullptr;
  Plane3<PIX> p;
  int frame_num = -1;
  void alloc(int w, int h, int pad) {
    int sy = (w + 2 * pad + 15) & ~15, sc = (w / 2 + 2 * (pad / 2) + 15) & ~15;
    size_t ay = (size_t)(h + 2 * pad) * sy + 64, ac = (size_t)(h / 2 + 2 * (pad / 2)) * sc + 64;
    base_y = (PIX*)backend::dev_alloc(ay * sizeof(PIX));
    base_c = (PIX*)backend::dev_alloc(2 * ac * sizeof(PIX));
    p.sy = sy; p.sc = sc;
    p.y = base_y + (size_t)pad * sy + pad;
    p.u = base_c + (size_t)(pad / 2) * sc + pad / 2;
    p.v = p.u + ac;
  }
  void release() { backend::dev_free(base_y); backend::dev_free(base_c); base_y = base_c = nullptr; }
};

template <typename PIX> struct Stream {
  DevFrame<PIX> orig, rec, tmp, interp;
  std::vector<DevFrame<PIX>> ring;  // sliding window, ring[0] = most recent reconstruction
  DbCell* cells = nullptr;
  uint32_t* sb_bits = nullptr;
  int* sb_nbits = nullptr;
  int* sb_status = nullptr;
  uint8_t* scratch = nullptr;
  // CDEF state
  int8_t* cdef_dir = nullptr; int* cdef_var = nullptr; int* cdef_fbc = nullptr; unsigned long long* cdef_mse = nullptr;
  int* cdef_sel = nullptr; int* cdef_fbsel = nullptr; CdefResult* cdef_res = nullptr; unsigned long long* cdef_tot = nullptr;
  uint32_t* clpf_stats = nullptr; uint8_t* clpf_fb_on = nullptr;   // CLPF: per-8x8 statistics, per-filter-block switches
  // temporal interpolation (interp_ref = 1): pyramid planes and per-level vector fields, device resident
  int ip_levels = 0;
  PIX* ip_pic[2][idev::kMaxLevels] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};  // allocation bases
  int ip_stride[idev::kMaxLevels] = {0, 0, 0, 0};
  idev::imv* ip_mv[idev::kMaxLevels][5] = {};   // mv0, mv1, nmv0, nmv1, guide per level
  int* ip_prog[idev::kMaxLevels] = {nullptr, nullptr, nullptr, nullptr};   // progress counters + ticket (last entry)
  int num_encoded = 0;
  GopScheduler gop;          // coding-order schedule (initialised by begin_sequence or lazily as open-ended low delay)
  FrameParams cur;           // frame returned by the last schedule()
  int cur_abs = 0;           // its absolute input frame index
  HostBits bits;             // bits of the frame being assembled (sequence header rides on frame 0)
  int bit_phase = 0;         // raw_frames mode: bit position mod 32 of the caller's stream at frame start
  std::vector<uint8_t> out;  // finished stream bytes (4-byte big-endian length + payload per frame)
  int sh_bits = 0;           // bits of the sequence header
  std::vector<FrameStat> log;  // one record per coded frame, in coding order (cleared by begin_sequence)
  // rate control (tk_rc.h; off unless Engine::set_rate_control turned it on): nothing below is allocated or touched while it is off
  RcConfig rc;
  RcState rcs;
  PIX* rc_half[2] = {nullptr, nullptr};  // the half-size luma of the frame analysed last and of the one before: they alternate
  int rc_flip = 0;                       // the plane the next analysis writes
  bool rc_prev = false;                  // the other plane holds the previous frame of this sequence
  RcStat rc_cur;                         // the frame in flight: the decision and its analysis sums
  std::vector<RcStat> rclog;             // one record per coded frame, like `log`
  // scene cuts (tk_rc.h: ScConfig; off unless Engine::set_scene_cut turned them on).  They share the analysis and its two half planes with rate control.
  ScConfig sc;
  bool key_analysed = false;             // the frame in flight was analysed: key_sums goes into its record
  unsigned long long key_sums[3] = {0, 0, 0};
};

// The caller-visible fields of the reference's deblock_data_t (common/types.h:178-187) in declaration order, from one DbCell:
// cbp.y/u/v are 0/1 in the reference too (quantize() returns a flag; transform-split blocks store 1/1/1, encode_block.c:1495-1498).
struct DdFields { int mode, cbp_y, cbp_u, cbp_v, size, tb_split, pb_part, mv0x, mv0y, mv1x, mv1y, ref_idx0, ref_idx1, bipred_flag; };
static inline DdFields dd_fields(const DbCell& c) {
  DdFields d;
  d.mode = c.mode; d.cbp_y = c.cbp & 1; d.cbp_u = (c.cbp >> 1) & 1; d.cbp_v = (c.cbp >> 2) & 1;
  d.size = c.size; d.tb_split = c.tbpb & 1; d.pb_part = c.tbpb >> 1;
  d.mv0x = c.mv0.x; d.mv0y = c.mv0.y; d.mv1x = c.mv1.x; d.mv1y = c.mv1.y;
  d.ref_idx0 = c.ref0; d.ref_idx1 = c.ref1; d.bipred_flag = c.dir;
  return d;
}

template <typename PIX> class Engine {
 public:
  SeqParams sp;
  int S = 0, sb_cols = 0, sb_rows = 0, nsb = 0, max_diag = 0, ring_size = 0;
  // Bit buffer of one 128x128 superblock: 2^19 bits for 24576 samples (4:2:0), 21.3 bits per sample.  The buffer of a smaller superblock
  // (sb_words) is its share by area: the same bound per sample, which is what the worst case follows (the split flags and block headers of a
  // 64x64 superblock are a quarter of those of a 128x128 one, its coefficients too).  The overflow check of finish_frames stays the guard.
  static const int kSbWords = 16384;
  int sb_words = kSbWords;
  std::vector<Stream<PIX>> st;
  FrameJob<PIX>* d_jobs = nullptr;
  std::vector<FrameJob<PIX>> h_jobs;
  CdefJob<PIX>* d_cjobs = nullptr;
  std::vector<CdefJob<PIX>> h_cjobs;
  ClpfJob<PIX>* d_ljobs = nullptr;
  std::vector<ClpfJob<PIX>> h_ljobs;
  int nfb_h = 0, nfb_v = 0;
  size_t ws_bytes = 0;
  int* d_nbits_all = nullptr; int* d_status_all = nullptr;   // [S][nsb]
  uint32_t* d_payload = nullptr; size_t payload_words = 0;   // compacted SB bits of all streams
  backend::GatherItem* d_items = nullptr;
  bool external_interp = false;  // drop-in mode: the caller uploads st[s].interp itself
  bool raw_frames = false;  // drop-in mode: no sequence header / framing; caller consumes st[s].bits
  unsigned long long* d_stats = nullptr;  // FrameJob::stats (4 counters + spare)
  long long* d_prof = nullptr;  // 32 cycle counters summed over all superblocks (THOR_PROF builds)
  idev::Job<PIX>* d_ijobs = nullptr;
  std::vector<idev::Job<PIX>> h_ijobs;
  bool frame_distortion = false;        // measure the per-plane SSE of every coded frame (off: a frame's launches and copies are unchanged)
  unsigned long long* d_sse = nullptr;  // [S][4]: Y, U, V sums of the frame just finished (allocated on first use)
  void* d_packed = nullptr;             // input_bitdepth < bitdepth: one packed frame of input-depth samples, staging for upload_orig / download_rec
  void* d_layout = nullptr;             // a host frame in a caller's layout, as it came (stage_layout_host / fetch_layout_host); allocated on first use
  size_t d_layout_bytes = 0;
  ScalePlan scale_plan;                 // the most recent scaled staging (resolve_scaled), its tables in device memory and whether those are stale
  void* d_scale = nullptr;
  ScaleTables scale_tab;
  bool scale_dirty = true;
  RcJob<PIX>* d_rcjobs = nullptr;         // rate control: the analysis jobs and, per stream, four slots for the three sums (allocated on first use)
  unsigned long long* d_rcsums = nullptr;
  RcJob<PIX>* d_scjob = nullptr;          // scene_cost: its one job and its sums (allocated on first use)
  unsigned long long* d_scsums = nullptr;
  TfJob<PIX>* d_tfjobs = nullptr;         // filter_frames: its jobs and the block records of tf_cap requests (allocated on first use, grown on demand)
  TfBlock* d_tfblk = nullptr;
  int tf_cap = 0;

  // Frames cross the engine's boundary at the INPUT depth (upload_orig, download_rec, the files of cli_run): one byte per sample for depth 8, two otherwise.
  int depth_shift() const { return sp.bitdepth - sp.input_bitdepth; }
  size_t frame_bytes() const { return (size_t)sp.width * sp.height * 3 / 2 * (sp.input_bitdepth > 8 ? 2 : 1); }

  void open(const SeqParams& p, int num_streams) {
    sp = p; S = num_streams;
    // the superblock grid (encode_frame.c:642-644); open() is only reached with log2_sb_size 6 or 7 (tk_cli.h, hip_abi_seq.h:unsupported)
    const int sb_size = 1 << p.log2_sb_size, sb_shift = kLog2MaxSb - p.log2_sb_size;
    if (sb_shift < 0 || sb_shift > 1) { fprintf(stderr, "Run-time error...\nthor_hip: log2_sb_size must be 6 or 7\n...now exiting to system...\n"); abort(); }
    sb_cols = (p.width + sb_size - 1) / sb_size; sb_rows = (p.height + sb_size - 1) / sb_size; nsb = sb_cols * sb_rows;
    sb_words = kSbWords >> (2 * sb_shift);
    max_diag = 0;
    for (int t = 0; t <= (sb_cols - 1) + 2 * (sb_rows - 1); t++) {
      int n = 0;
      for (int k = 0; k < sb_rows; k++) { int l = t - 2 * k; if (l >= 0 && l < sb_cols) n++; }
      if (n > max_diag) max_diag = n;
    }
    nfb_h = (p.width + 63) >> 6; nfb_v = (p.height + 63) >> 6;
    ring_size = (p.HQperiod > p.max_num_ref ? p.HQperiod : p.max_num_ref) + 1;
    if (p.num_reorder_pics > 0) ring_size = 2 * (p.num_reorder_pics + 1) + 1 > ring_size ? 2 * (p.num_reorder_pics + 1) + 1 : ring_size;
    if (ring_size > 33) ring_size = 33;
    ws_bytes = (backend::team_ws_bytes((int)sizeof(PIX)) + 255) & ~(size_t)255;
    st.resize(S);
    d_nbits_all = (int*)backend::dev_alloc((size_t)S * nsb * sizeof(int));
    d_status_all = (int*)backend::dev_alloc((size_t)S * nsb * sizeof(int));
    d_items = (backend::GatherItem*)backend::dev_alloc((size_t)S * nsb * sizeof(backend::GatherItem));
    { int si = 0; for (auto& s : st) { s.sb_nbits = d_nbits_all + (size_t)si * nsb; s.sb_status = d_status_all + (size_t)si * nsb; si++; } }
    const int cw = p.width / 4, chh = p.height / 4;
    for (auto& s : st) {
      s.orig.alloc(p.width, p.height, 0);
      s.rec.alloc(p.width, p.height, 0);
      s.tmp.alloc(p.width, p.height, 0);
      s.ring.resize(ring_size);
      for (auto& r : s.ring) r.alloc(p.width, p.height, kPadY);
      if (p.interp_ref) s.interp.alloc(p.width, p.height, kPadY);
      if (p.interp_ref && !external_interp) {
        const int mn = p.width < p.height ? p.width : p.height;
        int lv = (int)(log10((double)mn) / log10(2.0) - 4.0);  // temporal_interp.c:913, evaluated in double as written
        if (lv > idev::kMaxLevels) lv = idev::kMaxLevels;
        if (lv < 1) { fprintf(stderr, "Run-time error...\nthor_hip: frame too small for interp_ref\n...now exiting to system...\n"); abort(); }
        s.ip_levels = lv;
        for (int l = 0; l < lv; l++) {
          const int lw = p.width >> l, lh = p.height >> l;
          const int bw = idev::kStep * ((lw + idev::kBbs - 1) / idev::kBbs), bh = idev::kStep * ((lh + idev::kBbs - 1) / idev::kBbs);
          const size_t n = (size_t)bw * bh + bw + 2;
          for (int k = 0; k < 5; k++) s.ip_mv[l][k] = (idev::imv*)backend::dev_alloc(n * sizeof(idev::imv));
          s.ip_prog[l] = (int*)backend::dev_alloc((size_t)(bh / idev::kStep + 1) * sizeof(int));
          if (l > 0) {
            s.ip_stride[l] = (lw + 64 + 15) & ~15;
            for (int k = 0; k < 2; k++) s.ip_pic[k][l] = (PIX*)backend::dev_alloc(((size_t)(lh + 64) * s.ip_stride[l] + 64) * sizeof(PIX));
          }
        }
      }
      s.cells = (DbCell*)backend::dev_alloc((size_t)cw * chh * sizeof(DbCell));
      backend::dev_memset(s.cells, 0, (size_t)cw * chh * sizeof(DbCell));
      s.sb_bits = (uint32_t*)backend::dev_alloc((size_t)nsb * sb_words * 4);
      s.scratch = (uint8_t*)backend::dev_alloc(ws_bytes * max_diag);
      const int nfb = nfb_h * nfb_v;
      s.cdef_dir = (int8_t*)backend::dev_alloc((size_t)(p.width / 8) * (p.height / 8));
      s.cdef_var = (int*)backend::dev_alloc((size_t)(p.width / 8) * (p.height / 8) * sizeof(int));
      s.cdef_fbc = (int*)backend::dev_alloc(nfb * sizeof(int));
      s.cdef_mse = (unsigned long long*)backend::dev_alloc((size_t)2 * nfb * kCdefMaxStr * 8);
      s.cdef_sel = (int*)backend::dev_alloc(nfb * sizeof(int));
      s.cdef_fbsel = (int*)backend::dev_alloc(nfb * sizeof(int));
      s.cdef_res = (CdefResult*)backend::dev_alloc(sizeof(CdefResult));
      s.cdef_tot = (unsigned long long*)backend::dev_alloc(((size_t)kCdefMaxStr * kCdefMaxStr + nfb) * 8);
      if (p.clpf) {
        s.clpf_stats = (uint32_t*)backend::dev_alloc(clpf_stat_words() * 4);
        s.clpf_fb_on = (uint8_t*)backend::dev_alloc((size_t)((p.width + 31) / 32) * ((p.height + 31) / 32));
      }
      if (!raw_frames) write_sequence_header(s.bits, sp);
      s.sh_bits = s.bits.nbits;
    }
    d_ljobs = (ClpfJob<PIX>*)backend::dev_alloc(sizeof(ClpfJob<PIX>) * S);
    h_ljobs.resize(S);
    d_jobs = (FrameJob<PIX>*)backend::dev_alloc(sizeof(FrameJob<PIX>) * S);
    h_jobs.resize(S);
    d_cjobs = (CdefJob<PIX>*)backend::dev_alloc(sizeof(CdefJob<PIX>) * S);
    h_cjobs.resize(S);
    d_prof = (long long*)backend::dev_alloc(32 * sizeof(long long));
    d_stats = (unsigned long long*)backend::dev_alloc(8 * sizeof(unsigned long long));
    backend::dev_memset(d_stats, 0, 8 * sizeof(unsigned long long));
    if (p.interp_ref && !external_interp) { d_ijobs = (idev::Job<PIX>*)backend::dev_alloc(sizeof(idev::Job<PIX>) * S); h_ijobs.resize(S); }
    if (depth_shift() > 0) d_packed = backend::dev_alloc(frame_bytes());
  }
  size_t clpf_stat_words() const { return 4 * ((size_t)(sp.width / 8) * (sp.height / 8) + 2 * (size_t)(sp.width / 16) * (sp.height / 16)); }
  void close() {
    for (auto& s : st) {
      backend::dev_free(s.rc_half[0]); backend::dev_free(s.rc_half[1]);
      backend::dev_free(s.clpf_stats); backend::dev_free(s.clpf_fb_on);
      s.orig.release(); s.rec.release(); s.tmp.release(); s.interp.release();
      backend::dev_free(s.cdef_dir); backend::dev_free(s.cdef_var); backend::dev_free(s.cdef_fbc); backend::dev_free(s.cdef_mse);
      backend::dev_free(s.cdef_sel); backend::dev_free(s.cdef_fbsel); backend::dev_free(s.cdef_res); backend::dev_free(s.cdef_tot);
      for (auto& r : s.ring) r.release();
      backend::dev_free(s.cells); backend::dev_free(s.sb_bits); backend::dev_free(s.scratch);
      for (int l = 0; l < idev::kMaxLevels; l++) {
        for (int k = 0; k < 5; k++) backend::dev_free(s.ip_mv[l][k]);
        backend::dev_free(s.ip_prog[l]); backend::dev_free(s.ip_pic[0][l]); backend::dev_free(s.ip_pic[1][l]);
      }
    }
    st.clear();
    backend::dev_free(d_nbits_all); backend::dev_free(d_status_all); backend::dev_free(d_items); backend::dev_free(d_payload);
    d_nbits_all = d_status_all = nullptr; d_items = nullptr; d_payload = nullptr; payload_words = 0;
    backend::release_superblocks(d_jobs);
    backend::dev_free(d_jobs); d_jobs = nullptr;
    backend::dev_free(d_cjobs); d_cjobs = nullptr;
    backend::dev_free(d_ljobs); d_ljobs = nullptr;
    backend::dev_free(d_prof); d_prof = nullptr;
    backend::dev_free(d_stats); d_stats = nullptr;
    backend::dev_free(d_ijobs); d_ijobs = nullptr;
    backend::dev_free(d_sse); d_sse = nullptr;
    backend::dev_free(d_packed); d_packed = nullptr;
    backend::dev_free(d_layout); d_layout = nullptr; d_layout_bytes = 0;
    backend::dev_free(d_scale); d_scale = nullptr; scale_dirty = true;
    backend::dev_free(d_rcjobs); d_rcjobs = nullptr;
    backend::dev_free(d_rcsums); d_rcsums = nullptr;
    backend::dev_free(d_scjob); d_scjob = nullptr;
    backend::dev_free(d_scsums); d_scsums = nullptr;
    backend::dev_free(d_tfjobs); d_tfjobs = nullptr;
    backend::dev_free(d_tfblk); d_tfblk = nullptr; tf_cap = 0;
  }

  // A packed frame of input-depth samples in device memory -> planes at the engine's depth (v << shift), and back (rounded and saturated).  Only with
  // input_bitdepth < bitdepth, which implies 16-bit planes.  Asynchronous on the device: ordered with the engine's other work.
  void widen(const void* packed, const Plane3<PIX>& dst) {
    if constexpr (sizeof(PIX) == 2) {
#if TK_HOST
      if (sp.input_bitdepth == 8) depth_up_rows((const uint8_t*)packed, dst, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
      else depth_up_rows((const uint16_t*)packed, dst, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
#else
      launch_depth_up(packed, dst, sp.width, sp.height, sp.bitdepth, sp.input_bitdepth);
#endif
    }
  }
  void narrow(const Plane3<PIX>& src, void* packed) {
    if constexpr (sizeof(PIX) == 2) {
#if TK_HOST
      if (sp.input_bitdepth == 8) depth_down_rows(src, (uint8_t*)packed, sp.width, sp.height, depth_shift(), sp.input_bitdepth, 0, 1, 0, 1);
      else depth_down_rows(src, (uint16_t*)packed, sp.width, sp.height, depth_shift(), sp.input_bitdepth, 0, 1, 0, 1);
#else
      launch_depth_down(src, packed, sp.width, sp.height, sp.bitdepth, sp.input_bitdepth);
#endif
    }
  }

  // A frame in a caller's layout (tk_filters.h: PixLayout; input-depth samples) in device memory -> planes at the engine's depth, and planes -> such a
  // frame: one kernel, no intermediate frame.  Asynchronous on the device: ordered with the engine's other work.
  void layout_in(const void* frame, const PixLayout& L, const Plane3<PIX>& dst) {
#if TK_HOST
    if constexpr (sizeof(PIX) == 1) layout_in_rows<uint8_t, PIX>(frame, L, dst, sp.width, sp.height, 0, 0, 1, 0, 1);
    else if (sp.input_bitdepth == 8) layout_in_rows<uint8_t, PIX>(frame, L, dst, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
    else layout_in_rows<uint16_t, PIX>(frame, L, dst, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
#else
    launch_layout_in<PIX>(frame, L, dst, sp.width, sp.height, sp.bitdepth, sp.input_bitdepth);
#endif
  }
  void layout_out(const Plane3<PIX>& src, void* frame, const PixLayout& L) {
#if TK_HOST
    if constexpr (sizeof(PIX) == 1) layout_out_rows<PIX, uint8_t>(src, frame, L, sp.width, sp.height, 0, sp.input_bitdepth, 0, 1, 0, 1);
    else if (sp.input_bitdepth == 8) layout_out_rows<PIX, uint8_t>(src, frame, L, sp.width, sp.height, depth_shift(), sp.input_bitdepth, 0, 1, 0, 1);
    else layout_out_rows<PIX, uint16_t>(src, frame, L, sp.width, sp.height, depth_shift(), sp.input_bitdepth, 0, 1, 0, 1);
#else
    launch_layout_out<PIX>(src, frame, L, sp.width, sp.height, sp.bitdepth, sp.input_bitdepth);
#endif
  }
  // The caller's description of a layout against this engine's pictures; false: refused (needs no device).
  bool resolve(int chroma, int msb_aligned, long long pitch_y, long long pitch_c, size_t off_u, size_t off_v, PixLayout& L) const {
    return resolve_layout(chroma, msb_aligned, pitch_y, pitch_c, off_u, off_v, sp.width, sp.height, sp.input_bitdepth, L);
  }
  // The same for a frame in host memory: its bytes travel once, as they are, into a device buffer (allocated on first use, grown when a larger layout
  // comes) and the same kernel runs.  Synchronous like upload_orig / download_rec.
  void* layout_buf(size_t bytes) {
    if (bytes > d_layout_bytes) { backend::dev_sync(); backend::dev_free(d_layout); d_layout = backend::dev_alloc(bytes); d_layout_bytes = bytes; }
    return d_layout;
  }
  void stage_layout_host(const void* frame, const PixLayout& L, const Plane3<PIX>& dst) {
    backend::h2d(layout_buf(L.bytes), frame, L.bytes);
    layout_in(d_layout, L, dst);
    backend::dev_sync();
  }
  // Only the picture's bytes of `frame` are written: a tight layout arrives with one copy; with a pitch or gaps the rows are cut out of a host copy
  // of the device buffer, as download_rec cuts them out of padded planes.
  void fetch_layout_host(const Plane3<PIX>& src, void* frame, const PixLayout& L) {
    layout_out(src, layout_buf(L.bytes), L);
    if (L.bytes == frame_bytes()) { backend::d2h(frame, d_layout, L.bytes); return; }
    std::vector<uint8_t> tmp(L.bytes);
    backend::d2h(tmp.data(), d_layout, L.bytes);
    const size_t B = sp.input_bitdepth > 8 ? 2 : 1, row_y = sp.width * B, row_c = L.chroma == 0 ? row_y / 2 : row_y;
    uint8_t* out = (uint8_t*)frame;
    for (int i = 0; i < sp.height; i++) memcpy(out + i * L.pitch_y, &tmp[i * L.pitch_y], row_y);
    for (int i = 0; i < sp.height / 2; i++) {
      memcpy(out + L.off_u + i * L.pitch_c, &tmp[L.off_u + i * L.pitch_c], row_c);
      if (L.chroma == 0) memcpy(out + L.off_v + i * L.pitch_c, &tmp[L.off_v + i * L.pitch_c], row_c);
    }
  }

  // An RGB frame (tk_filters.h: RgbFormat) in device memory -> planes at the engine's depth, and planes -> such a frame: colour conversion, 4:2:0
  // downsampling and depth conversion in one kernel.  Asynchronous on the device.
  void rgb_in(const void* frame, const RgbFormat& R, const Plane3<PIX>& dst) {
#if TK_HOST
    if (R.sbytes == 1) rgb_in_rows<uint8_t, PIX>(frame, R, dst, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
    else rgb_in_rows<uint16_t, PIX>(frame, R, dst, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
#else
    launch_rgb_in<PIX>(frame, R, dst, sp.width, sp.height, sp.bitdepth, sp.input_bitdepth);
#endif
  }
  void rgb_out(const Plane3<PIX>& src, void* frame, const RgbFormat& R) {
#if TK_HOST
    if (R.sbytes == 1) rgb_out_rows<PIX, uint8_t>(src, frame, R, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
    else rgb_out_rows<PIX, uint16_t>(src, frame, R, sp.width, sp.height, depth_shift(), 0, 1, 0, 1);
#else
    launch_rgb_out<PIX>(src, frame, R, sp.width, sp.height, sp.bitdepth, sp.input_bitdepth);
#endif
  }
  // The same for a frame in host memory, through the device buffer of the layouts (layout_buf).  Synchronous.
  void stage_rgb_host(const void* frame, const RgbFormat& R, const Plane3<PIX>& dst) {
    backend::h2d(layout_buf(R.bytes), frame, R.bytes);
    rgb_in(d_layout, R, dst);
    backend::dev_sync();
  }
  // Only the picture's bytes of `frame` are written, as in fetch_layout_host.
  void fetch_rgb_host(const Plane3<PIX>& src, void* frame, const RgbFormat& R) {
    rgb_out(src, layout_buf(R.bytes), R);
    const size_t row = (size_t)sp.width * R.sbytes * (R.kind == 0 ? 4 : R.kind == 1 ? 3 : 1);
    if (R.pitch == row && (R.kind != 2 || R.plane == row * sp.height)) { backend::d2h(frame, d_layout, R.bytes); return; }
    std::vector<uint8_t> tmp(R.bytes);
    backend::d2h(tmp.data(), d_layout, R.bytes);
    for (int k = 0; k < (R.kind == 2 ? 3 : 1); k++)
      for (int i = 0; i < sp.height; i++) memcpy((uint8_t*)frame + k * R.plane + i * R.pitch, &tmp[k * R.plane + i * R.pitch], row);
  }

  // A frame of another size (tk_scale.h): resolve_scaled checks the caller's description against this engine's pictures and keeps the plan - its
  // tables are rebuilt only when the source size, the filter or the site changed, and travel to the device only then.  false: refused, nothing
  // changed on the device.  scale_in then resamples a frame in device memory into planes at the engine's depth (asynchronous on the device).
  bool resolve_scaled(int src_w, int src_h, int filter, int site, int chroma, int msb_aligned, long long pitch_y, long long pitch_c, size_t off_u, size_t off_v) {
    bool rebuilt = false;
    const bool ok = resolve_scale(src_w, src_h, filter, site, chroma, msb_aligned, pitch_y, pitch_c, off_u, off_v, sp.width, sp.height, sp.input_bitdepth, scale_plan, &rebuilt);
    if (rebuilt || !ok) scale_dirty = true;
    return ok;
  }
  void scale_in(const void* frame, const Plane3<PIX>& dst) {
    const ScalePlan& P = scale_plan;
#if TK_HOST
    const ScaleTables tab = P.host_tables();
    if (sp.input_bitdepth == 8) scale_in_host<uint8_t, PIX>(frame, P.L, tab, dst, P.src_w, sp.width, sp.height, sp.input_bitdepth, depth_shift(), 1, 1);
    else if constexpr (sizeof(PIX) == 2) scale_in_host<uint16_t, PIX>(frame, P.L, tab, dst, P.src_w, sp.width, sp.height, sp.input_bitdepth, depth_shift(), 1, 1);
#else
    if (scale_dirty) {  // the device copy of the most recent plan
      std::vector<uint8_t> h(P.blob_bytes());
      backend::dev_sync();
      backend::dev_free(d_scale);
      d_scale = backend::dev_alloc(h.size());
      scale_tab = P.pack(h.data(), (const uint8_t*)d_scale);
      backend::h2d(d_scale, h.data(), h.size());
      scale_dirty = false;
    }
    launch_scale_in<PIX>(frame, P.L, scale_tab, P.t[1].span > P.t[3].span ? P.t[1].span : P.t[3].span, dst, P.src_w, sp.width, sp.height, sp.bitdepth, sp.input_bitdepth);
#endif
  }
  // The same for a frame in host memory, through the device buffer of the layouts (layout_buf).  Synchronous.
  void stage_scaled_host(const void* frame, const Plane3<PIX>& dst) {
    backend::h2d(layout_buf(scale_plan.L.bytes), frame, scale_plan.L.bytes);
    scale_in(d_layout, dst);
    backend::dev_sync();
  }

  // planar 4:2:0 frame of input-depth samples in host memory -> device `orig` of stream s
  void upload_orig(int s, const void* yuv_in) {
    if (depth_shift() > 0) {  // the narrow frame travels; the device widens it
      backend::h2d(d_packed, yuv_in, frame_bytes());
      widen(d_packed, st[s].orig.p);
      return;
    }
    const PIX* yuv = (const PIX*)yuv_in;
    const int w = sp.width, h = sp.height;
    std::vector<PIX> tmp;
    DevFrame<PIX>& f = st[s].orig;
    if (f.p.sy == w) backend::h2d(f.p.y, yuv, (size_t)w * h * sizeof(PIX));
    else { tmp.assign((size_t)f.p.sy * h, 0); for (int i = 0; i < h; i++) memcpy(&tmp[(size_t)i * f.p.sy], yuv + (size_t)i * w, w * sizeof(PIX)); backend::h2d(f.p.y, tmp.data(), tmp.size() * sizeof(PIX)); }
    const PIX* cu = yuv + (size_t)w * h; const PIX* cv = cu + (size_t)(w / 2) * (h / 2);
    if (f.p.sc == w / 2) { backend::h2d(f.p.u, cu, (size_t)(w / 2) * (h / 2) * sizeof(PIX)); backend::h2d(f.p.v, cv, (size_t)(w / 2) * (h / 2) * sizeof(PIX)); }
    else {
      tmp.assign((size_t)f.p.sc * (h / 2), 0);
      for (int i = 0; i < h / 2; i++) memcpy(&tmp[(size_t)i * f.p.sc], cu + (size_t)i * (w / 2), (w / 2) * sizeof(PIX));
      backend::h2d(f.p.u, tmp.data(), tmp.size() * sizeof(PIX));
      for (int i = 0; i < h / 2; i++) memcpy(&tmp[(size_t)i * f.p.sc], cv + (size_t)i * (w / 2), (w / 2) * sizeof(PIX));
      backend::h2d(f.p.v, tmp.data(), tmp.size() * sizeof(PIX));
    }
  }
  // planes with arbitrary host strides (drop-in path)
  void upload_planes(int s, const PIX* y, int sy, const PIX* u, const PIX* v, int sc) {
    const int w = sp.width, h = sp.height;
    DevFrame<PIX>& f = st[s].orig;
    std::vector<PIX> tmp((size_t)f.p.sy * h);
    for (int i = 0; i < h; i++) memcpy(&tmp[(size_t)i * f.p.sy], y + (size_t)i * sy, w * sizeof(PIX));
    backend::h2d(f.p.y, tmp.data(), tmp.size() * sizeof(PIX));
    tmp.assign((size_t)f.p.sc * (h / 2), 0);
    for (int i = 0; i < h / 2; i++) memcpy(&tmp[(size_t)i * f.p.sc], u + (size_t)i * sc, (w / 2) * sizeof(PIX));
    backend::h2d(f.p.u, tmp.data(), tmp.size() * sizeof(PIX));
    for (int i = 0; i < h / 2; i++) memcpy(&tmp[(size_t)i * f.p.sc], v + (size_t)i * sc, (w / 2) * sizeof(PIX));
    backend::h2d(f.p.v, tmp.data(), tmp.size() * sizeof(PIX));
  }
  // reconstruction of stream s -> planar 4:2:0 frame of input-depth samples in host memory (what the reference writes with -rf)
  void download_rec(int s, void* yuv_out) {
    if (depth_shift() > 0) {
      narrow(st[s].rec.p, d_packed);
      backend::d2h(yuv_out, d_packed, frame_bytes());
      return;
    }
    PIX* yuv = (PIX*)yuv_out;
    const int w = sp.width, h = sp.height;
    DevFrame<PIX>& f = st[s].rec;
    std::vector<PIX> tmp((size_t)f.p.sy * h);
    backend::d2h(tmp.data(), f.p.y, tmp.size() * sizeof(PIX));
    for (int i = 0; i < h; i++) memcpy(yuv + (size_t)i * w, &tmp[(size_t)i * f.p.sy], w * sizeof(PIX));
    PIX* cu = yuv + (size_t)w * h; PIX* cv = cu + (size_t)(w / 2) * (h / 2);
    tmp.resize((size_t)f.p.sc * (h / 2));
    backend::d2h(tmp.data(), f.p.u, tmp.size() * sizeof(PIX));
    for (int i = 0; i < h / 2; i++) memcpy(cu + (size_t)i * (w / 2), &tmp[(size_t)i * f.p.sc], (w / 2) * sizeof(PIX));
    backend::d2h(tmp.data(), f.p.v, tmp.size() * sizeof(PIX));
    for (int i = 0; i < h / 2; i++) memcpy(cv + (size_t)i * (w / 2), &tmp[(size_t)i * f.p.sc], (w / 2) * sizeof(PIX));
  }

  // The frame's per-4x4 block data (DbCell, tk_common.h) as the block decisions and the in-loop filters left it: what the
  // reference keeps in encoder_info->deblock_data[] (written by copy_deblock_data, enc/encode_block.c:1568-1613).
  size_t num_cells() const { return (size_t)(sp.width / 4) * (sp.height / 4); }
  void download_cells(int s, DbCell* out) { backend::d2h(out, st[s].cells, num_cells() * sizeof(DbCell)); }

  // Coding-order schedule.  begin_sequence fixes the chunk [skip, skip+num_frames) of an input holding
  // file_frames frames (needed for the reference's end-of-sequence behaviour with reordered GOPs).
  void begin_sequence(int s, int skip, int num_frames, int file_frames) {
    st[s].gop.init(sp, skip, num_frames, file_frames); st[s].log.clear();
    if (st[s].rc.on()) set_rate_control(s, st[s].rc);   // the target stays, the controller starts again
    if (st[s].sc.on()) st[s].rc_prev = false;           // the scene-cut setting stays too; the next analysis has no previous frame
  }
  bool low_delay() const { return sp.num_reorder_pics == 0; }
  // Scene cuts of stream s from its next frame on (c.on() false: off); legal where set_rate_control is - the caller checks, and that the stream is low delay.
  void set_scene_cut(int s, const ScConfig& c) {
    st[s].sc = c;
    st[s].rc_prev = false;
  }
  // A key frame at chunk-relative frame idx of the low-delay stream s.  pending: st[s].cur is scheduled and not coded yet.  0; 1: idx is outside the
  // chunk or coded already, or the set is full.
  int force_key_frame(int s, int idx, bool pending) {
    Stream<PIX>& q = st[s];
    if (!q.gop.started) q.gop.init(sp, 0, 1 << 28, 1 << 28);
    if (idx < 0 || idx >= q.gop.num_frames) return 1;
    if (pending && q.cur.frame_num == idx) {
      if (q.cur.frame_type != F_I) q.gop.promote(q.cur, KEY_FORCED);
      return 0;
    }
    if (idx < q.gop.num_encoded + (pending ? 1 : 0)) return 1;   // low delay: the coded index is the frame number
    return q.gop.request_key(idx) ? 0 : 1;
  }
  // The analysis (tk_rc.h) of the original `cur` against the original `prev` (nullptr: none, inter = intra) as a call of its own: k_rc_cost's second
  // instantiation halves the previous original itself, so neither a stream's half planes nor its controller are touched.
  void scene_cost(const DevFrame<PIX>& cur, const DevFrame<PIX>* prev, unsigned long long sums[3]) {
    if (!d_scsums) {
      d_scsums = (unsigned long long*)backend::dev_alloc(4 * sizeof(unsigned long long));
      d_scjob = (RcJob<PIX>*)backend::dev_alloc(sizeof(RcJob<PIX>));
    }
    RcJob<PIX> J;
    J.y = cur.p.y; J.sy = cur.p.sy; J.hw = sp.width / 2; J.hh = sp.height / 2;
    J.cur = nullptr; J.prev = nullptr;
    J.prev_y = prev ? prev->p.y : nullptr; J.prev_sy = prev ? prev->p.sy : 0;
    J.out = d_scsums;
    backend::dev_memset(d_scsums, 0, 4 * sizeof(unsigned long long));
#if TK_HOST
    rc_cost_frame(J, true);
#else
    backend::h2d(d_scjob, &J, sizeof(J));
    launch_rc_cost_orig<PIX>(d_scjob, &J, 1);
#endif
    backend::dev_sync();
    backend::d2h(sums, d_scsums, 3 * sizeof(unsigned long long));
  }
  // The temporal filter (tk_tf.h) of n requests in one launch sequence with one synchronisation: every `cur` against its neighbours into its `dst`, which
  // is none of the call's sources - the caller checks (tf_requests_ok).  Originals in, a pure function of them out; nothing of a stream's state is touched.
  struct TfItem {
    const DevFrame<PIX>* cur; const DevFrame<PIX>* dst;
    const DevFrame<PIX>* ref[TF_MAX_REFS];
    int dist[TF_MAX_REFS], nrefs;
  };
  // Per-block vectors and weights of the last filter_frames call, request i: TF_MAX_REFS * (width / 8) * (height / 8) records (the known-answer entry reads them).
  size_t tf_blocks_per_request() const { return (size_t)TF_MAX_REFS * (sp.width / TF_BLK) * (sp.height / TF_BLK); }
  void filter_frames(const TfItem* it, int n, int strength) {
    if (n > tf_cap) {
      backend::dev_free(d_tfjobs); backend::dev_free(d_tfblk);
      d_tfjobs = (TfJob<PIX>*)backend::dev_alloc((size_t)n * sizeof(TfJob<PIX>));
      d_tfblk = (TfBlock*)backend::dev_alloc((size_t)n * tf_blocks_per_request() * sizeof(TfBlock));
      tf_cap = n;
    }
    std::vector<TfJob<PIX>> hj(n);
    for (int i = 0; i < n; i++) {
      TfJob<PIX>& J = hj[i];
      J.cur = it[i].cur->p; J.dst = it[i].dst->p;
      for (int k = 0; k < TF_MAX_REFS; k++) {
        J.ref[k] = k < it[i].nrefs ? it[i].ref[k]->p : it[i].cur->p;
        J.dist[k] = k < it[i].nrefs ? it[i].dist[k] : 1;
      }
      J.nrefs = it[i].nrefs; J.width = sp.width; J.height = sp.height; J.strength = strength; J.sh = sp.bitdepth - 8;
      J.blk = d_tfblk + (size_t)i * tf_blocks_per_request();
    }
#if TK_HOST
    for (int i = 0; i < n; i++) tf_filter_frame(hj[i]);
#else
    backend::h2d(d_tfjobs, hj.data(), (size_t)n * sizeof(TfJob<PIX>));
    launch_tf<PIX>(d_tfjobs, hj.data(), n);
#endif
    backend::dev_sync();
  }
  // Rate control of stream s from its next frame on (tk_rc.h; c.on() false: off).  Legal while the stream's log is empty: before its first frame or right
  // after begin_sequence - the caller checks.  The controller starts empty and the next analysis has no previous frame.
  void set_rate_control(int s, const RcConfig& c) {
    Stream<PIX>& q = st[s];
    q.rc = c;
    if (q.rc.on() && q.rc.initial_qp == 0) q.rc.initial_qp = sp.qp;
    q.rcs.begin(q.rc, sp.frame_rate);
    q.rc_prev = false;
    q.rclog.clear();
  }
  // The base QP of the frames fp[s] of the rate-controlled streams in [first, first + count), origs in place: one analysis launch for all of them, the
  // three sums of each back to the host, the controller's decision, and the frame's QP from it by the rule the schedule gave the frame.
  // A stream with scene cuts on is analysed too, rate-controlled or not; per stream the order is analysis, cut decision and promotion (a P frame
  // becomes the I frame GopScheduler::promote makes), and only then the controller, which therefore sees a promoted frame as class 0.
  void rate_control(std::vector<FrameParams>& fp, int first, int count) {
    std::vector<RcJob<PIX>> hj;
    std::vector<int> who;
    const int hw = sp.width / 2, hh = sp.height / 2;
    if (!d_rcsums) {
      d_rcsums = (unsigned long long*)backend::dev_alloc((size_t)S * 4 * sizeof(unsigned long long));
      d_rcjobs = (RcJob<PIX>*)backend::dev_alloc((size_t)S * sizeof(RcJob<PIX>));
    }
    for (int s = first; s < first + count; s++) {
      Stream<PIX>& q = st[s];
      if (!q.rc.on() && !q.sc.on()) continue;
      for (int k = 0; k < 2; k++)
        if (!q.rc_half[k]) q.rc_half[k] = (PIX*)backend::dev_alloc((size_t)hw * hh * sizeof(PIX));
      RcJob<PIX> J;
      J.y = q.orig.p.y; J.sy = q.orig.p.sy; J.hw = hw; J.hh = hh;
      J.cur = q.rc_half[q.rc_flip]; J.prev = q.rc_prev ? q.rc_half[q.rc_flip ^ 1] : nullptr;
      J.out = d_rcsums + (size_t)s * 4;
      hj.push_back(J);
      who.push_back(s);
    }
    const int n = (int)who.size();
    backend::dev_memset(d_rcsums + (size_t)first * 4, 0, (size_t)count * 4 * sizeof(unsigned long long));
#if TK_HOST
    for (int k = 0; k < n; k++) rc_cost_frame(hj[k]);
#else
    backend::h2d(d_rcjobs, hj.data(), (size_t)n * sizeof(RcJob<PIX>));
    launch_rc_cost<PIX>(d_rcjobs, hj.data(), n);
#endif
    backend::dev_sync();
    std::vector<unsigned long long> sums((size_t)count * 4);
    backend::d2h(sums.data(), d_rcsums + (size_t)first * 4, sums.size() * sizeof(unsigned long long));
    for (int k = 0; k < n; k++) {
      const int s = who[k];
      Stream<PIX>& q = st[s];
      FrameParams& f = fp[s];
      const bool had_prev = q.rc_prev;
      q.rc_flip ^= 1;
      q.rc_prev = true;
      q.key_analysed = true;
      for (int j = 0; j < 3; j++) q.key_sums[j] = sums[(size_t)(s - first) * 4 + j];
      if (f.frame_type == F_P && q.gop.started && low_delay() && sc_is_cut(q.sc, had_prev, f.frame_num, q.gop.last_intra, q.key_sums[0], q.key_sums[1])) {
        q.gop.promote(f, KEY_SCENE_CUT);
        q.cur = f;
      }
      if (!q.rc.on()) continue;
      RcStat& r = q.rc_cur;
      r = RcStat();
      r.frame_class = rc_class(f.frame_type, f.b_level);
      r.qp_rule = f.qp_rule;
      r.sum_intra = sums[(size_t)(s - first) * 4]; r.sum_best = sums[(size_t)(s - first) * 4 + 1]; r.n_intra = sums[(size_t)(s - first) * 4 + 2];
      int fq[52];
      for (int b = 0; b < 52; b++) fq[b] = GopScheduler::rule_qp(sp, f.qp_rule, b);
      r.base_qp = rc_decide(q.rc, q.rcs, r.frame_class, (long long)(r.frame_class == 0 ? r.sum_intra : r.sum_best), fq);
      f.qp = fq[r.base_qp];
      q.cur.qp = f.qp;
    }
  }
  // Next frame to code for stream s: fills st[s].cur / st[s].cur_abs; false when the chunk is finished.
  bool schedule(int s) {
    Stream<PIX>& q = st[s];
    if (!q.gop.started) q.gop.init(sp, 0, 1 << 28, 1 << 28);
    return q.gop.next(q.cur, q.cur_abs, [&](int idx) { return q.ring[idx].frame_num; });
  }

  // Temporally interpolated reference (enc/mainenc.c:350-355, common/temporal_interp.c:909): built on the device from
  // the two window frames of every stream whose frame uses it (tk_interp_dev.h) - no frame leaves HBM.
  void make_interp_frames(const std::vector<FrameParams>& fp, int first, int count) {
    int n = 0;
    for (int s = first; s < first + count; s++) {
      if (!fp[s].interp_ref) continue;
      Stream<PIX>& q = st[s];
      const FrameParams& f = fp[s];
      idev::Job<PIX>& J = h_ijobs[n++];
      memset(&J, 0, sizeof(J));
      const int ratio = 2, k = 1;  // interpolate_frames(..., 2, 1): the frame half way between the two anchors (mainenc.c:353)
      J.levels = q.ip_levels;
      J.width = sp.width; J.height = sp.height;
      J.ref[0] = q.ring[f.interp_src[0]].p; J.ref[1] = q.ring[f.interp_src[1]].p; J.out = q.interp.p;
      const int reversed = k > ratio / 2;
      const int wt0 = reversed ? k : ratio - k, wt1 = ratio - wt0;
      for (int l = 0; l < J.levels; l++) {
        idev::Level<PIX>& L = J.lv[l];
        const int lw = sp.width >> l, lh = sp.height >> l;
        const PIX* in[2];
        int str[2];
        if (l == 0) { in[0] = J.ref[0].y; in[1] = J.ref[1].y; str[0] = J.ref[0].sy; str[1] = J.ref[1].sy; L.pad = kPadY; }
        else {
          for (int r = 0; r < 2; r++) { J.dpic[r][l] = q.ip_pic[r][l] + (size_t)32 * q.ip_stride[l] + 32; in[r] = J.dpic[r][l]; str[r] = q.ip_stride[l]; }
          J.dstride[l] = q.ip_stride[l];
          L.pad = 32;
        }
        L.pic[0] = reversed ? in[1] : in[0]; L.pic[1] = reversed ? in[0] : in[1];
        L.s[0] = reversed ? str[1] : str[0]; L.s[1] = reversed ? str[0] : str[1];
        L.w = lw; L.h = lh;
        L.mv[0] = q.ip_mv[l][0]; L.mv[1] = q.ip_mv[l][1]; L.nmv[0] = q.ip_mv[l][2]; L.nmv[1] = q.ip_mv[l][3]; L.gmv1 = q.ip_mv[l][4];
        L.guide_mv1 = l == J.levels - 1 ? nullptr : L.gmv1;
        L.guide_reversed = reversed; L.guide_wt0 = wt0;
        L.wt[0] = wt0; L.wt[1] = wt1; L.reversed = reversed;
        L.bw = idev::kStep * ((lw + idev::kBbs - 1) / idev::kBbs); L.bh = idev::kStep * ((lh + idev::kBbs - 1) / idev::kBbs);
        L.prog = q.ip_prog[l]; L.ticket = q.ip_prog[l] + L.bh / idev::kStep;
      }
      q.interp.frame_num = f.frame_num;
    }
    if (!n) return;
    backend::h2d(d_ijobs, h_ijobs.data(), sizeof(idev::Job<PIX>) * n);
    backend::run_interp<PIX>(d_ijobs, h_ijobs.data(), n);
  }

  // Encode one frame per stream (origs already uploaded). Appends to st[s].out.
  void encode_frames(std::vector<FrameParams>& fp) {
    prepare_jobs(fp, 0, S);
    backend::run_superblocks<PIX>(d_jobs, h_jobs.data(), S, nullptr);
    finish_frames(fp, 0, S);
  }

  // Anti-diagonals of the superblock grid (t = l + 2k): their number, and where a frame is cut in two for encode_run.
  int num_diags() const { return (sb_cols - 1) + 2 * (sb_rows - 1) + 1; }

  // Code the next `nframes` frames of every stream, the streams in TWO GROUPS HALF A FRAME APART (the first half of the streams leads):
  // one launch of the persistent superblock kernel carries the second half (anti-diagonals [Th, T)) of one group's frame - the narrowing end
  // of its dependency wavefront - together with the first half of the other group's frame, its widening start, so the workgroup slots one
  // group leaves idle are taken by the other (in lock step every stream ramps up and down at the same time: 13 % of the workgroup-time idle
  // at 3840x2160 x 128 streams, profiles/r04_sbtimes_4k_s128_final.log).  The run starts and ends on frame boundaries for every stream: the
  // first launch holds only the leading group's first half, the last one only the trailing group's second half.  Every superblock still
  // starts after its two dependencies and sees the same reference frames: results do not depend on the schedule.
  //   next(s): make stream s ready for its next frame - schedule() it and point st[s].orig at its input; false: no frame left (an error here)
  //   done(first, count): the frames of streams [first, first + count) are complete (bits appended, st[s].rec = the reconstruction,
  //                       st[s].cur = the frame) - called before any later launch touches those streams again
  template <class NextF, class DoneF> void encode_run(int nframes, NextF next, DoneF done) {
    std::vector<FrameParams> fp(S);
    auto prep = [&](int first, int count) {
      for (int s = first; s < first + count; s++) {
        if (!next(s)) { fprintf(stderr, "thor_hip: stream %d has no frame left to code\n", s); abort(); }
        fp[s] = st[s].cur;
      }
      prepare_jobs(fp, first, count);
    };
    if (S < 2 || num_diags() < 2) {   // nothing to stagger: frame by frame
      for (int f = 0; f < nframes; f++) {
        prep(0, S);
        backend::run_superblocks<PIX>(d_jobs, h_jobs.data(), S, nullptr);
        finish_frames(fp, 0, S);
        done(0, S);
      }
      return;
    }
    const int T = num_diags(), Th = (T + 1) / 2, S0 = S / 2, S1 = S - S0;
    std::vector<backend::SbRange> rg(S);
    auto set = [&](int first, int count, int lo, int hi) { for (int s = first; s < first + count; s++) { rg[s].lo = (unsigned short)lo; rg[s].hi = (unsigned short)hi; } };
    if (nframes < 1) return;
    prep(0, S0);
    set(0, S0, 0, Th); set(S0, S1, 0, 0);
    backend::run_superblocks<PIX>(d_jobs, h_jobs.data(), S, rg.data());
    for (int f = 0; f < nframes; f++) {
      prep(S0, S1);
      set(0, S0, Th, T); set(S0, S1, 0, Th);
      backend::run_superblocks<PIX>(d_jobs, h_jobs.data(), S, rg.data());
      finish_frames(fp, 0, S0);
      done(0, S0);
      if (f + 1 < nframes) { prep(0, S0); set(0, S0, 0, Th); } else set(0, S0, 0, 0);
      set(S0, S1, Th, T);
      backend::run_superblocks<PIX>(d_jobs, h_jobs.data(), S, rg.data());
      finish_frames(fp, S0, S1);
      done(S0, S1);
    }
  }

  // Frame jobs of streams [first, first + count) for the frames fp[s] (origs in place): interpolated references, FrameJob set-up, upload.
  // With rate control on for one of them the frames' QPs are chosen here (rate_control), which is why fp is not const.
  void prepare_jobs(std::vector<FrameParams>& fp, int first, int count) {
    for (int s = first; s < first + count; s++)
      if (st[s].rc.on() || st[s].sc.on()) { rate_control(fp, first, count); break; }
    if (!external_interp) make_interp_frames(fp, first, count);
    for (int s = first; s < first + count; s++) {
      Stream<PIX>& q = st[s];
      const FrameParams& f = fp[s];
      FrameJob<PIX>& J = h_jobs[s];
      memset(&J, 0, sizeof(J));
      EncCfg& c = J.cfg;
      c.width = sp.width; c.height = sp.height; c.bitdepth = sp.bitdepth;
      c.enable_tb_split = sp.enable_tb_split; c.enable_pb_split = sp.enable_pb_split; c.enable_bipred = sp.enable_bipred;
      c.encoder_speed = sp.encoder_speed; c.intra_rdo = sp.intra_rdo; c.use_block_contexts = sp.use_block_contexts;
      c.cfl_intra = sp.cfl_intra; c.cfl_inter = sp.cfl_inter; c.max_num_ref = sp.max_num_ref; c.interp_ref_cfg = sp.interp_ref;
      c.early_skip_thr = sp.early_skip_thr; c.sb_shift = kLog2MaxSb - sp.log2_sb_size;
      J.frame_type = f.frame_type; J.qp = f.qp; J.num_ref = f.num_ref; J.frame_num = f.frame_num;
      J.interp_ref = f.interp_ref; J.num_intra_modes = f.num_intra_modes;
      J.lambda = f.lambda_coeff * kSquaredLambdaQP[f.qp];
      J.sqrt_lambda = sqrt(J.lambda);
      J.orig = q.orig.p; J.rec = q.rec.p;
      for (int r = 0; r < f.num_ref; r++) {
        const DevFrame<PIX>& rf = f.ref_array[r] < 0 ? q.interp : q.ring[f.ref_array[r]];
        J.ref[r] = rf.p;
        J.sign[r] = rf.frame_num > f.frame_num;
        J.sign_ge[r] = rf.frame_num >= f.frame_num;
      }
      J.cells = q.cells; J.cell_stride = sp.width / 4;
      J.sb_cols = sb_cols; J.sb_rows = sb_rows;
      J.sb_bits = q.sb_bits; J.sb_words = sb_words; J.sb_nbits = q.sb_nbits; J.sb_status = q.sb_status;
      J.scratch = q.scratch; J.scratch_bytes = ws_bytes;
      J.prof = d_prof;
      J.stats = d_stats;
      if (f.frame_type == F_I) backend::dev_memset(q.cells, 0, (size_t)(sp.width / 4) * (sp.height / 4) * sizeof(DbCell));
    }
    backend::h2d(d_jobs + first, h_jobs.data() + first, sizeof(FrameJob<PIX>) * count);
  }

  // Everything after the superblocks of streams [first, first + count): in-loop filters, reference creation, bitstream assembly.
  void finish_frames(const std::vector<FrameParams>& fp, int first, int count) {
    const int end = first + count;
    if (sp.deblocking) backend::run_deblock<PIX>(d_jobs + first, h_jobs.data() + first, count);
    // CDEF (encode_frame.c:685-689 frame-level guesses, :768-783 search + filter)
    if (sp.cdef) {
      for (int s = first; s < end; s++) {
        Stream<PIX>& q = st[s];
        CdefJob<PIX>& C = h_cjobs[s];
        C.rec = q.rec.p; C.src = q.tmp.p; C.org = q.orig.p;
        C.width = sp.width; C.height = sp.height; C.bitdepth = sp.bitdepth;
        C.cells = q.cells; C.cs = sp.width / 4; C.nfb_h = nfb_h; C.nfb_v = nfb_v;
        C.speed = sp.cdef - 1; C.damping = 5;
        C.cdef_bits = fp[s].frame_type == F_I ? 3 : 3 - (fp[s].qp + 4) / 16;
        if (C.speed == 3) C.cdef_bits = 0;
        C.qp = fp[s].qp;
        C.dir = q.cdef_dir; C.var = q.cdef_var; C.fb_compact = q.cdef_fbc; C.mse = q.cdef_mse; C.sel = q.cdef_sel;
        C.fb_sel = q.cdef_fbsel; C.res = q.cdef_res; C.tot = q.cdef_tot;
      }
      backend::h2d(d_cjobs + first, h_cjobs.data() + first, sizeof(CdefJob<PIX>) * count);
      backend::run_cdef<PIX>(d_cjobs + first, h_cjobs.data() + first, count);
    }
    // CLPF (encode_frame.c:785-817): statistics on the device, frame-level plan on the host, filter on the device
    std::vector<ClpfPlan> lplan(sp.clpf ? S : 0);
    if (sp.clpf) {
      bool any = false;
      for (int s = first; s < end; s++) {
        Stream<PIX>& q = st[s];
        ClpfJob<PIX>& L = h_ljobs[s];
        L.rec = q.rec.p; L.src = q.tmp.p; L.org = q.orig.p;
        L.width = sp.width; L.height = sp.height; L.bitdepth = sp.bitdepth; L.qp = fp[s].qp;
        L.cells = q.cells; L.cs = sp.width / 4; L.stats = q.clpf_stats;
        L.strength[0] = L.strength[1] = L.strength[2] = 0; L.fb_log2 = 7; L.fb_on = q.clpf_fb_on;
        any = any || fp[s].qp > 16;
      }
      if (any) {
        backend::h2d(d_ljobs + first, h_ljobs.data() + first, sizeof(ClpfJob<PIX>) * count);
        backend::run_clpf_stats<PIX>(d_ljobs + first, h_ljobs.data() + first, count);
        backend::dev_sync();
        std::vector<uint32_t> hst(clpf_stat_words());
        bool filt = false;
        for (int s = first; s < end; s++) {
          if (fp[s].qp > 16) backend::d2h(hst.data(), st[s].clpf_stats, hst.size() * 4);
          lplan[s] = clpf_plan(hst.data(), sp.width, sp.height, fp[s].qp, h_jobs[s].lambda, sp.max_clpf_strength);
          ClpfJob<PIX>& L = h_ljobs[s];
          for (int k = 0; k < 3; k++) { L.strength[k] = lplan[s].strength[k]; filt = filt || L.strength[k]; }
          L.fb_log2 = lplan[s].fb_log2;
          if (!lplan[s].fb_on.empty()) backend::h2d(st[s].clpf_fb_on, lplan[s].fb_on.data(), lplan[s].fb_on.size());
        }
        if (filt) {
          backend::h2d(d_ljobs + first, h_ljobs.data() + first, sizeof(ClpfJob<PIX>) * count);
          backend::run_clpf_apply<PIX>(d_ljobs + first, h_ljobs.data() + first, count);
        }
      } else
        for (int s = first; s < end; s++) lplan[s] = clpf_plan(nullptr, sp.width, sp.height, fp[s].qp, h_jobs[s].lambda, sp.max_clpf_strength);
    }
    // the frame's record (mainenc.c:553-591); the frame numbers of its references are read before the window moves
    for (int s = first; s < end; s++) {
      Stream<PIX>& q = st[s];
      const FrameParams& f = fp[s];
      FrameStat r;
      r.display = f.frame_num + (q.gop.started ? q.gop.skip : 0);
      r.frame_type = f.frame_type; r.qp = f.qp; r.num_ref = f.num_ref;
      for (int k = 0; k < kMaxRefs; k++) {
        r.ref_array[k] = f.ref_array[k];
        r.ref_frame_num[k] = f.ref_array[k] >= 0 && f.ref_array[k] < ring_size ? q.ring[f.ref_array[k]].frame_num : -1;
      }
      r.num_bits = -q.bits.nbits;  // completed below, when the frame's bits are assembled
      r.key_reason = f.key_reason;
      if (q.key_analysed) {
        for (int k = 0; k < 3; k++) r.key_sums[k] = q.key_sums[k];
        q.key_analysed = false;
      }
      q.log.push_back(r);
    }
    // sliding window: the slot shifted out becomes ref[0] (encode_frame.c:826-835)
    std::vector<Plane3<PIX>> dst(S);
    for (int s = first; s < end; s++) {
      Stream<PIX>& q = st[s];
      DevFrame<PIX> last = q.ring.back();
      for (int r = ring_size - 1; r > 0; r--) q.ring[r] = q.ring[r - 1];
      q.ring[0] = last;
      q.ring[0].frame_num = fp[s].frame_num;
      dst[s] = q.ring[0].p;
    }
    backend::run_make_ref<PIX>(h_jobs.data() + first, dst.data() + first, count);
    if (frame_distortion) {  // per-plane SSE of the final reconstructions (after deblocking, CDEF, CLPF)
      if (!d_sse) d_sse = (unsigned long long*)backend::dev_alloc((size_t)S * 4 * sizeof(unsigned long long));
      backend::dev_memset(d_sse + (size_t)first * 4, 0, (size_t)count * 4 * sizeof(unsigned long long));
      bool at_input_depth = false;  // input_bitdepth < bitdepth: the sums snr_yuv forms, both frames rounded back to the input depth
      if constexpr (sizeof(PIX) == 2) {
        if (depth_shift() > 0) {
          at_input_depth = true;
#if TK_HOST
          for (int s = first; s < end; s++)
            frame_sse_depth_rows(h_jobs[s].orig, h_jobs[s].rec, sp.width, sp.height, depth_shift(), sp.input_bitdepth, 0, 1, 0, 1, d_sse + (size_t)s * 4);
#else
          launch_frame_sse_depth(d_jobs + first, h_jobs.data() + first, count, sp.bitdepth, sp.input_bitdepth, d_sse + (size_t)first * 4);
#endif
        }
      }
      if (!at_input_depth) {
#if TK_HOST
        for (int s = first; s < end; s++) frame_sse_rows(h_jobs[s].orig, h_jobs[s].rec, sp.width, sp.height, 0, 1, 0, 1, d_sse + (size_t)s * 4);
#else
        launch_frame_sse<PIX>(d_jobs + first, h_jobs.data() + first, count, d_sse + (size_t)first * 4);
#endif
      }
    }
    backend::dev_sync();
    if (frame_distortion) {
      std::vector<unsigned long long> sse((size_t)count * 4);
      backend::d2h(sse.data(), d_sse + (size_t)first * 4, sse.size() * sizeof(unsigned long long));
      for (int s = first; s < end; s++) {
        FrameStat& r = st[s].log.back();
        r.has_sse = 1;
        for (int k = 0; k < 3; k++) r.sse[k] = sse[(size_t)(s - first) * 4 + k];
      }
    }
    // bitstream assembly: one D2H of all bit counts, a device-side bit-level gather of the per-SB
    // strings into one compact buffer, one D2H of that buffer.
    // (arrays indexed by stream: only the entries of [first, end) are filled and used)
    std::vector<int> nb((size_t)S * nsb), stt((size_t)S * nsb);
    backend::d2h(nb.data() + (size_t)first * nsb, d_nbits_all + (size_t)first * nsb, (size_t)count * nsb * sizeof(int));
    backend::d2h(stt.data() + (size_t)first * nsb, d_status_all + (size_t)first * nsb, (size_t)count * nsb * sizeof(int));
    std::vector<backend::GatherItem> items((size_t)S * nsb);
    std::vector<long long> stream_off(S + 1, 0);
    {
      long long pos = 0;
      for (int s = first; s < end; s++) {
        stream_off[s] = pos;
        for (int i = 0; i < nsb; i++) {
          if (stt[(size_t)s * nsb + i]) { fprintf(stderr, "Run-time error...\nthor_hip: superblock %d bit buffer overflow\n...now exiting to system...\n", i); abort(); }
          backend::GatherItem& g = items[(size_t)s * nsb + i];
          g.src = st[s].sb_bits + (size_t)i * sb_words; g.nbits = nb[(size_t)s * nsb + i]; g.dst_bit = pos;
          pos += g.nbits;
        }
        pos = (pos + 31) & ~31ll;  // streams start word aligned
      }
      stream_off[end] = pos;
    }
    const size_t need_words = (size_t)(stream_off[end] >> 5) + 2;
    if (need_words > payload_words) {
      backend::dev_free(d_payload);
      payload_words = need_words + need_words / 2;
      d_payload = (uint32_t*)backend::dev_alloc(payload_words * 4);
    }
    backend::dev_memset(d_payload, 0, need_words * 4);
    backend::h2d(d_items + (size_t)first * nsb, items.data() + (size_t)first * nsb, (size_t)count * nsb * sizeof(backend::GatherItem));
    backend::run_gather(d_items + (size_t)first * nsb, count * nsb, d_payload);
    std::vector<uint32_t> words(need_words);
    backend::d2h(words.data(), d_payload, need_words * 4);
    for (int s = first; s < end; s++) {
      Stream<PIX>& q = st[s];
      const FrameParams& f = fp[s];
      HostBits& b = q.bits;
      // write_frame_header (write_bits.c:98-121)
      b.put(1, f.frame_type != F_I); b.put(8, f.qp); b.put(4, f.num_intra_modes);
      if (f.frame_type != F_I) b.put(2, f.num_ref - 1);
      for (int r = 0; r < f.num_ref; r++) b.put(6, f.ref_array[r] + 1);
      b.put(16, f.frame_num);
      CdefHeader ch;
      const int cdef_pos = b.nbits;
      if (sp.cdef) {
        ch.bits = h_cjobs[s].cdef_bits;
        for (int i = 0; i < 8; i++) ch.strengths[i] = ch.uv_strengths[i] = 127;
      }
      write_cdef_params(b, -1, sp.cdef, ch);
      {
        long long pbits = 0;
        for (int i = 0; i < nsb; i++) pbits += nb[(size_t)s * nsb + i];
        b.append_words(words.data() + (stream_off[s] >> 5), (int)pbits);
      }
      if (sp.cdef) {
        CdefResult R;
        backend::d2h(&R, q.cdef_res, sizeof(R));
        if (h_cjobs[s].cdef_bits != 0 && R.nb_bits) {
          std::vector<int> sel(R.sb_count);
          if (R.sb_count) backend::d2h(sel.data(), q.cdef_sel, R.sb_count * sizeof(int));
          for (int i = 0; i < R.sb_count; i++) b.put(R.nb_bits, (uint32_t)sel[i]);
        }
        ch.bits = R.nb_bits;
        for (int i = 0; i < 8; i++) { ch.strengths[i] = R.strengths[i]; ch.uv_strengths[i] = R.uv_strengths[i]; }
        write_cdef_params(b, cdef_pos, 1, ch, raw_frames ? q.bit_phase : 0);
      }
      if (sp.clpf)
        for (auto& pr : lplan[s].bits) b.put(pr.first, pr.second);
      q.log.back().num_bits += b.nbits;
      if (q.rc.on()) {  // the controller learns the frame's bits before the stream's next frame is prepared
        RcStat& r = q.rc_cur;
        rc_update(q.rcs, r.frame_class, (long long)(r.frame_class == 0 ? r.sum_intra : r.sum_best), f.qp, q.log.back().num_bits);
        r.fullness = q.rcs.F; r.buffer_bits = q.rcs.B; r.target_bits = q.rcs.T; r.overflows = q.rcs.overflows;
        q.rclog.push_back(r);
      }
      q.num_encoded++;
      if (q.gop.started) q.gop.advance(f);
      if (raw_frames) continue;
      // flush_all_bits framing (putbits.c:45-83)
      uint32_t nbytes = (uint32_t)b.num_bytes();
      for (int i = 0; i < 4; i++) q.out.push_back((uint8_t)(nbytes >> (24 - 8 * i)));
      b.to_bytes(q.out);
      b.clear();
    }
  }
};

}  // namespace tk
