// hip_kernels.h - the frame-level kernels of the throughput build (part of the translation unit thor_hip.cpp, device-only): deblocking, padded
// reference, frame SSE, bit gather, CDEF, CLPF, the temporally interpolated reference, the bit-depth conversion of frames that enter and leave at a lower
// input depth, the conversion between a caller's frame layout (NV12, P010, a row pitch) and the engine's planes.  Launched by hip_backend.h.
// The dependency-driven persistent superblock kernel is not here: a task is (stream, superblock), SB(k,l) needs its left neighbour (k,l-1) and its
// up-right neighbour (k-1,l+1) ((k-1,l) in the last column) - SURVEY.md Appendix A; the kernel is in tk_kernel.h, its ready-task queue in tk_sched.h.
#pragma once
namespace tk {

template <typename PIX> __global__ void k_deblock(const FrameJob<PIX>* jobs, int pass) {
  const FrameJob<PIX>& J = jobs[blockIdx.y];
  DbParams P;
  P.width = J.cfg.width; P.height = J.cfg.height; P.bitdepth = J.cfg.bitdepth;
  const int qpc = g_tab.chroma_qp[J.qp];
  P.beta = g_tab.beta[J.qp] << (P.bitdepth - 8);
  P.tc_y = g_tab.tc[J.qp] >> (12 - P.bitdepth);
  P.tc_c = g_tab.tc[qpc] >> (12 - P.bitdepth);
  P.cells = J.cells; P.cs = J.cell_stride;
  deblock_pass(J.rec, P, pass, (int)(blockIdx.x * blockDim.x + threadIdx.x), (int)(gridDim.x * blockDim.x));
}

template <typename PIX> struct RefJob { Plane3<PIX> rec, ref; int width, height; };
template <typename PIX> __global__ void k_make_ref(const RefJob<PIX>* rj) {
  const RefJob<PIX>& R = rj[blockIdx.y];
  make_ref_rows(R.rec, R.ref, R.width, R.height, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, (int)blockDim.x);
}

// Per-plane SSE of the final reconstruction against the original (frame_sse_rows), streams along y: each wavefront takes rows
// (blockIdx.x * 4 + wave, + 4 * gridDim.x, ...), sums its lanes' 64-bit partials with DPP and adds them to the stream's slots with one
// 64-bit atomic per plane.  Integer sums: the result does not depend on the order.
template <typename PIX> __global__ __launch_bounds__(256) void k_frame_sse(const FrameJob<PIX>* jobs, unsigned long long* out) {
  const FrameJob<PIX>& J = jobs[blockIdx.y];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  unsigned long long acc[3] = {0, 0, 0};
  frame_sse_rows(J.orig, J.rec, J.cfg.width, J.cfg.height, (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4, lane, 64, acc);
  for (int k = 0; k < 3; k++) {
    const unsigned long long v = wave_sum64_dpp(acc[k]);
    if (lane == 0 && v) atomicAdd(&out[4 * (size_t)blockIdx.y + k], v);
  }
}

// Bit-level concatenation: one workgroup per item.  dst is zero-filled; words are OR-ed in.
__global__ void k_gather_bits(const backend::GatherItem* items, int n, uint32_t* dst) {
  const int it = blockIdx.x;
  if (it >= n) return;
  const backend::GatherItem g = items[it];
  const int nw = (g.nbits + 31) >> 5;
  const int sh = (int)(g.dst_bit & 31);
  const long long w0 = g.dst_bit >> 5;
  for (int j = threadIdx.x; j < nw; j += blockDim.x) {
    uint32_t v = g.src[j];
    const int valid = g.nbits - 32 * j;           // bits of this word that belong to the string
    if (valid < 32) v &= ~((1u << (32 - valid)) - 1u);
    if (sh == 0) atomicOr(&dst[w0 + j], v);
    else {
      atomicOr(&dst[w0 + j], v >> sh);
      const uint32_t lo = v << (32 - sh);
      if (lo) atomicOr(&dst[w0 + j + 1], lo);
    }
  }
}

template <typename PIX> __global__ void k_copy_planes(const CdefJob<PIX>* cj) {
  const CdefJob<PIX>& C = cj[blockIdx.y];
  const int rows = C.height + C.height;  // Y rows + U rows + V rows
  for (int it = blockIdx.x; it < rows; it += gridDim.x) {
    const PIX* s; PIX* d; int w;
    if (it < C.height) { s = C.rec.y + (size_t)it * C.rec.sy; d = C.src.y + (size_t)it * C.src.sy; w = C.width; }
    else if (it < C.height + C.height / 2) { int r = it - C.height; s = C.rec.u + (size_t)r * C.rec.sc; d = C.src.u + (size_t)r * C.src.sc; w = C.width / 2; }
    else { int r = it - C.height - C.height / 2; s = C.rec.v + (size_t)r * C.rec.sc; d = C.src.v + (size_t)r * C.src.sc; w = C.width / 2; }
    for (int x = threadIdx.x; x < w; x += blockDim.x) d[x] = s[x];
  }
}
// passes 0 (flags), 1 (direction / variance per 8x8 block) and 4 (apply) of CDEF: one instance per pass, so that each gets its own register allocation
template <typename PIX, int PASS> __global__ __launch_bounds__(256) void k_cdef(const CdefJob<PIX>* cj) {   // (no bound = 1024 threads = a 128-VGPR cap: the apply pass spilled 30)
  const CdefJob<PIX>& C = cj[blockIdx.y];
  const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x), gsize = (int)(gridDim.x * blockDim.x);
  if constexpr (PASS == 0) cdef_pass_flags(C, gid, gsize);
  else if constexpr (PASS == 1) cdef_pass_dir(C, gid, gsize);
  else cdef_pass_apply(C, gid, gsize);
}
// pass 2 of the CDEF search (tk_cdef.h: wavefront form): one wavefront per 8x8 luma-unit block, four independent wavefronts per workgroup (no workgroup
// barrier: a wavefront whose block is skipped leaves at once)
template <typename PIX> __global__ __launch_bounds__(256) void k_cdef_mse(const CdefJob<PIX>* cj) {
  const CdefJob<PIX>& C = cj[blockIdx.y];
  if (!C.cdef_bits) return;
  __shared__ CdefWaveWs<PIX> ws[4];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  const int b = (int)blockIdx.x * 4 + wave;
  if (b >= (C.width / 8) * (C.height / 8)) return;
  cdef_mse_block_wave(mk_team(lane, 64), C, b, &ws[wave]);
}
template <typename PIX> __global__ void k_clpf(const ClpfJob<PIX>* lj, int pass) {
  const ClpfJob<PIX>& L = lj[blockIdx.y];
  const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x), gsize = (int)(gridDim.x * blockDim.x);
  if (pass == 0) clpf_pass_stats(L, gid, gsize);
  else clpf_pass_apply(L, gid, gsize);
}
template <typename PIX> __global__ void k_clpf_copy(const ClpfJob<PIX>* lj) {  // rec -> src (unfiltered copy)
  const ClpfJob<PIX>& C = lj[blockIdx.y];
  const int rows = C.height + C.height;
  for (int it = blockIdx.x; it < rows; it += gridDim.x) {
    const PIX* s; PIX* d; int w;
    if (it < C.height) { s = C.rec.y + (size_t)it * C.rec.sy; d = C.src.y + (size_t)it * C.src.sy; w = C.width; }
    else if (it < C.height + C.height / 2) { int r = it - C.height; s = C.rec.u + (size_t)r * C.rec.sc; d = C.src.u + (size_t)r * C.src.sc; w = C.width / 2; }
    else { int r = it - C.height - C.height / 2; s = C.rec.v + (size_t)r * C.rec.sc; d = C.src.v + (size_t)r * C.src.sc; w = C.width / 2; }
    for (int x = threadIdx.x; x < w; x += blockDim.x) d[x] = s[x];
  }
}
template <typename PIX> __global__ __launch_bounds__(1024) void k_cdef_select(const CdefJob<PIX>* cj) {
  BlockTeam t{(int)threadIdx.x, (int)blockDim.x};
  cdef_pass_select(t, cj[blockIdx.x]);
}

// ---- temporally interpolated reference (tk_interp_dev.h) -----------------------------------------------------------
template <typename PIX> __global__ void k_interp_clear(const idev::Job<PIX>* jobs) {
  const idev::Job<PIX>& J = jobs[blockIdx.y];
  const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x), gsz = (int)(gridDim.x * blockDim.x);
  for (int l = 0; l < J.levels; l++) {
    const idev::Level<PIX>& L = J.lv[l];
    const int cnt = L.bw * L.bh + L.bw + 2;
    uint32_t* a = (uint32_t*)L.mv[0];
    uint32_t* b = (uint32_t*)L.mv[1];
    for (int k = gid; k < cnt; k += gsz) { a[k] = 0; b[k] = 0; }
    for (int k = gid; k < L.bh / idev::kStep + 1; k += gsz) L.prog[k] = 0;
  }
}
template <typename PIX> __global__ void k_interp_down(const idev::Job<PIX>* jobs, int l) {
  const idev::Job<PIX>& J = jobs[blockIdx.y];
  if (l >= J.levels) return;
  const int ow = J.width >> l, oh = J.height >> l, pw = ow + 64;
  const int total = (oh + 64) * pw;
  for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < total; k += (int)(gridDim.x * blockDim.x)) {
    const int i = k / pw - 32, j = k % pw - 32;
    for (int r = 0; r < 2; r++)
      idev::down2x2_item(l == 1 ? J.ref[r].y : J.dpic[r][l - 1], l == 1 ? J.ref[r].sy : J.dstride[l - 1], J.dpic[r][l], J.dstride[l], ow, oh, i, j);
  }
}
// One wavefront per 16x16-block row.  Rows are handed out by a ticket, so the row above a wave's row was always taken by
// a wave that started earlier: the wave waits until that row is two blocks ahead (or finished) and never dead-locks.
template <typename PIX> __global__ __launch_bounds__(64) void k_interp_estimate(const idev::Job<PIX>* jobs, int lvl) {
  const idev::Job<PIX>& J = jobs[blockIdx.y];
  if (lvl >= J.levels) return;
  const idev::Level<PIX>& L = J.lv[lvl];
  const Team t = mk_team((int)threadIdx.x, 64);
  int row = 0;
  if (threadIdx.x == 0) row = (int)atomicAdd((unsigned*)L.ticket, 1u);
  row = __builtin_amdgcn_readfirstlane(row);
  const int nrows = L.bh / idev::kStep, ncols = L.bw / idev::kStep;
  if (row >= nrows) return;
  for (int c = 0; c < ncols; c++) {
    if (row > 0) {
      const int need = c + 2 < ncols ? c + 2 : ncols;
      while (__hip_atomic_load(&L.prog[row - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) __builtin_amdgcn_s_sleep(8);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    idev::estimate_block(t, L, row * idev::kStep, c * idev::kStep);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (threadIdx.x == 0) __hip_atomic_store(&L.prog[row], c + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}
template <typename PIX> __global__ __launch_bounds__(64) void k_interp_merge(const idev::Job<PIX>* jobs, int lvl) {
  const idev::Job<PIX>& J = jobs[blockIdx.y];
  if (lvl >= J.levels) return;
  const idev::Level<PIX>& L = J.lv[lvl];
  const Team t = mk_team((int)threadIdx.x, 64);
  for (int k = blockIdx.x; k < L.bw * L.bh; k += gridDim.x) idev::merge_block(t, L, k / L.bw, k % L.bw);
}
template <typename PIX> __global__ void k_interp_upscale(const idev::Job<PIX>* jobs, int lvl) {  // level lvl -> guide of lvl-1
  const idev::Job<PIX>& J = jobs[blockIdx.y];
  if (lvl >= J.levels || lvl < 1) return;
  const idev::Level<PIX>& L = J.lv[lvl];
  const idev::Level<PIX>& O = J.lv[lvl - 1];
  for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < O.bw * O.bh; k += (int)(gridDim.x * blockDim.x))
    idev::upscale_item(L.nmv[1], L.bw, O.gmv1, O.bw, k / O.bw, k % O.bw);
}
template <typename PIX> __global__ __launch_bounds__(64) void k_interp_mc(const idev::Job<PIX>* jobs) {
  const idev::Job<PIX>& J = jobs[blockIdx.y];
  const idev::Level<PIX>& L = J.lv[0];
  const Team t = mk_team((int)threadIdx.x, 64);
  for (int k = blockIdx.x; k < L.bw * L.bh; k += gridDim.x) idev::mot_comp_unit(t, J, k / L.bw, k % L.bw);
}
template <typename PIX> __global__ void k_interp_pad(const idev::Job<PIX>* jobs) {
  const idev::Job<PIX>& J = jobs[blockIdx.y];
  idev::pad_item(J, (int)blockIdx.x, (int)threadIdx.x, (int)blockDim.x);
}

// ---- input at a lower bit depth than the engine's (tk_filters.h: depth_up_rows, depth_down_rows, frame_sse_depth_rows) --------
// One frame per launch, one wavefront per row (blockIdx.x * 4 + wave, + 4 * gridDim.x, ...), lanes along the row.
template <typename SRC> __global__ __launch_bounds__(256) void k_depth_up(const SRC* src, Plane3<uint16_t> dst, int width, int height, int shift) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  depth_up_rows(src, dst, width, height, shift, (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4, lane, 64);
}
template <typename DST> __global__ __launch_bounds__(256) void k_depth_down(Plane3<uint16_t> src, DST* dst, int width, int height, int shift, int input_bitdepth) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  depth_down_rows(src, dst, width, height, shift, input_bitdepth, (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4, lane, 64);
}
// k_frame_sse at the input depth: same grid, same reduction, same slots.
__global__ __launch_bounds__(256) void k_frame_sse_depth(const FrameJob<uint16_t>* jobs, int shift, int input_bitdepth, unsigned long long* out) {
  const FrameJob<uint16_t>& J = jobs[blockIdx.y];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  unsigned long long acc[3] = {0, 0, 0};
  frame_sse_depth_rows(J.orig, J.rec, J.cfg.width, J.cfg.height, shift, input_bitdepth, (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4, lane, 64, acc);
  for (int k = 0; k < 3; k++) {
    const unsigned long long v = wave_sum64_dpp(acc[k]);
    if (lane == 0 && v) atomicAdd(&out[4 * (size_t)blockIdx.y + k], v);
  }
}

// ---- frames in a caller's layout (tk_filters.h: layout_in_rows, layout_out_rows) --------
// One frame per launch, one wavefront per luma or chroma row, lanes along the row, as above.  `frame`: device memory in layout L.
template <typename SRC, typename PIX>
__global__ __launch_bounds__(256) void k_layout_in(const void* frame, PixLayout L, Plane3<PIX> dst, int width, int height, int up) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  layout_in_rows<SRC, PIX>(frame, L, dst, width, height, up, (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4, lane, 64);
}
template <typename PIX, typename DST>
__global__ __launch_bounds__(256) void k_layout_out(Plane3<PIX> src, void* frame, PixLayout L, int width, int height, int shift, int input_bitdepth) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
  layout_out_rows<PIX, DST>(src, frame, L, width, height, shift, input_bitdepth, (int)blockIdx.x * 4 + wave, (int)gridDim.x * 4, lane, 64);
}

// ---- RGB frames (tk_filters.h: rgb_in_rows, rgb_out_rows) --------
// One frame per launch, one workgroup per pair of luma rows with its chroma row, its 256 lanes along the rows in runs of whole 16-byte vectors of the
// RGB side.  `frame`: device memory in format R, whose coefficients come by value.  No LDS, no atomics.
template <typename SRC, typename PIX>
__global__ __launch_bounds__(256) void k_rgb_in(const void* frame, RgbFormat R, Plane3<PIX> dst, int width, int height, int up) {
  rgb_in_rows<SRC, PIX>(frame, R, dst, width, height, up, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, 256);
}
template <typename PIX, typename DST>
__global__ __launch_bounds__(256) void k_rgb_out(Plane3<PIX> src, void* frame, RgbFormat R, int width, int height, int shift) {
  rgb_out_rows<PIX, DST>(src, frame, R, width, height, shift, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x, 256);
}

// ---- frames of another size (tk_scale.h: scale_load_row, scale_hfilter_row, scale_vfilter) --------
// One frame per launch, all three planes: one workgroup per tile of SCALE_TW x SCALE_TH destination samples (luma tiles, then U, then V).  Each of
// the four wavefronts takes every fourth source row the tile needs: 16-byte vectors of it into the wavefront's row buffer, the horizontal taps from
// there into `inter`; then all 256 lanes filter `inter` vertically and write the plane.  LDS: the row buffers and the tile's horizontal
// coefficients (static), the intermediate rows (dynamic: `vrows` of the plan x SCALE_TW x 2 bytes, at most 36 KiB).  The intermediate never leaves LDS.
template <typename SRC, typename PIX>
__global__ __launch_bounds__(256) void k_scale_in(const void* frame, PixLayout L, ScaleTables tab, Plane3<PIX> dst, int src_w, int width, int height, int maxv, int up) {
  __shared__ __attribute__((aligned(16))) int16_t rowbuf[SCALE_WAVES * SCALE_ROWCAP];
  __shared__ __attribute__((aligned(16))) int16_t coef[SCALE_MAX_TAPS * SCALE_TW];
  extern __shared__ __attribute__((aligned(16))) int16_t inter[];
  const int tid = (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const bool luma = (int)blockIdx.x < scale_tiles(width, height);
  const ScaleAxis H = luma ? tab.a[0] : tab.a[2];
  const ScaleAxis V = luma ? tab.a[1] : tab.a[3];
  const ScaleTile t = scale_tile((int)blockIdx.x, width, height, H, V);
  const ScaleSrc s = scale_src(frame, L, t.plane, src_w);
  scale_stage_coef(H, t, coef, tid, 256);
  __syncthreads();
  for (int r = 0; r < t.nrows; r += SCALE_WAVES) {   // t.nrows is the same in every lane: the barriers are met by all
    if (r + wave < t.nrows) scale_load_row<SRC>(s, L.msb, t.r0 + r + wave, t.klo, t.khi, rowbuf + wave * SCALE_ROWCAP, lane, 64);
    __syncthreads();
    if (r + wave < t.nrows) scale_hfilter_row(H, t, coef, rowbuf + wave * SCALE_ROWCAP, inter + (r + wave) * SCALE_TW, lane, 64);
    __syncthreads();
  }
  scale_vfilter<PIX>(V, t, inter, scale_plane(dst, t.plane), t.plane ? dst.sc : dst.sy, maxv, up, tid, 256);
}

// ---- rate control: the frame analysis (tk_rc.h: rc_half_sample, rc_block_sum, rc_block_dev, rc_block_inter) --------
// Streams along y.  One workgroup per tile of RC_TILE x RC_TILE half-size samples (4 x 4 blocks): its 256 lanes make the tile from the staged original
// (into LDS and into the stream's current half-size plane) and load the previous plane's tile with a halo of RC_RANGE into LDS - samples outside the
// plane as zeros, which no legal candidate reads.  Then each wavefront takes every fourth block: one lane per sample for the mean and the intra cost,
// one lane per candidate vector for the inter cost (five rounds of 64 for the 289), DPP reductions; the lanes read neighbouring LDS addresses (the
// candidates of a round differ in dx) and the block's sample as a broadcast.  The wavefronts' sums meet in LDS: three 64-bit atomic adds per workgroup.
// Integer sums: the result does not depend on the order.  LDS: 3.3 KiB (8-bit) / 6.6 KiB (16-bit).
// PREV_ORIG (thor_hip_scene_cost): the previous frame is a full-size original (J.prev_y), not a stored half-size plane.  Its 96 x 96 window is halved while
// it is loaded - a lane makes four neighbouring half-size samples from two 8-sample loads (rc_half_quad) and stores them as one LDS word pair - so the
// LDS stays what it is; the window's groups of four lie wholly inside or outside the plane (its width is a multiple of 4).  Nothing but the sums is stored.
template <typename PIX, bool PREV_ORIG> __global__ __launch_bounds__(256) void k_rc_cost(const RcJob<PIX>* jobs) {
  const RcJob<PIX> J = jobs[blockIdx.y];
  __shared__ PIX s_cur[RC_TILE * RC_TILE];
  __shared__ PIX s_prev[RC_WIN * RC_WIN];
  __shared__ unsigned long long s_acc[4][3];
  const int tid = (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int tiles_x = (J.hw + RC_TILE - 1) / RC_TILE;
  const int tx0 = ((int)blockIdx.x % tiles_x) * RC_TILE, ty0 = ((int)blockIdx.x / tiles_x) * RC_TILE;
  for (int i = tid; i < RC_TILE * RC_TILE; i += 256) {
    const int gx = tx0 + (i & (RC_TILE - 1)), gy = ty0 + i / RC_TILE;
    PIX v = 0;
    if (gx < J.hw && gy < J.hh) {
      v = (PIX)rc_half_sample(J.y, J.sy, gx, gy);
      if constexpr (!PREV_ORIG) J.cur[(size_t)gy * J.hw + gx] = v;
    }
    s_cur[i] = v;
  }
  const bool has_prev = PREV_ORIG ? J.prev_y != nullptr : J.prev != nullptr;
  if constexpr (PREV_ORIG) {
    if (has_prev)
      for (int i = tid; i < RC_WIN * RC_WIN / 4; i += 256) {
        const int wx = (i % (RC_WIN / 4)) * 4, wy = i / (RC_WIN / 4);
        const int gx = tx0 - RC_RANGE + wx, gy = ty0 - RC_RANGE + wy;
        PIX q[4] = {0, 0, 0, 0};
        if (gx >= 0 && gx + 4 <= J.hw && gy >= 0 && gy < J.hh) rc_half_quad(J.prev_y, J.prev_sy, gx, gy, q);
        for (int k = 0; k < 4; k++) s_prev[wy * RC_WIN + wx + k] = q[k];
      }
  } else if (has_prev)
    for (int i = tid; i < RC_WIN * RC_WIN; i += 256) {
      const int gx = tx0 - RC_RANGE + i % RC_WIN, gy = ty0 - RC_RANGE + i / RC_WIN;
      s_prev[i] = gx >= 0 && gx < J.hw && gy >= 0 && gy < J.hh ? J.prev[(size_t)gy * J.hw + gx] : (PIX)0;
    }
  __syncthreads();
  unsigned long long acc[3] = {0, 0, 0};
  for (int b = wave; b < (RC_TILE / RC_BLK) * (RC_TILE / RC_BLK); b += 4) {   // b, and with it every branch below, is the same in all lanes of a wavefront
    const int lx = (b % (RC_TILE / RC_BLK)) * RC_BLK, ly = (b / (RC_TILE / RC_BLK)) * RC_BLK;
    const int x0 = tx0 + lx, y0 = ty0 + ly;
    if (x0 >= J.hw || y0 >= J.hh) continue;
    const int bw = J.hw - x0 < RC_BLK ? J.hw - x0 : RC_BLK, bh = J.hh - y0 < RC_BLK ? J.hh - y0 : RC_BLK, n = bw * bh;
    const PIX* blk = s_cur + ly * RC_TILE + lx;
    const unsigned sum = (unsigned)wave_sum_dpp((int)rc_block_sum(blk, RC_TILE, bw, bh, lane, 64));   // at most 64 * 4095: fits the 32-bit reductions
    const int mean = (int)((sum + (unsigned)(n / 2)) / (unsigned)n);
    const unsigned intra = (unsigned)wave_sum_dpp((int)rc_block_dev(blk, RC_TILE, bw, bh, mean, lane, 64));
    unsigned inter = intra;
    if (has_prev)
      inter = wave_min_u32_dpp(rc_block_inter(blk, RC_TILE, s_prev + (ly + RC_RANGE) * RC_WIN + lx + RC_RANGE, RC_WIN, bw, bh, x0, y0, J.hw, J.hh, lane, 64));
    rc_block_add(intra, inter, acc);
  }
  if (lane == 0)
    for (int k = 0; k < 3; k++) s_acc[wave][k] = acc[k];
  __syncthreads();
  if (tid < 3) {
    const unsigned long long v = s_acc[0][tid] + s_acc[1][tid] + s_acc[2][tid] + s_acc[3][tid];
    if (v) atomicAdd(&J.out[tid], v);
  }
}

// ---- temporal filter (tk_tf.h: tf_block_search, tf_block_record, tf_blend_quad) --------
// k_tf_search: requests along z, their neighbours along y (a workgroup beyond its request's nrefs leaves at once).  One workgroup per tile of TF_TILE x
// TF_TILE luma samples (4 x 4 blocks): its 256 lanes load the current tile and the neighbour's tile with a halo of TF_RANGE into LDS, four samples per
// lane and load - the window starts at a multiple of 8, so a group of four lies wholly inside or outside the plane; outside is zeros, which no legal
// candidate reads.  Then each wavefront takes every fourth block: one lane per candidate vector (five rounds of 64 for the 289), packed SADs on dwords,
// a DPP minimum of the (SAD, rank) keys, and lane 0 stores the block's record.  LDS: 3.3 KiB (8-bit) / 6.6 KiB (16-bit).
template <typename PIX> __global__ __launch_bounds__(256) void k_tf_search(const TfJob<PIX>* jobs) {
  struct alignas(4 * sizeof(PIX)) Quad { PIX v[4]; };
  const TfJob<PIX>& J = jobs[blockIdx.z];
  const int k = (int)blockIdx.y;
  if (k >= J.nrefs) return;   // the same for the whole workgroup, before its barrier
  __shared__ __attribute__((aligned(16))) PIX s_cur[TF_TILE * TF_TILE];
  __shared__ __attribute__((aligned(16))) PIX s_ref[TF_WIN * TF_WIN + 8];   // + 8: tf_sad8x8 reads one dword beyond a row's last
  const int tid = (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int W = J.width, H = J.height;
  const int tiles_x = (W + TF_TILE - 1) / TF_TILE;
  const int tx0 = ((int)blockIdx.x % tiles_x) * TF_TILE, ty0 = ((int)blockIdx.x / tiles_x) * TF_TILE;
  {
    const int lx = (tid & 7) * 4, ly = tid >> 3, gx = tx0 + lx, gy = ty0 + ly;
    Quad q = {{0, 0, 0, 0}};
    if (gx < W && gy < H) __builtin_memcpy(&q, __builtin_assume_aligned(J.cur.y + (size_t)gy * J.cur.sy + gx, sizeof(Quad)), sizeof(Quad));
    __builtin_memcpy(__builtin_assume_aligned(s_cur + ly * TF_TILE + lx, sizeof(Quad)), &q, sizeof(Quad));
  }
  const PIX* ry = J.ref[k].y;
  const int rsy = J.ref[k].sy;
  for (int i = tid; i < TF_WIN * TF_WIN / 4; i += 256) {
    const int wx = (i % (TF_WIN / 4)) * 4, wy = i / (TF_WIN / 4);
    const int gx = tx0 - TF_RANGE + wx, gy = ty0 - TF_RANGE + wy;
    Quad q = {{0, 0, 0, 0}};
    if (gx >= 0 && gx + 4 <= W && gy >= 0 && gy < H) __builtin_memcpy(&q, __builtin_assume_aligned(ry + (size_t)gy * rsy + gx, sizeof(Quad)), sizeof(Quad));
    __builtin_memcpy(__builtin_assume_aligned(s_ref + wy * TF_WIN + wx, sizeof(Quad)), &q, sizeof(Quad));
  }
  if (tid < 8) s_ref[TF_WIN * TF_WIN + tid] = 0;
  __syncthreads();
  const int bw = W / TF_BLK, nb = bw * (H / TF_BLK);
  for (int b = wave; b < (TF_TILE / TF_BLK) * (TF_TILE / TF_BLK); b += 4) {   // b, and with it every branch below, is the same in all lanes of a wavefront
    const int lx = (b % (TF_TILE / TF_BLK)) * TF_BLK, ly = (b / (TF_TILE / TF_BLK)) * TF_BLK;
    const int x0 = tx0 + lx, y0 = ty0 + ly;
    if (x0 >= W || y0 >= H) continue;
    const unsigned key = wave_min_u32_dpp(tf_block_search(s_cur + ly * TF_TILE + lx, TF_TILE, s_ref, (ly + TF_RANGE) * TF_WIN + lx + TF_RANGE, TF_WIN, x0, y0, W, H, lane, 64));
    if (lane == 0) J.blk[(size_t)k * nb + (y0 / TF_BLK) * bw + x0 / TF_BLK] = tf_block_record(key, J.sh, J.strength, J.dist[k]);
  }
}
// k_tf_blend: requests along y, one workgroup per tile of TF_TILE x TF_TILE luma samples and its two 16 x 16 chroma tiles.  One lane per four neighbouring
// samples of a row: 256 lanes for the luma tile, 64 each for U and V; a group lies inside one block, reads that block's records, its own four samples
// and the displaced four of every neighbour with a weight from the planes, and stores four samples at once.  No LDS.  nrefs 0 copies the frame.
template <typename PIX> __global__ __launch_bounds__(256) void k_tf_blend(const TfJob<PIX>* jobs) {
  const TfJob<PIX>& J = jobs[blockIdx.y];
  const int tid = (int)threadIdx.x;
  const int W = J.width, H = J.height;
  const int tiles_x = (W + TF_TILE - 1) / TF_TILE;
  const int tx0 = ((int)blockIdx.x % tiles_x) * TF_TILE, ty0 = ((int)blockIdx.x / tiles_x) * TF_TILE;
  {
    const int x = tx0 + (tid & 7) * 4, y = ty0 + (tid >> 3);
    if (x < W && y < H) tf_blend_quad(J, 0, x, y);
  }
  if (tid < 128) {
    const int l = tid & 63, x = tx0 / 2 + (l & 3) * 4, y = ty0 / 2 + (l >> 2);
    if (x < W / 2 && y < H / 2) tf_blend_quad(J, 1 + (tid >> 6), x, y);
  }
}
}  // namespace tk
