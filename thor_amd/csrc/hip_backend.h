// hip_backend.h - host side of the device (part of the translation unit thor_hip.cpp, device-only): initialisation, namespace backend of tk_encoder.h
// (memory, copies, the superblock scheduler state and every run_* launch sequence), launch_frame_sse, and the helpers the C ABI shares (DevBuf,
// upload_yuv / download_yuv).
#pragma once
namespace tk {
static bool g_inited = false;
static hipStream_t g_stream = nullptr;
struct KernelClock {
  double sb_ms = 0, filt_ms = 0;
  long sb_launches = 0;
};
static KernelClock g_clk;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_sb_events, g_filt_events;

// The backend is one-device-per-process and single-threaded by design (one process per GPU, include/thor_hip.h): the
// first call fixes the device; a later request for another device, or a device index the node does not have, is an
// error (returns false) - never a silent fall-back to device 0.
static int g_device = -1;
static bool ensure_init(int device) {
  if (g_inited) {
    if (device != g_device) { fprintf(stderr, "thor_hip: this process is bound to HIP device %d (requested %d); use one process per GPU\n", g_device, device); return false; }
    HIPCHECK(hipSetDevice(g_device));  // hipSetDevice is per thread
    return true;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    fprintf(stderr, "Run-time error...\nthor_hip: no HIP device available - this library has no CPU path\n...now exiting to system...\n");
    abort();
  }
  if (device < 0 || device >= n) { fprintf(stderr, "thor_hip: HIP device %d requested but only %d visible (check LOCAL_RANK / HIP_VISIBLE_DEVICES)\n", device, n); return false; }
  g_device = device;
  HIPCHECK(hipSetDevice(device));
  HIPCHECK(hipStreamCreate(&g_stream));
  static Tables h;
  init_tables(&h);
  HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_tab), &h, sizeof(h)));
  if (thor_lat_upload_tables(&h, sizeof(h)) || thor_wide_upload_tables(&h, sizeof(h)) || thor_katbits_upload_tables(&h, sizeof(h))) { fprintf(stderr, "Run-time error...\nthor_hip: table upload of the other translation units (few-stream kernels, block-syntax test kernels) failed\n...now exiting to system...\n"); abort(); }
  g_inited = true;
  return true;
}
// entry points without a device argument: the device this process is bound to, else device 0
static bool ensure_init_any() { return ensure_init(g_inited ? g_device : 0); }

namespace backend {
void* dev_alloc(size_t n) {
  void* p = nullptr;
  HIPCHECK(hipMalloc(&p, n ? n : 1));
  HIPCHECK(hipMemsetAsync(p, 0, n ? n : 1, g_stream));
  return p;
}
void dev_free(void* p) { if (p) HIPCHECK(hipFree(p)); }
void h2d(void* d, const void* h, size_t n) { HIPCHECK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, g_stream)); HIPCHECK(hipStreamSynchronize(g_stream)); }
void d2h(void* h, const void* d, size_t n) { HIPCHECK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, g_stream)); HIPCHECK(hipStreamSynchronize(g_stream)); }
void dev_memset(void* d, int v, size_t n) { HIPCHECK(hipMemsetAsync(d, v, n, g_stream)); }
static void harvest(std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double& acc) {
  for (auto& p : v) {
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, p.first, p.second));
    acc += ms;
    HIPCHECK(hipEventDestroy(p.first));
    HIPCHECK(hipEventDestroy(p.second));
  }
  v.clear();
}
void dev_sync() {
  HIPCHECK(hipStreamSynchronize(g_stream));
  harvest(g_sb_events, g_clk.sb_ms);
  harvest(g_filt_events, g_clk.filt_ms);
}
size_t team_ws_bytes(int pix_bytes) { return pix_bytes == 1 ? sizeof(BigWs<uint8_t>) : sizeof(BigWs<uint16_t>); }

static std::pair<hipEvent_t, hipEvent_t> ev_begin() {
  std::pair<hipEvent_t, hipEvent_t> p;
  HIPCHECK(hipEventCreate(&p.first));
  HIPCHECK(hipEventCreate(&p.second));
  HIPCHECK(hipEventRecord(p.first, g_stream));
  return p;
}
// A timed section of filter launches on g_stream: begins where it is declared, ends with its scope (second event, kernel time book-keeping, launch errors).
namespace {
struct FilterTimer {
  std::pair<hipEvent_t, hipEvent_t> ev = ev_begin();
  FilterTimer() = default;
  FilterTimer(const FilterTimer&) = delete;
  ~FilterTimer() {
    HIPCHECK(hipEventRecord(ev.second, g_stream));
    g_filt_events.push_back(ev);
    HIPCHECK(hipGetLastError());
  }
};
}  // namespace

struct DfState {  // per engine (keyed by its device job array)
  DfCtl* ctl = nullptr;
  unsigned* queue = nullptr;
  unsigned* cnt = nullptr;
  uint8_t* pool = nullptr;
  unsigned long long* times = nullptr;
  unsigned* range = nullptr;
  int S = 0, nsb = 0, wgs = 0;
  size_t slot = 0;
  int frame = 0;
  int kern = 0;  // the build of the 8-bit kernel this engine's launches use: 0 thor_hip.cpp (throughput), 1 thor_hip_lat.cpp, 2 thor_hip_wide.cpp
};
static std::map<const void*, DfState> g_df;
static int g_last_kern = 0;   // build of the 8-bit kernel the most recently configured engine uses (thor_hip_superblock_kernel_in_use)
static void df_free(DfState& D) {
  if (!D.ctl) return;
  HIPCHECK(hipFree(D.ctl)); HIPCHECK(hipFree(D.queue)); HIPCHECK(hipFree(D.cnt)); HIPCHECK(hipFree(D.pool)); HIPCHECK(hipFree(D.range));
  if (D.times) HIPCHECK(hipFree(D.times));
}
template <typename PIX> void run_superblocks(const FrameJob<PIX>* jobs, const FrameJob<PIX>* hjobs, int S, const SbRange* ranges) {
  const int cols = hjobs[0].sb_cols, rows = hjobs[0].sb_rows, nsb = cols * rows;
  const size_t all = (size_t)S * nsb;
  DfState& D = g_df[jobs];
  const size_t slot = (sizeof(BigWs<PIX>) + 255) & ~(size_t)255;
  if (D.S != S || D.nsb != nsb || D.slot != slot) {
    df_free(D);
    D = DfState();
    D.S = S; D.nsb = nsb; D.slot = slot;
    int per_cu = 0;
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_superblocks<PIX>, kWgThreads, 0));
    hipDeviceProp_t prop;
    int dev = 0;
    HIPCHECK(hipGetDevice(&dev));
    HIPCHECK(hipGetDeviceProperties(&prop, dev));
    long cap = (long)(per_cu > 0 ? per_cu : 1) * prop.multiProcessorCount;
    // Which build of the kernel: a stream offers at most min(rows, (cols + 1) / 2) superblocks at a time (the dependency wavefront).  Eight-wave workgroups
    // (one per CU) finish a superblock ~25 % sooner than four-wave ones and saturate at ~3/4 of the throughput build's peak, which that build only reaches
    // with well over a hundred streams: measured (round 6, call 13) the wide build wins by 24-26 % up to S x wavefront = 2 x CUs (3840x2160: 24 / 32 streams
    // 61.3 / 80.2 against 49.2 / 64.1 Mpx/s with four-wave workgroups, 1920x1080: 32 / 64 streams 40.8 / 76.9 against 32.9 / 61.6) and still by 5 % at 2.8 x CUs
    // (48 streams at 3840x2160: 96.3 against 91.5).  Rule: wide up to 2.5 x CUs, the throughput build above.  The latency build (256 VGPRs, two four-wave
    // workgroups per CU) lost its range to the wide build and runs only when forced.  8-bit samples only (the 16-bit kernel has one build).
    // THOR_HIP_KERNEL=std|lat|wide forces one (tests, A/B).
    int pool_waves = kWaves;
    if constexpr (sizeof(PIX) == 1) {
      const long lat_cap = (long)thor_lat_workgroups_per_cu() * prop.multiProcessorCount;
      const long wide_cap = (long)thor_wide_workgroups_per_cu() * prop.multiProcessorCount;
      const long wave_front = (long)S * (rows < (cols + 1) / 2 ? rows : (cols + 1) / 2);
      D.kern = wide_cap > 0 && 2 * wave_front <= 5 * wide_cap ? 2 : 0;
      if (const char* e = getenv("THOR_HIP_KERNEL")) {
        if (!strcmp(e, "lat")) D.kern = lat_cap > 0 ? 1 : 0;
        else if (!strcmp(e, "wide")) D.kern = wide_cap > 0 ? 2 : 0;
        else if (!strcmp(e, "std")) D.kern = 0;
      }
      if (D.kern == 1) cap = lat_cap;
      if (D.kern == 2) { cap = wide_cap; pool_waves = thor_wide_waves(); }
    }
    g_last_kern = sizeof(PIX) == 1 ? D.kern : 0;
    if (const char* e = getenv("THOR_HIP_WGS")) { if (*e) cap = atol(e); }
    D.wgs = (int)(cap < (long)all ? cap : (long)all);
    HIPCHECK(hipMalloc(&D.ctl, sizeof(DfCtl)));
    HIPCHECK(hipMalloc(&D.queue, sizeof(unsigned) * all));
    HIPCHECK(hipMalloc(&D.cnt, sizeof(unsigned) * all));
    HIPCHECK(hipMalloc(&D.range, sizeof(unsigned) * S));
    HIPCHECK(hipMalloc(&D.pool, slot * (size_t)D.wgs * pool_waves));  // one BigWs slot per wavefront
    if (getenv("THOR_SBTIMES")) { HIPCHECK(hipMalloc(&D.times, sizeof(unsigned long long) * 3 * all)); }
  }
  // launch start: the superblocks of every stream's range whose dependencies all lie below the range (whole frames: SB(0,0))
  size_t total = 0;
  {
    std::vector<unsigned> q0, hr(S);
    for (int s2 = 0; s2 < S; s2++) {
      const int lo = ranges ? ranges[s2].lo : 0, hi = ranges ? ranges[s2].hi : 0x7fff;
      hr[s2] = (unsigned)lo | ((unsigned)hi << 16);
      if (lo >= hi) continue;
      for (int k = 0; k < rows; k++)
        for (int l = 0; l < cols; l++) {
          const int t = df_diag(k, l);
          if (t < lo || t >= hi) continue;
          total++;
          if (df_need(k, l, cols, lo) == 0) q0.push_back((unsigned)s2 * (unsigned)nsb + (unsigned)(k * cols + l));
        }
    }
    if (!total) return;
    DfCtl hc0 = {0u, (unsigned)q0.size(), 0u, 0u};
    HIPCHECK(hipMemsetAsync(D.queue, 0xff, sizeof(unsigned) * total, g_stream));
    HIPCHECK(hipMemsetAsync(D.cnt, 0, sizeof(unsigned) * all, g_stream));
    if (D.times) HIPCHECK(hipMemsetAsync(D.times, 0, sizeof(unsigned long long) * 3 * all, g_stream));
    HIPCHECK(hipMemcpyAsync(D.queue, q0.data(), sizeof(unsigned) * q0.size(), hipMemcpyHostToDevice, g_stream));
    HIPCHECK(hipMemcpyAsync(D.range, hr.data(), sizeof(unsigned) * S, hipMemcpyHostToDevice, g_stream));
    HIPCHECK(hipMemcpyAsync(D.ctl, &hc0, sizeof(hc0), hipMemcpyHostToDevice, g_stream));
    HIPCHECK(hipStreamSynchronize(g_stream));
  }
  DfArgs A;
  A.ctl = D.ctl; A.queue = D.queue; A.cnt = D.cnt; A.pool = D.pool; A.slot_bytes = slot; A.times = D.times;
  A.S = S; A.nsb = nsb; A.cols = cols; A.rows = rows;
  A.range = ranges ? D.range : nullptr; A.total = (unsigned)total;
  double lim_s = 300.0;
  if (const char* e = getenv("THOR_HIP_SPIN_TIMEOUT_S")) lim_s = atof(e);
  A.spin_limit = (unsigned long long)(lim_s * 1e8);
  auto ev = ev_begin();
  if (D.kern) {
    if ((D.kern == 2 ? thor_wide_launch_u8 : thor_lat_launch_u8)(D.wgs, (void*)g_stream, jobs, &A, sizeof(A), sizeof(FrameJob<PIX>), slot)) { fprintf(stderr, "Run-time error...\nthor_hip: launch of a few-stream kernel failed\n...now exiting to system...\n"); abort(); }
  } else
    hipLaunchKernelGGL(k_superblocks<PIX>, dim3(D.wgs), dim3(kWgThreads), 0, g_stream, jobs, A);
  g_clk.sb_launches++;
  HIPCHECK(hipEventRecord(ev.second, g_stream));
  g_sb_events.push_back(ev);
  HIPCHECK(hipGetLastError());
  DfCtl hc;
  HIPCHECK(hipMemcpyAsync(&hc, D.ctl, sizeof(hc), hipMemcpyDeviceToHost, g_stream));
  if (hipError_t e = hipStreamSynchronize(g_stream)) {
    // an aborted launch: the kernel traps when a wavefront waits for another wave of its workgroup beyond kWgWaitLimit
    // (tk_block_queue.h:wg_wait_at_least - a protocol error of the block decision's work queue, never a matter of load)
    fprintf(stderr, "Run-time error...\nthor_hip: k_superblocks was aborted: %s (a trap inside the kernel = an intra-workgroup wait that did not end)\n...now exiting to system...\n",
            hipGetErrorString(e));
    abort();
  }
  const unsigned handed_out = hc.tail;
  if (hc.error || handed_out != (unsigned)total) {
    fprintf(stderr, "Run-time error...\nthor_hip: superblock scheduler failed (error %u, %u of %zu tasks released)\n...now exiting to system...\n", hc.error, handed_out, total);
    abort();
  }
  if (D.times) {
    std::vector<unsigned long long> h(3 * all);   // superblocks outside this launch's ranges: zeros
    HIPCHECK(hipMemcpy(h.data(), D.times, h.size() * 8, hipMemcpyDeviceToHost));
    FILE* f = fopen(getenv("THOR_SBTIMES"), D.frame == 0 ? "wb" : "ab");
    if (f) { int hdr[4] = {D.frame, S, nsb, cols}; fwrite(hdr, 4, 4, f); fwrite(h.data(), 8, h.size(), f); fclose(f); }
  }
  D.frame++;
}
// Engine::close: the scheduler state belongs to the engine that owns `jobs`; without this a later engine whose job
// array lands on the same device address would inherit a pool sized for another sample type.
void release_superblocks(const void* jobs) {
  auto it = g_df.find(jobs);
  if (it == g_df.end()) return;
  DfState& D = it->second;
  df_free(D);
  g_df.erase(it);
}
template <typename PIX> void run_deblock(const FrameJob<PIX>* jobs, const FrameJob<PIX>* hjobs, int S) {
  const int items = (hjobs[0].cfg.width / 8) * (hjobs[0].cfg.height / 8);
  FilterTimer timed;
  for (int pass = 0; pass < 4; pass++)
    hipLaunchKernelGGL(k_deblock<PIX>, dim3((items + 63) / 64, S), dim3(64), 0, g_stream, jobs, pass);
}
template <typename PIX> void run_make_ref(const FrameJob<PIX>* hjobs, const Plane3<PIX>* dst, int S) {
  static RefJob<PIX>* d_rj = nullptr;
  static int cap = 0;
  std::vector<RefJob<PIX>> h(S);
  for (int s = 0; s < S; s++) { h[s].rec = hjobs[s].rec; h[s].ref = dst[s]; h[s].width = hjobs[s].cfg.width; h[s].height = hjobs[s].cfg.height; }
  if (cap < S) { if (d_rj) HIPCHECK(hipFree(d_rj)); HIPCHECK(hipMalloc(&d_rj, sizeof(RefJob<PIX>) * S)); cap = S; }
  HIPCHECK(hipMemcpyAsync(d_rj, h.data(), sizeof(RefJob<PIX>) * S, hipMemcpyHostToDevice, g_stream));
  HIPCHECK(hipStreamSynchronize(g_stream));  // h goes out of scope
  const int rows = hjobs[0].cfg.height * 2 + 4 * kPadY;
  FilterTimer timed;
  hipLaunchKernelGGL(k_make_ref<PIX>, dim3(rows, S), dim3(256), 0, g_stream, d_rj);
}
template <typename PIX> void run_cdef(const CdefJob<PIX>* cj, const CdefJob<PIX>* hcj, int S) {
  const int blocks8 = (hcj[0].width / 8) * (hcj[0].height / 8);
  FilterTimer timed;
  hipLaunchKernelGGL(k_copy_planes<PIX>, dim3(hcj[0].height * 2, S), dim3(256), 0, g_stream, cj);
  hipLaunchKernelGGL((k_cdef<PIX, 0>), dim3(64, S), dim3(256), 0, g_stream, cj);
  hipLaunchKernelGGL((k_cdef<PIX, 1>), dim3((blocks8 + 63) / 64, S), dim3(64), 0, g_stream, cj);
  hipLaunchKernelGGL(k_cdef_mse<PIX>, dim3((blocks8 + 3) / 4, S), dim3(256), 0, g_stream, cj);
  hipLaunchKernelGGL(k_cdef_select<PIX>, dim3(S), dim3(1024), 0, g_stream, cj);
  hipLaunchKernelGGL((k_cdef<PIX, 4>), dim3((blocks8 + 63) / 64, S), dim3(64), 0, g_stream, cj);
}
template <typename PIX> void run_clpf_stats(const ClpfJob<PIX>* lj, const ClpfJob<PIX>* hlj, int S) {
  const int nb = (hlj[0].width / 8) * (hlj[0].height / 8) + 2 * (hlj[0].width / 16) * (hlj[0].height / 16);
  FilterTimer timed;
  hipLaunchKernelGGL(k_clpf<PIX>, dim3((nb + 63) / 64, S), dim3(64), 0, g_stream, lj, 0);
}
template <typename PIX> void run_clpf_apply(const ClpfJob<PIX>* lj, const ClpfJob<PIX>* hlj, int S) {
  const int nu = 3 * (hlj[0].width / 8) * (hlj[0].height / 8);
  FilterTimer timed;
  hipLaunchKernelGGL(k_clpf_copy<PIX>, dim3(hlj[0].height * 2, S), dim3(256), 0, g_stream, lj);
  hipLaunchKernelGGL(k_clpf<PIX>, dim3((nu + 63) / 64, S), dim3(64), 0, g_stream, lj, 1);
}
template <typename PIX> void run_interp(const idev::Job<PIX>* jobs, const idev::Job<PIX>* hjobs, int n) {
  const idev::Job<PIX>& H = hjobs[0];  // all streams share the geometry
  FilterTimer timed;
  hipLaunchKernelGGL(k_interp_clear<PIX>, dim3(64, n), dim3(256), 0, g_stream, jobs);
  for (int l = 1; l < H.levels; l++) {
    const int total = ((H.height >> l) + 64) * ((H.width >> l) + 64);
    hipLaunchKernelGGL(k_interp_down<PIX>, dim3((total + 255) / 256, n), dim3(256), 0, g_stream, jobs, l);
  }
  for (int lvl = H.levels - 1; lvl >= 0; --lvl) {
    const idev::Level<PIX>& L = H.lv[lvl];
    hipLaunchKernelGGL(k_interp_estimate<PIX>, dim3(L.bh / idev::kStep, n), dim3(64), 0, g_stream, jobs, lvl);
    const int units = L.bw * L.bh;
    hipLaunchKernelGGL(k_interp_merge<PIX>, dim3(units < 16384 ? units : 16384, n), dim3(64), 0, g_stream, jobs, lvl);
    if (lvl > 0) {
      const int fine = H.lv[lvl - 1].bw * H.lv[lvl - 1].bh;
      hipLaunchKernelGGL(k_interp_upscale<PIX>, dim3((fine + 255) / 256, n), dim3(256), 0, g_stream, jobs, lvl);
    } else {
      hipLaunchKernelGGL(k_interp_mc<PIX>, dim3(units < 16384 ? units : 16384, n), dim3(64), 0, g_stream, jobs);
      const int rows = H.height + 2 * kPadY + 2 * (H.height / 2 + kPadY);
      hipLaunchKernelGGL(k_interp_pad<PIX>, dim3(rows, n), dim3(256), 0, g_stream, jobs);
    }
  }
}
// Written out, here and below, rather than TK_BACKEND_INSTANTIATE (tk_encoder.h): the order of these instantiations is the order of the kernels in the
// code object, and scripts/device_code_same.sh compares that with earlier states of the unit.
template void run_interp<uint8_t>(const idev::Job<uint8_t>*, const idev::Job<uint8_t>*, int);
template void run_interp<uint16_t>(const idev::Job<uint16_t>*, const idev::Job<uint16_t>*, int);
void run_gather(const GatherItem* d_items, int n, uint32_t* dst) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gather_bits, dim3(n), dim3(64), 0, g_stream, d_items, n, dst);
  HIPCHECK(hipGetLastError());
}
template void run_superblocks<uint8_t>(const FrameJob<uint8_t>*, const FrameJob<uint8_t>*, int, const SbRange*);
template void run_deblock<uint8_t>(const FrameJob<uint8_t>*, const FrameJob<uint8_t>*, int);
template void run_make_ref<uint8_t>(const FrameJob<uint8_t>*, const Plane3<uint8_t>*, int);
template void run_cdef<uint8_t>(const CdefJob<uint8_t>*, const CdefJob<uint8_t>*, int);
template void run_superblocks<uint16_t>(const FrameJob<uint16_t>*, const FrameJob<uint16_t>*, int, const SbRange*);
template void run_clpf_stats<uint8_t>(const ClpfJob<uint8_t>*, const ClpfJob<uint8_t>*, int);
template void run_clpf_stats<uint16_t>(const ClpfJob<uint16_t>*, const ClpfJob<uint16_t>*, int);
template void run_clpf_apply<uint8_t>(const ClpfJob<uint8_t>*, const ClpfJob<uint8_t>*, int);
template void run_clpf_apply<uint16_t>(const ClpfJob<uint16_t>*, const ClpfJob<uint16_t>*, int);
template void run_deblock<uint16_t>(const FrameJob<uint16_t>*, const FrameJob<uint16_t>*, int);
template void run_make_ref<uint16_t>(const FrameJob<uint16_t>*, const Plane3<uint16_t>*, int);
template void run_cdef<uint16_t>(const CdefJob<uint16_t>*, const CdefJob<uint16_t>*, int);
}  // namespace backend

// jobs: device array of S FrameJob (orig, rec, geometry); out: device, 4 slots per stream, cleared by the caller on g_stream.
// Up to 64 four-wavefront workgroups per stream (2 * height rows: Y, U, V).
template <typename PIX> void launch_frame_sse(const FrameJob<PIX>* jobs, const FrameJob<PIX>* hjobs, int S, unsigned long long* out) {
  if (S <= 0) return;
  const int rows = 2 * hjobs[0].cfg.height;
  const int blocks = (rows + 3) / 4 < 64 ? (rows + 3) / 4 : 64;
  hipLaunchKernelGGL(k_frame_sse<PIX>, dim3(blocks, S), dim3(256), 0, g_stream, jobs, out);
  HIPCHECK(hipGetLastError());
}
template void launch_frame_sse<uint8_t>(const FrameJob<uint8_t>*, const FrameJob<uint8_t>*, int, unsigned long long*);
template void launch_frame_sse<uint16_t>(const FrameJob<uint16_t>*, const FrameJob<uint16_t>*, int, unsigned long long*);

// Input at a lower bit depth than the engine's: the three frame-level kernels on g_stream (tk_encoder.h declares them).  `packed`: a packed planar
// 4:2:0 frame of input-depth samples in device memory, one byte per sample for depth 8 and two otherwise, 16-byte aligned.
static dim3 depth_grid(int height) { return dim3((2 * height + 3) / 4); }   // Y, U and V rows, four wavefronts per workgroup
void launch_depth_up(const void* packed, const Plane3<uint16_t>& dst, int width, int height, int bitdepth, int input_bitdepth) {
  const int shift = bitdepth - input_bitdepth;
  if (input_bitdepth == 8) hipLaunchKernelGGL(k_depth_up<uint8_t>, depth_grid(height), dim3(256), 0, g_stream, (const uint8_t*)packed, dst, width, height, shift);
  else hipLaunchKernelGGL(k_depth_up<uint16_t>, depth_grid(height), dim3(256), 0, g_stream, (const uint16_t*)packed, dst, width, height, shift);
  HIPCHECK(hipGetLastError());
}
void launch_depth_down(const Plane3<uint16_t>& src, void* packed, int width, int height, int bitdepth, int input_bitdepth) {
  const int shift = bitdepth - input_bitdepth;
  if (input_bitdepth == 8) hipLaunchKernelGGL(k_depth_down<uint8_t>, depth_grid(height), dim3(256), 0, g_stream, src, (uint8_t*)packed, width, height, shift, input_bitdepth);
  else hipLaunchKernelGGL(k_depth_down<uint16_t>, depth_grid(height), dim3(256), 0, g_stream, src, (uint16_t*)packed, width, height, shift, input_bitdepth);
  HIPCHECK(hipGetLastError());
}
void launch_frame_sse_depth(const FrameJob<uint16_t>* jobs, const FrameJob<uint16_t>* hjobs, int S, int bitdepth, int input_bitdepth, unsigned long long* out) {
  if (S <= 0) return;
  const int rows = 2 * hjobs[0].cfg.height;
  const int blocks = (rows + 3) / 4 < 64 ? (rows + 3) / 4 : 64;
  hipLaunchKernelGGL(k_frame_sse_depth, dim3(blocks, S), dim3(256), 0, g_stream, jobs, bitdepth - input_bitdepth, input_bitdepth, out);
  HIPCHECK(hipGetLastError());
}

// A frame in a caller's layout <-> the engine's planes, on g_stream (tk_encoder.h declares them).  `frame`: device memory, L.bytes of it.
static dim3 layout_grid(int height) { return dim3((height + height / 2 + 3) / 4); }   // luma rows and chroma rows, four wavefronts per workgroup
template <typename PIX> void launch_layout_in(const void* frame, const PixLayout& L, const Plane3<PIX>& dst, int width, int height, int bitdepth, int input_bitdepth) {
  const int up = bitdepth - input_bitdepth;
  if constexpr (sizeof(PIX) == 1) hipLaunchKernelGGL((k_layout_in<uint8_t, uint8_t>), layout_grid(height), dim3(256), 0, g_stream, frame, L, dst, width, height, up);
  else if (input_bitdepth == 8) hipLaunchKernelGGL((k_layout_in<uint8_t, uint16_t>), layout_grid(height), dim3(256), 0, g_stream, frame, L, dst, width, height, up);
  else hipLaunchKernelGGL((k_layout_in<uint16_t, uint16_t>), layout_grid(height), dim3(256), 0, g_stream, frame, L, dst, width, height, up);
  HIPCHECK(hipGetLastError());
}
template <typename PIX> void launch_layout_out(const Plane3<PIX>& src, void* frame, const PixLayout& L, int width, int height, int bitdepth, int input_bitdepth) {
  const int shift = bitdepth - input_bitdepth;
  if constexpr (sizeof(PIX) == 1) hipLaunchKernelGGL((k_layout_out<uint8_t, uint8_t>), layout_grid(height), dim3(256), 0, g_stream, src, frame, L, width, height, shift, input_bitdepth);
  else if (input_bitdepth == 8) hipLaunchKernelGGL((k_layout_out<uint16_t, uint8_t>), layout_grid(height), dim3(256), 0, g_stream, src, frame, L, width, height, shift, input_bitdepth);
  else hipLaunchKernelGGL((k_layout_out<uint16_t, uint16_t>), layout_grid(height), dim3(256), 0, g_stream, src, frame, L, width, height, shift, input_bitdepth);
  HIPCHECK(hipGetLastError());
}
template void launch_layout_in<uint8_t>(const void*, const PixLayout&, const Plane3<uint8_t>&, int, int, int, int);
template void launch_layout_in<uint16_t>(const void*, const PixLayout&, const Plane3<uint16_t>&, int, int, int, int);
template void launch_layout_out<uint8_t>(const Plane3<uint8_t>&, void*, const PixLayout&, int, int, int, int);
template void launch_layout_out<uint16_t>(const Plane3<uint16_t>&, void*, const PixLayout&, int, int, int, int);

// An RGB frame <-> the engine's planes, on g_stream (tk_encoder.h declares them).  `frame`: device memory, R.bytes of it.  The 8-bit engine exists
// only for bitdepth == input_bitdepth == 8; the RGB side has one or two bytes per sample with either engine.
template <typename PIX> void launch_rgb_in(const void* frame, const RgbFormat& R, const Plane3<PIX>& dst, int width, int height, int bitdepth, int input_bitdepth) {
  const int up = bitdepth - input_bitdepth;
  if (R.sbytes == 1) hipLaunchKernelGGL((k_rgb_in<uint8_t, PIX>), dim3(height / 2), dim3(256), 0, g_stream, frame, R, dst, width, height, up);
  else hipLaunchKernelGGL((k_rgb_in<uint16_t, PIX>), dim3(height / 2), dim3(256), 0, g_stream, frame, R, dst, width, height, up);
  HIPCHECK(hipGetLastError());
}
template <typename PIX> void launch_rgb_out(const Plane3<PIX>& src, void* frame, const RgbFormat& R, int width, int height, int bitdepth, int input_bitdepth) {
  const int shift = bitdepth - input_bitdepth;
  if (R.sbytes == 1) hipLaunchKernelGGL((k_rgb_out<PIX, uint8_t>), dim3(height / 2), dim3(256), 0, g_stream, src, frame, R, width, height, shift);
  else hipLaunchKernelGGL((k_rgb_out<PIX, uint16_t>), dim3(height / 2), dim3(256), 0, g_stream, src, frame, R, width, height, shift);
  HIPCHECK(hipGetLastError());
}
template void launch_rgb_in<uint8_t>(const void*, const RgbFormat&, const Plane3<uint8_t>&, int, int, int, int);
template void launch_rgb_in<uint16_t>(const void*, const RgbFormat&, const Plane3<uint16_t>&, int, int, int, int);
template void launch_rgb_out<uint8_t>(const Plane3<uint8_t>&, void*, const RgbFormat&, int, int, int, int);
template void launch_rgb_out<uint16_t>(const Plane3<uint16_t>&, void*, const RgbFormat&, int, int, int, int);

// A frame of another size -> the engine's planes, on g_stream (tk_encoder.h declares it).  `frame`: device memory in layout L at the source size;
// `tab`: the plan's tables in device memory; `vrows`: the most source rows one tile reaches (ScaleAxisTable::span of the two vertical tables).
template <typename PIX> void launch_scale_in(const void* frame, const PixLayout& L, const ScaleTables& tab, int vrows, const Plane3<PIX>& dst, int src_w, int width,
                                             int height, int bitdepth, int input_bitdepth) {
  const int up = bitdepth - input_bitdepth, maxv = (1 << input_bitdepth) - 1;
  const dim3 grid(scale_items(width, height));
  const size_t lds = (size_t)vrows * SCALE_TW * sizeof(int16_t);
  if (vrows < 1 || vrows > SCALE_VROWS) { fprintf(stderr, "launch_scale_in: %d intermediate rows\n", vrows); abort(); }
  if constexpr (sizeof(PIX) == 1) hipLaunchKernelGGL((k_scale_in<uint8_t, uint8_t>), grid, dim3(256), lds, g_stream, frame, L, tab, dst, src_w, width, height, maxv, up);
  else if (input_bitdepth == 8) hipLaunchKernelGGL((k_scale_in<uint8_t, uint16_t>), grid, dim3(256), lds, g_stream, frame, L, tab, dst, src_w, width, height, maxv, up);
  else hipLaunchKernelGGL((k_scale_in<uint16_t, uint16_t>), grid, dim3(256), lds, g_stream, frame, L, tab, dst, src_w, width, height, maxv, up);
  HIPCHECK(hipGetLastError());
}
template void launch_scale_in<uint8_t>(const void*, const PixLayout&, const ScaleTables&, int, const Plane3<uint8_t>&, int, int, int, int, int);
template void launch_scale_in<uint16_t>(const void*, const PixLayout&, const ScaleTables&, int, const Plane3<uint16_t>&, int, int, int, int, int);

// The frame analysis of rate control for n streams of one size, on g_stream (tk_encoder.h declares it): one workgroup per tile of the half-size plane.
template <typename PIX> void launch_rc_cost(const RcJob<PIX>* jobs, const RcJob<PIX>* hjobs, int n) {
  if (n <= 0) return;
  const int tiles = ((hjobs[0].hw + RC_TILE - 1) / RC_TILE) * ((hjobs[0].hh + RC_TILE - 1) / RC_TILE);
  hipLaunchKernelGGL((k_rc_cost<PIX, false>), dim3(tiles, n), dim3(256), 0, g_stream, jobs);
  HIPCHECK(hipGetLastError());
}
template void launch_rc_cost<uint8_t>(const RcJob<uint8_t>*, const RcJob<uint8_t>*, int);
template void launch_rc_cost<uint16_t>(const RcJob<uint16_t>*, const RcJob<uint16_t>*, int);
// The same analysis against previous ORIGINALS (RcJob::prev_y; thor_hip_scene_cost): the kernel's other instantiation, which stores nothing but the sums.
template <typename PIX> void launch_rc_cost_orig(const RcJob<PIX>* jobs, const RcJob<PIX>* hjobs, int n) {
  if (n <= 0) return;
  const int tiles = ((hjobs[0].hw + RC_TILE - 1) / RC_TILE) * ((hjobs[0].hh + RC_TILE - 1) / RC_TILE);
  hipLaunchKernelGGL((k_rc_cost<PIX, true>), dim3(tiles, n), dim3(256), 0, g_stream, jobs);
  HIPCHECK(hipGetLastError());
}
template void launch_rc_cost_orig<uint8_t>(const RcJob<uint8_t>*, const RcJob<uint8_t>*, int);
template void launch_rc_cost_orig<uint16_t>(const RcJob<uint16_t>*, const RcJob<uint16_t>*, int);
// The temporal filter of n requests of one size, on g_stream (tk_encoder.h declares it): the search of every neighbour of every request in one launch, the
// blend of every request in the next; the stream orders them.  The caller synchronises once.
template <typename PIX> void launch_tf(const TfJob<PIX>* jobs, const TfJob<PIX>* hjobs, int n) {
  if (n <= 0) return;
  const int tiles = ((hjobs[0].width + TF_TILE - 1) / TF_TILE) * ((hjobs[0].height + TF_TILE - 1) / TF_TILE);
  int refs = 0;
  for (int i = 0; i < n; i++) refs = hjobs[i].nrefs > refs ? hjobs[i].nrefs : refs;
  if (refs) hipLaunchKernelGGL((k_tf_search<PIX>), dim3(tiles, refs, n), dim3(256), 0, g_stream, jobs);
  hipLaunchKernelGGL((k_tf_blend<PIX>), dim3(tiles, n), dim3(256), 0, g_stream, jobs);
  HIPCHECK(hipGetLastError());
}
template void launch_tf<uint8_t>(const TfJob<uint8_t>*, const TfJob<uint8_t>*, int);
template void launch_tf<uint16_t>(const TfJob<uint16_t>*, const TfJob<uint16_t>*, int);

// ---- helpers of the C ABI (internal linkage: the library exports nothing of them) -----------------------------------------
namespace {
// Owning device array of n elements, zeroed (dev_alloc clears), filled from `h` when given; freed with its scope.
template <typename T> struct DevBuf {
  T* p;
  explicit DevBuf(size_t n, const T* h = nullptr) : p((T*)backend::dev_alloc(n * sizeof(T))) { if (h) backend::h2d(p, h, n * sizeof(T)); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { backend::dev_free(p); }
  T* get() const { return p; }
  operator T*() const { return p; }
};
// The planes of a 4:2:0 frame in device memory against a packed frame (Y, U, V one after the other, no row padding):
// copy(device plane, its stride, offset of the plane in the packed frame, width, rows), all in samples.
template <typename PIX, typename F> void for_yuv_planes(const Plane3<PIX>& p, int w, int h, F copy) {
  const size_t ny = (size_t)w * h, nc = (size_t)(w / 2) * (h / 2);
  copy(p.y, p.sy, (size_t)0, w, h);
  copy(p.u, p.sc, ny, w / 2, h / 2);
  copy(p.v, p.sc, ny + nc, w / 2, h / 2);
}
template <typename PIX> void upload_yuv(DevFrame<PIX>& f, const PIX* yuv, int w, int h) {
  const size_t B = sizeof(PIX);
  for_yuv_planes(f.p, w, h, [&](PIX* d, int ds, size_t off, int pw, int ph) { HIPCHECK(hipMemcpy2D(d, ds * B, yuv + off, pw * B, pw * B, ph, hipMemcpyHostToDevice)); });
}
template <typename PIX> void download_yuv(const DevFrame<PIX>& f, PIX* yuv, int w, int h) {
  const size_t B = sizeof(PIX);
  for_yuv_planes(f.p, w, h, [&](const PIX* d, int ds, size_t off, int pw, int ph) { HIPCHECK(hipMemcpy2D(yuv + off, pw * B, d, ds * B, pw * B, ph, hipMemcpyDeviceToHost)); });
}
}  // namespace
}  // namespace tk
