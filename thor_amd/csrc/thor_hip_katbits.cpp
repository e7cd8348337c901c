// thor_hip_katbits.cpp - the known-answer kernels of the block syntax writer and its bit counter (tk_bits.h) behind thor_hip_kat_coeff_syntax /
// thor_hip_kat_block_syntax (hip_kat.h).  The engine sources compiled with the throughput build's parameters (TK_OCC, TK_WAVES: the defaults) in a translation unit
// of their own, namespace tk_katbits, with its own copy of the constant tables - NOT inside thor_hip.cpp like the other known-answer kernels: bs_block_t,
// bs_coeff_team, bs_coeff and coeff_bits_team are internal __noinline__ functions whose code the compiler specialises for the call sites it sees, and call sites
// with other constant arguments (a null team, emit == 0 into an emitting instance) in the same unit changed the code of 43 functions of the superblock kernels,
// register allocation of k_superblocks included (per-function diff of the gfx950 assembly).  Here the product's unit stays byte for byte what it was.  What these kernels pin on the device is therefore a
// SECOND compilation of tk_bits.h (same source, same flags and parameters), not the code objects k_superblocks calls: the product's own binary of bs_block_t /
// coeff_bits_team / bs_coeff_team stays covered by the stream goldens (tests/test_gpu_parity.py, test_gpu_fullsize.py) only.
#define tk tk_katbits
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "tk_kernel.h"
#include "tk_kat_bits.h"

namespace tk {
__device__ Tables g_tab;
// ---- the block syntax writer and its bit counter (tk_bits.h): one workgroup of one wavefront per item through tk_kat_bits.h, with the superblock kernel's LDS
// workspace (WgShared: the scan tables the teams read, SmallWs: the coefficient buffers of a trial) - coefficient buffers in LDS take the SP_LDS instances, the
// item's own copy in global memory the SP_GLOBAL ones (in the product: the chroma buffers of tb-split 64 / 128 blocks, BigWs).  bs_block_t, bs_coeff_team,
// bs_coeff and coeff_bits_team are __noinline__ functions the superblock kernel calls too, so these kernels carry its launch bounds (as k_kat_inter_yuv in hip_kat.h does, which says why).
__global__ __launch_bounds__(kWgThreads, (int)kOcc) void k_kat_coeff_syntax(const int* par, const int16_t* coef, int words, uint32_t* buf_single, uint32_t* buf_team, int* out) {
  __shared__ WgShared sh;
  __shared__ SmallWs<uint8_t> sws;
  const int lane = (int)threadIdx.x, it = (int)blockIdx.x;
  const Team t = mk_team(lane, 64, sh.tabs.izz);
  xform_tables_fill(&sh.tabs, lane, 64);
  const int16_t* g = coef + (size_t)it * 256;
  for (int k = lane; k < 256; k += 64) sws.coef_y[k] = g[k];
  __syncthreads();
  kat_coeff_item(t, par + kKatCoPar * it, sws.coef_y, g, buf_single + (size_t)it * words, buf_team + (size_t)it * words, out + kKatCoOut * it);
}
__global__ __launch_bounds__(kWgThreads, (int)kOcc) void k_kat_block_syntax(const int* par, const int16_t* coef, int words, uint32_t* buf_coop, uint32_t* buf_single, int* out) {
  __shared__ WgShared sh;
  __shared__ SmallWs<uint8_t> sws;
  const int lane = (int)threadIdx.x, it = (int)blockIdx.x;
  const Team t = mk_team(lane, 64, sh.tabs.izz);
  xform_tables_fill(&sh.tabs, lane, 64);
  const int* q = par + kKatBlPar * it;
  const int16_t* g = coef + (size_t)it * 3072;
  // SmallWs holds 256 chroma coefficients per plane: everything but the four 16x16 units of a tb-split 64 / 128 block (tk_block_rd.h: bigc)
  const int fits = __builtin_amdgcn_readfirstlane(!(q[0] == 0 && q[25] && q[9] >= 64));
  for (int k = lane; k < 1024; k += 64) sws.coef_y[k] = g[k];
  if (fits)
    for (int k = lane; k < 256; k += 64) { sws.coef_u[k] = g[1024 + k]; sws.coef_v[k] = g[2048 + k]; }
  __syncthreads();
  kat_block_item(t, q, sws.coef_y, fits ? sws.coef_u : nullptr, fits ? sws.coef_v : nullptr, g, g + 1024, g + 2048, words * 32, buf_coop + (size_t)it * words,
                 buf_single + (size_t)it * words, out + kKatBlOut * it);
}
}  // namespace tk

#define TK_INTERNAL __attribute__((visibility("hidden")))
extern "C" {
// (internal to libthor_hip.so: hidden symbols, called only by thor_hip.cpp; every pointer is a device pointer)
TK_INTERNAL int thor_katbits_upload_tables(const void* tables, size_t bytes) {
  if (bytes != sizeof(tk::Tables)) return 1;
  return hipMemcpyToSymbol(HIP_SYMBOL(tk::g_tab), tables, bytes) == hipSuccess ? 0 : 2;
}
TK_INTERNAL int thor_katbits_launch_coeff(void* stream, int n, const int* par, const int16_t* coef, int words, uint32_t* buf_single, uint32_t* buf_team, int* out) {
  hipLaunchKernelGGL(tk::k_kat_coeff_syntax, dim3(n), dim3(64), 0, (hipStream_t)stream, par, coef, words, buf_single, buf_team, out);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
TK_INTERNAL int thor_katbits_launch_block(void* stream, int n, const int* par, const int16_t* coef, int words, uint32_t* buf_coop, uint32_t* buf_single, int* out) {
  hipLaunchKernelGGL(tk::k_kat_block_syntax, dim3(n), dim3(64), 0, (hipStream_t)stream, par, coef, words, buf_coop, buf_single, out);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
}
