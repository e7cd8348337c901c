// thor_hip.cpp - libthor_hip.so: gfx950 kernels, device backend and the C ABI (include/thor_hip.h).
// One workgroup of 4 wavefronts encodes one 128x128 superblock at a time (wave 0 walks the quadtree, all four share the
// trials of each block decision); one persistent, dependency-driven launch per frame covers every superblock of every stream (SB(k,l) needs (k,l-1) and
// (k-1,l+1)).  There is NO CPU path in this library: every entry point that computes aborts if no
// HIP device is usable (thor_hip_open reports it by returning NULL).
// This file is the ONE translation unit of the throughput build (a kernel can only be launched from the unit that defines it: the library is built
// without relocatable device code).  Its parts, by role, are the hip_*.h headers included at the end - device-only, never part of the host simulation:
//   hip_kernels.h   the frame-level __global__ kernels (the superblock kernel itself is tk_kernel.h)
//   hip_backend.h   device initialisation, namespace backend (memory, scheduler state, every run_* launch sequence), host <-> device helpers
//   hip_abi_seq.h   the sequence API of include/thor_hip.h
//   hip_abi_seam.h  the drop-in seam of include/thor_abi.h (encode_frame_lbd / _hbd)
//   hip_kat.h       the known-answer kernels and their entry points (the two block-syntax kernels: thor_hip_katbits.cpp), thor_hip_superblock_kernel_info / _in_use
// The order of the includes is the order in which kernels are defined and templates instantiated, i.e. the order of the code object: keep it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>

#include "tk_block.h"
#include "tk_filters.h"
#include "tk_cdef.h"
#include "tk_clpf.h"
#include "tk_encoder.h"
#include "tk_cli.h"
#include "tk_sched.h"
#include "tk_kernel.h"
#include "../../include/thor_hip.h"
#include "../../include/thor_abi.h"

#define HIPCHECK(x)                                                                              \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess) {                                                                      \
      fprintf(stderr, "Run-time error...\nthor_hip: %s failed: %s (%s:%d)\n...now exiting to system...\n", #x, \
              hipGetErrorString(e_), __FILE__, __LINE__);                                        \
      abort();                                                                                   \
    }                                                                                            \
  } while (0)

// the second build of the engine (thor_hip_lat.cpp: 256 VGPRs, two workgroups per CU - the few-stream operating point)
#define TK_ALT_DECLS(P)                                                                                                                  \
  extern "C" __attribute__((visibility("hidden"))) int P##upload_tables(const void* tables, size_t bytes);                                 \
  extern "C" __attribute__((visibility("hidden"))) int P##workgroups_per_cu(void);                                                         \
  extern "C" __attribute__((visibility("hidden"))) int P##waves(void);                                                                     \
  extern "C" __attribute__((visibility("hidden"))) int P##kernel_info(int* num_regs, int* lds_bytes, int* private_bytes);                  \
  extern "C" __attribute__((visibility("hidden"))) int P##launch_u8(int wgs, void* stream, const void* jobs, const void* dfargs, size_t dfargs_bytes, size_t job_bytes, size_t slot_bytes);
TK_ALT_DECLS(thor_lat_)    // thor_hip_lat.cpp: 256 VGPRs, two four-wave workgroups per CU
TK_ALT_DECLS(thor_wide_)   // thor_hip_wide.cpp: eight-wave workgroups, one per CU
// thor_hip_katbits.cpp: the known-answer kernels of the block syntax (device pointers throughout)
extern "C" __attribute__((visibility("hidden"))) int thor_katbits_upload_tables(const void* tables, size_t bytes);
extern "C" __attribute__((visibility("hidden"))) int thor_katbits_launch_coeff(void* stream, int n, const int* par, const int16_t* coef, int words, uint32_t* buf_single, uint32_t* buf_team, int* out);
extern "C" __attribute__((visibility("hidden"))) int thor_katbits_launch_block(void* stream, int n, const int* par, const int16_t* coef, int words, uint32_t* buf_coop, uint32_t* buf_single, int* out);


namespace tk {
__device__ Tables g_tab;
}

#include "hip_kernels.h"
#include "hip_backend.h"
#include "hip_abi_seq.h"
#include "hip_abi_seam.h"
#include "hip_kat.h"
#include "hip_kat_block.h"
