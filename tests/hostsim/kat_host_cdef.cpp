// kat_host_cdef.cpp - TEST INFRASTRUCTURE ONLY.  The 1-lane host build of the five CDEF passes (thor_amd/csrc/tk_cdef.h) in the order backend::run_cdef
// launches them - copy, cdef_pass_flags, cdef_pass_dir, cdef_mse_block_wave per 8x8 block (the wavefront form with its lanes as a loop; skipped like
// k_cdef_mse when cdef_bits is 0), cdef_pass_select with a one-thread team, cdef_pass_apply - behind the arguments of thor_hip_kat_cdef_frame
// (include/thor_hip.h), so that tests/golden/kat10.npz (recorded from the reference's cdef_search + cdef_frame, tests/golden/gen_kat10.py) pins the source on
// the CPU (tests/test_kat_host_cdef.py).  What only exists on the device - the packed dot-product builtins, the LDS row pitch, four wavefronts per
// workgroup, the 1024-thread barrier - is what tests/test_gpu_cdef.py adds with the same fixture.
#include <math.h>
#include "../../thor_amd/csrc/tk_cdef.h"
#include <cstring>
#include <vector>
namespace tk { Tables g_tab; }
using namespace tk;

template <typename PIX>
static int run(int S, const PIX* rec_yuv, const PIX* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, const int* qp, const int* speed, const int* cdef_bits,
               int8_t* dir, int* var, int* fb_compact, unsigned long long* mse, int* res, int* fb_sel, PIX* out_yuv) {
  if (S <= 0 || width < 8 || height < 8 || width % 8 || height % 8) return 1;
  const int nfb_h = (width + 63) / 64, nfb_v = (height + 63) / 64, nfb = nfb_h * nfb_v, nb8 = (width / 8) * (height / 8);
  const size_t ny = (size_t)width * height, nc = ny / 4, fsz = ny + 2 * nc, ncell = (size_t)(width / 4) * (height / 4);
  static CdefWaveWs<PIX> ws;
  for (int s = 0; s < S; s++) {
    if (speed[s] < 0 || speed[s] > 2 || cdef_bits[s] < 0 || cdef_bits[s] > 3 || qp[s] < 0 || qp[s] > 51) return 1;
    std::vector<PIX> src(rec_yuv + fsz * s, rec_yuv + fsz * (s + 1)), org(org_yuv + fsz * s, org_yuv + fsz * (s + 1));
    PIX* out = out_yuv + fsz * s;
    memcpy(out, src.data(), fsz * sizeof(PIX));   // k_copy_planes: the passes read `src`, cdef_pass_apply overwrites the filtered blocks of `rec`
    std::vector<DbCell> cells(ncell);
    memset(cells.data(), 0, ncell * sizeof(DbCell));
    for (size_t i = 0; i < ncell; i++) { cells[i].mode = mode[ncell * s + i]; cells[i].size = 8; }
    auto planes = [&](PIX* p) { Plane3<PIX> q; q.y = p; q.u = p + ny; q.v = p + ny + nc; q.sy = width; q.sc = width / 2; return q; };
    std::vector<int> sel(nfb, 0);
    std::vector<unsigned long long> tot((size_t)kCdefMaxStr * kCdefMaxStr + nfb, 0);
    CdefResult R;
    memset(&R, 0, sizeof(R));
    CdefJob<PIX> J;
    memset(&J, 0, sizeof(J));
    J.rec = planes(out); J.src = planes(src.data()); J.org = planes(org.data());
    J.width = width; J.height = height; J.bitdepth = bitdepth;
    J.cells = cells.data(); J.cs = width / 4; J.nfb_h = nfb_h; J.nfb_v = nfb_v;
    J.speed = speed[s]; J.damping = 5; J.cdef_bits = cdef_bits[s]; J.qp = qp[s];
    J.dir = dir + (size_t)nb8 * s; J.var = var + (size_t)nb8 * s; J.fb_compact = fb_compact + (size_t)nfb * s;
    J.mse = mse + (size_t)2 * nfb * kCdefMaxStr * s; J.sel = sel.data(); J.fb_sel = fb_sel + (size_t)nfb * s;
    J.res = &R; J.tot = tot.data();
    memset(J.dir, 0, nb8); memset(J.var, 0, nb8 * sizeof(int));
    const Team t = mk_team(0, 1);
    cdef_pass_flags(J, 0, 1);
    cdef_pass_dir(J, 0, 1);
    if (J.cdef_bits)
      for (int b = 0; b < nb8; b++) cdef_mse_block_wave(t, J, b, &ws);
    cdef_pass_select(t, J);
    cdef_pass_apply(J, 0, 1);
    memcpy(res + (sizeof(CdefResult) / sizeof(int)) * s, &R, sizeof(R));
  }
  return 0;
}

extern "C" int h_cdef_frame(int n_jobs, const void* rec_yuv, const void* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, const int* qp, const int* speed,
                            const int* cdef_bits, int8_t* dir, int* var, int* fb_compact, unsigned long long* mse, int* result, int* fb_sel, void* out_yuv) {
  if (bitdepth == 8)
    return run<uint8_t>(n_jobs, (const uint8_t*)rec_yuv, (const uint8_t*)org_yuv, mode, width, height, 8, qp, speed, cdef_bits, dir, var, fb_compact, mse, result, fb_sel, (uint8_t*)out_yuv);
  if (bitdepth < 9 || bitdepth > 12) return 1;
  return run<uint16_t>(n_jobs, (const uint16_t*)rec_yuv, (const uint16_t*)org_yuv, mode, width, height, bitdepth, qp, speed, cdef_bits, dir, var, fb_compact, mse, result, fb_sel,
                       (uint16_t*)out_yuv);
}
