// kat_host_interp.cpp - TEST INFRASTRUCTURE ONLY.  The host build of the temporally interpolated reference behind the arguments of
// thor_hip_kat_interp_stages (include/thor_hip.h): the translation unit of hostsim.cpp (its main() renamed) supplies the host backend - plain memory, and
// run_interp with 1-lane teams, block rows in raster order - and thor_amd/csrc/tk_kat_interp.h the very statements the device entry point runs
// (Engine::open, make_ref, Engine::make_interp_frames, the copies back).  tests/golden/kat12*.npz (recorded from the reference's temporal_interp.c stage by
// stage, tests/golden/gen_kat12.py) thereby pins thor_amd/csrc/tk_interp_dev.h on the CPU (tests/test_kat_host_interp.py).  What only exists on the device -
// the 64-lane team_sum, one wavefront per block row kept two blocks behind the row above (ticket dispenser, progress counters, acquire / release), the launch
// geometry, blockIdx.y as the stream - is what tests/test_gpu_interp.py adds with the same fixture.
#define main hostsim_main
#include "hostsim.cpp"
#undef main
#include "../../thor_amd/csrc/tk_kat_interp.h"

extern "C" int h_interp_stages(int n_streams, const void* yuv0, const void* yuv1, int width, int height, int bitdepth, int levels, void* pyramid, int16_t* nmv,
                               void* out_padded) {
  static bool tables = false;
  if (!tables) { tk::init_tables(&tk::g_tab); tables = true; }
  if (bitdepth == 8)
    return tk::kat_interp_stages<uint8_t>(n_streams, (const uint8_t*)yuv0, (const uint8_t*)yuv1, width, height, 8, levels, (uint8_t*)pyramid, nmv, (uint8_t*)out_padded);
  if (bitdepth < 9 || bitdepth > 12) return 1;
  return tk::kat_interp_stages<uint16_t>(n_streams, (const uint16_t*)yuv0, (const uint16_t*)yuv1, width, height, bitdepth, levels, (uint16_t*)pyramid, nmv,
                                         (uint16_t*)out_padded);
}
