// unit_report.cpp - TEST INFRASTRUCTURE ONLY.  Prints the encoder report (thor_amd/csrc/tk_report.h) of small synthetic frame
// logs for tests/test_frame_report.py: an exact match (sse 0 -> inf), frames without measured distortion (-snrcalc 0), the
// padding of short reference lists up to max_num_ref and the I(a,b) entries of an interpolated reference, the -stat line.
#include "../../thor_amd/csrc/tk_report.h"

int main() {
  using namespace tk;
  std::vector<FrameStat> log(3);
  log[0].display = 0; log[0].frame_type = 0; log[0].qp = 30; log[0].num_bits = 1000; log[0].has_sse = 1;  // sse 0: inf
  log[1].display = 4; log[1].frame_type = 1; log[1].qp = 32; log[1].num_bits = 200; log[1].num_ref = 1; log[1].has_sse = 1;
  log[1].ref_frame_num[0] = 0; log[1].sse[0] = 1234567; log[1].sse[1] = 89; log[1].sse[2] = 1;
  log[2].display = 2; log[2].frame_type = 2; log[2].qp = 36; log[2].num_bits = 50; log[2].num_ref = 3;   // not measured: zeros
  const int ra[3] = {-1, 1, 0}, fn[3] = {-1, 0, 4};
  for (int k = 0; k < 3; k++) { log[2].ref_array[k] = ra[k]; log[2].ref_frame_num[k] = fn[k]; }
  fputs(format_report(log, 58, 4, 30.f, 64, 32, 8).c_str(), stdout);
  fputs(format_stat_line(log, 58, 30.f, 64, 32, 8, 3).c_str(), stdout);
  std::vector<FrameStat> one(1);
  one[0].has_sse = 1; one[0].sse[0] = 4095ull * 4095ull * 64 * 32; one[0].sse[1] = 1; one[0].sse[2] = 2;
  fputs(format_report(one, 60, 1, 60.f, 64, 32, 12).c_str(), stdout);
  return 0;
}
