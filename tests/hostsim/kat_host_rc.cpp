// kat_host_rc.cpp - TEST INFRASTRUCTURE ONLY.
// The frame analysis of rate control (thor_amd/csrc/tk_rc.h: the TK_DEV block functions k_rc_cost runs) compiled for the host with one lane, in the
// launch sequence of thor_hip_kat_rc_cost: the previous frame first, without a previous plane, then the current one against what that wrote.
//   kat_host_rc <w> <h> <bitdepth> <has_prev> <in> <out>
// in: the current luma plane, then (has_prev) the previous one, w x h samples each (bytes for bitdepth 8, uint16_t above).
// out: sum_intra, sum_best, n_intra as three uint64_t, then the current frame's half-size plane.
#include "../../thor_amd/csrc/tk_rc.h"
#include <vector>

template <typename PIX> static int run(int w, int h, int has_prev, FILE* fi, FILE* fo) {
  const size_t ny = (size_t)w * h, nh = (size_t)(w / 2) * (h / 2);
  std::vector<PIX> cur(ny), prev(ny), half0(nh), half1(nh);
  if (fread(cur.data(), sizeof(PIX), ny, fi) != ny) return 3;
  if (has_prev && fread(prev.data(), sizeof(PIX), ny, fi) != ny) return 3;
  unsigned long long sums[4] = {0, 0, 0, 0};
  tk::RcJob<PIX> J;
  J.sy = w; J.hw = w / 2; J.hh = h / 2; J.out = sums;
  if (has_prev) {
    J.y = prev.data(); J.cur = half0.data(); J.prev = nullptr;
    tk::rc_cost_frame(J);
    sums[0] = sums[1] = sums[2] = 0;
  }
  J.y = cur.data(); J.cur = half1.data(); J.prev = has_prev ? half0.data() : nullptr;
  tk::rc_cost_frame(J);
  fwrite(sums, sizeof(unsigned long long), 3, fo);
  fwrite(half1.data(), sizeof(PIX), nh, fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: %s w h bitdepth has_prev in out\n", argv[0]); return 2; }
  const int w = atoi(argv[1]), h = atoi(argv[2]), bd = atoi(argv[3]), has_prev = atoi(argv[4]);
  if (w % 8 || h % 8 || w < 16 || h < 16 || (bd != 8 && bd != 10 && bd != 12)) return 2;
  FILE* fi = fopen(argv[5], "rb");
  FILE* fo = fopen(argv[6], "wb");
  if (!fi || !fo) return 2;
  const int rc = bd == 8 ? run<uint8_t>(w, h, has_prev, fi, fo) : run<uint16_t>(w, h, has_prev, fi, fo);
  fclose(fi);
  fclose(fo);
  return rc;
}
