// unit_depth.cpp - TEST INFRASTRUCTURE ONLY.
// The three row functions of the mixed-depth path (thor_amd/csrc/tk_filters.h: depth_up_rows, depth_down_rows, frame_sse_depth_rows) on the host, on
// vectors tests/test_mixed_depth.py makes and checks against a numpy restatement of the reference's formulas (stream goldens from natural clips never
// reach the clamp).  Stand-alone: it has its own main, so it may also be compiled with -fsanitize=address,undefined - the planes are allocated exactly
// (16-sample strides like DevFrame, the padding filled with 0xffff), so a vector that reaches past a row or is misaligned is reported.
//   unit_depth W H BITDEPTH INPUT_BITDEPTH IN OUT
// IN:  one packed frame of input-depth samples (bytes for depth 8, else uint16), then two packed frames a, b of uint16 samples at BITDEPTH.
// OUT: the widened input (uint16, packed), a narrowed (input-depth samples, packed), the three sums of frame_sse_depth_rows(a, b) (uint64).
// Every function runs twice - as one work item, and split over 3 row items x 5 lanes the way a launch splits it - and both results must agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../thor_amd/csrc/tk_filters.h"

using namespace tk;

struct Frame {  // planes laid out like DevFrame::alloc(w, h, 0)
  Plane3<uint16_t> p;
  void* mem[3];
  int w, h;
  Frame(int w_, int h_) : w(w_), h(h_) {
    p.sy = (w + 15) & ~15; p.sc = (w / 2 + 15) & ~15;
    const size_t ny = (size_t)p.sy * h, nc = (size_t)p.sc * (h / 2);
    mem[0] = aligned_alloc(16, ny * 2); mem[1] = aligned_alloc(16, nc * 2); mem[2] = aligned_alloc(16, nc * 2);
    memset(mem[0], 0xff, ny * 2); memset(mem[1], 0xff, nc * 2); memset(mem[2], 0xff, nc * 2);
    p.y = (uint16_t*)mem[0]; p.u = (uint16_t*)mem[1]; p.v = (uint16_t*)mem[2];
  }
  ~Frame() { for (void* m : mem) free(m); }
  void from_packed(const uint16_t* s) {
    for (int i = 0; i < h; i++) memcpy(p.y + (size_t)i * p.sy, s + (size_t)i * w, w * 2);
    const uint16_t* cu = s + (size_t)w * h; const uint16_t* cv = cu + (size_t)(w / 2) * (h / 2);
    for (int i = 0; i < h / 2; i++) { memcpy(p.u + (size_t)i * p.sc, cu + (size_t)i * (w / 2), w); memcpy(p.v + (size_t)i * p.sc, cv + (size_t)i * (w / 2), w); }
  }
  void to_packed(uint16_t* d) const {
    for (int i = 0; i < h; i++) memcpy(d + (size_t)i * w, p.y + (size_t)i * p.sy, w * 2);
    uint16_t* cu = d + (size_t)w * h; uint16_t* cv = cu + (size_t)(w / 2) * (h / 2);
    for (int i = 0; i < h / 2; i++) { memcpy(cu + (size_t)i * (w / 2), p.u + (size_t)i * p.sc, w); memcpy(cv + (size_t)i * (w / 2), p.v + (size_t)i * p.sc, w); }
  }
};

// a packed frame in memory of its own, 16-byte aligned as the engine's staging buffer is
struct Packed {
  void* m;
  size_t bytes;
  explicit Packed(size_t n) : m(aligned_alloc(16, (n + 15) & ~(size_t)15)), bytes(n) { memset(m, 0xee, (n + 15) & ~(size_t)15); }
  ~Packed() { free(m); }
};

template <class F> static void split(F f) { for (int g = 0; g < 3; g++) for (int l = 0; l < 5; l++) f(g, 3, l, 5); }

template <typename T> static int run(int w, int h, int bd, int in_bd, FILE* fi, FILE* fo) {
  const size_t n = (size_t)w * h * 3 / 2;
  const int shift = bd - in_bd;
  Packed in(n * sizeof(T));
  std::vector<uint16_t> a(n), b(n);
  if (fread(in.m, sizeof(T), n, fi) != n || fread(a.data(), 2, n, fi) != n || fread(b.data(), 2, n, fi) != n) return fprintf(stderr, "short input\n"), 2;
  // widen
  Frame up1(w, h), up2(w, h);
  depth_up_rows((const T*)in.m, up1.p, w, h, shift, 0, 1, 0, 1);
  split([&](int g, int gs, int l, int nl) { depth_up_rows((const T*)in.m, up2.p, w, h, shift, g, gs, l, nl); });
  std::vector<uint16_t> o1(n), o2(n);
  up1.to_packed(o1.data()); up2.to_packed(o2.data());
  if (o1 != o2) return fprintf(stderr, "depth_up_rows: the split run differs\n"), 1;
  fwrite(o1.data(), 2, n, fo);
  // narrow
  Frame fa(w, h), fb(w, h);
  fa.from_packed(a.data()); fb.from_packed(b.data());
  Packed d1(n * sizeof(T)), d2(n * sizeof(T));
  depth_down_rows(fa.p, (T*)d1.m, w, h, shift, in_bd, 0, 1, 0, 1);
  split([&](int g, int gs, int l, int nl) { depth_down_rows(fa.p, (T*)d2.m, w, h, shift, in_bd, g, gs, l, nl); });
  if (memcmp(d1.m, d2.m, d1.bytes)) return fprintf(stderr, "depth_down_rows: the split run differs\n"), 1;
  fwrite(d1.m, sizeof(T), n, fo);
  // SSE at the input depth
  unsigned long long s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
  frame_sse_depth_rows(fa.p, fb.p, w, h, shift, in_bd, 0, 1, 0, 1, s1);
  split([&](int g, int gs, int l, int nl) { frame_sse_depth_rows(fa.p, fb.p, w, h, shift, in_bd, g, gs, l, nl, s2); });
  if (memcmp(s1, s2, sizeof s1)) return fprintf(stderr, "frame_sse_depth_rows: the split run differs\n"), 1;
  fwrite(s1, 8, 3, fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 7) return fprintf(stderr, "usage: %s W H BITDEPTH INPUT_BITDEPTH IN OUT\n", argv[0]), 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), bd = atoi(argv[3]), in_bd = atoi(argv[4]);
  if (w % 8 || h % 8 || w < 8 || h < 8 || in_bd >= bd) return fprintf(stderr, "bad geometry or depths\n"), 2;
  FILE* fi = fopen(argv[5], "rb");
  FILE* fo = fopen(argv[6], "wb");
  if (!fi || !fo) return fprintf(stderr, "cannot open files\n"), 2;
  const int rc = in_bd == 8 ? run<uint8_t>(w, h, bd, in_bd, fi, fo) : run<uint16_t>(w, h, bd, in_bd, fi, fo);
  fclose(fi); fclose(fo);
  return rc;
}
