// unit_rgb.cpp - TEST INFRASTRUCTURE ONLY.
// The host build of what stages and fetches RGB frames (thor_amd/csrc/tk_filters.h: resolve_rgb, rgb_in_rows, rgb_out_rows) on buffers
// tests/test_rgb_format.py makes and checks against tests/rgb_format.py.  Stand-alone: it has its own main.  The planes are allocated like DevFrame's
// (16-sample strides, 16-byte aligned, padding 0xff); the RGB buffers are allocated exactly (no byte after the frame, or after the frame and its
// guard), SKEW bytes off a 16-byte boundary, so the caller chooses between the vector and the sample-by-sample path and a sanitizer sees any access
// outside the frame.
//   unit_rgb W H INPUT_BITDEPTH BITDEPTH ORDER DEPTH MSB MATRIX FULL SITE PITCH PLANE_STRIDE SKEW IN OUT
//   unit_rgb coefficients W H INPUT_BITDEPTH ORDER DEPTH MSB MATRIX FULL SITE      prints "name value" lines of the resolved format
// IN:  an RGB frame (resolve_rgb's `bytes`), a packed planar frame of engine-depth samples, the destination of rgb_out_rows as it is before the call
//      (`bytes` + 64 guard bytes).
// OUT: the planes rgb_in_rows made of the first (packed, engine-depth samples), the destination after rgb_out_rows wrote the second into it.
// Every function runs twice - as one work item with one lane, and split over 3 work items x 64 lanes the way a launch splits it - and both results
// must agree.  Exit status 3: resolve_rgb refused the format.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../thor_amd/csrc/tk_filters.h"

using namespace tk;

template <typename PIX> struct Frame {  // planes laid out like DevFrame::alloc(w, h, 0)
  Plane3<PIX> p;
  void* mem[3];
  int w, h;
  Frame(int w_, int h_) : w(w_), h(h_) {
    p.sy = (w + 15) & ~15; p.sc = (w / 2 + 15) & ~15;
    const size_t ny = (size_t)p.sy * h, nc = (size_t)p.sc * (h / 2);
    mem[0] = aligned_alloc(16, ny * sizeof(PIX)); mem[1] = aligned_alloc(16, nc * sizeof(PIX)); mem[2] = aligned_alloc(16, nc * sizeof(PIX));
    memset(mem[0], 0xff, ny * sizeof(PIX)); memset(mem[1], 0xff, nc * sizeof(PIX)); memset(mem[2], 0xff, nc * sizeof(PIX));
    p.y = (PIX*)mem[0]; p.u = (PIX*)mem[1]; p.v = (PIX*)mem[2];
  }
  ~Frame() { for (void* m : mem) free(m); }
  void from_packed(const PIX* s) {
    const int cw = w / 2, ch = h / 2;
    for (int i = 0; i < h; i++) memcpy(p.y + (size_t)i * p.sy, s + (size_t)i * w, w * sizeof(PIX));
    const PIX* cu = s + (size_t)w * h; const PIX* cv = cu + (size_t)cw * ch;
    for (int i = 0; i < ch; i++) { memcpy(p.u + (size_t)i * p.sc, cu + (size_t)i * cw, cw * sizeof(PIX)); memcpy(p.v + (size_t)i * p.sc, cv + (size_t)i * cw, cw * sizeof(PIX)); }
  }
  void to_packed(PIX* d) const {
    const int cw = w / 2, ch = h / 2;
    for (int i = 0; i < h; i++) memcpy(d + (size_t)i * w, p.y + (size_t)i * p.sy, w * sizeof(PIX));
    PIX* cu = d + (size_t)w * h; PIX* cv = cu + (size_t)cw * ch;
    for (int i = 0; i < ch; i++) { memcpy(cu + (size_t)i * cw, p.u + (size_t)i * p.sc, cw * sizeof(PIX)); memcpy(cv + (size_t)i * cw, p.v + (size_t)i * p.sc, cw * sizeof(PIX)); }
  }
};

// exactly n bytes that start `skew` bytes after a 16-byte boundary and end where their block ends
struct Skewed {
  uint8_t* m = nullptr;
  uint8_t* p;
  Skewed(size_t n, size_t skew) {
    if (posix_memalign((void**)&m, 16, skew + n)) { fprintf(stderr, "out of memory\n"); exit(2); }
    p = m + skew;
  }
  ~Skewed() { free(m); }
};

template <class F> static void split(F f) { for (int g = 0; g < 3; g++) for (int l = 0; l < 64; l++) f(g, 3, l, 64); }

static const size_t kGuard = 64;

template <typename S, typename PIX> static int run(int w, int h, int in_bd, int bd, const RgbFormat& R, size_t skew, FILE* fi, FILE* fo) {
  const size_t n = (size_t)w * h * 3 / 2;
  Skewed src(R.bytes, skew), d1(R.bytes + kGuard, skew), d2(R.bytes + kGuard, skew);
  std::vector<PIX> planar(n);
  if (fread(src.p, 1, R.bytes, fi) != R.bytes || fread(planar.data(), sizeof(PIX), n, fi) != n || fread(d1.p, 1, R.bytes + kGuard, fi) != R.bytes + kGuard)
    return fprintf(stderr, "short input\n"), 2;
  memcpy(d2.p, d1.p, R.bytes + kGuard);
  // RGB -> planes
  Frame<PIX> a1(w, h), a2(w, h);
  rgb_in_rows<S, PIX>(src.p, R, a1.p, w, h, bd - in_bd, 0, 1, 0, 1);
  split([&](int g, int gs, int l, int nl) { rgb_in_rows<S, PIX>(src.p, R, a2.p, w, h, bd - in_bd, g, gs, l, nl); });
  std::vector<PIX> o1(n), o2(n);
  a1.to_packed(o1.data()); a2.to_packed(o2.data());
  if (o1 != o2) return fprintf(stderr, "rgb_in_rows: the split run differs\n"), 1;
  fwrite(o1.data(), sizeof(PIX), n, fo);
  // planes -> RGB
  Frame<PIX> f(w, h);
  f.from_packed(planar.data());
  rgb_out_rows<PIX, S>(f.p, d1.p, R, w, h, bd - in_bd, 0, 1, 0, 1);
  split([&](int g, int gs, int l, int nl) { rgb_out_rows<PIX, S>(f.p, d2.p, R, w, h, bd - in_bd, g, gs, l, nl); });
  if (memcmp(d1.p, d2.p, R.bytes + kGuard)) return fprintf(stderr, "rgb_out_rows: the split run differs\n"), 1;
  fwrite(d1.p, 1, R.bytes + kGuard, fo);
  return 0;
}

int main(int argc, char** argv) {
  RgbFormat R;
  if (argc == 11 && !strcmp(argv[1], "coefficients")) {
    if (!resolve_rgb(atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), 0, 0, atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), R)) return 3;
    printf("yr %d\nyg %d\nyb %d\nur %d\nug %d\nub %d\nvr %d\nvg %d\nvb %d\niy %d\nrv %d\ngu %d\ngv %d\nbu %d\nbytes %zu\n", R.yr, R.yg, R.yb, R.ur, R.ug, R.ub, R.vr, R.vg,
           R.vb, R.iy, R.rv, R.gu, R.gv, R.bu, R.bytes);
    return 0;
  }
  if (argc != 16) return fprintf(stderr, "usage: %s W H INPUT_BITDEPTH BITDEPTH ORDER DEPTH MSB MATRIX FULL SITE PITCH PLANE_STRIDE SKEW IN OUT\n", argv[0]), 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), in_bd = atoi(argv[3]), bd = atoi(argv[4]);
  if (in_bd > bd) return fprintf(stderr, "bad depths\n"), 2;
  if (!resolve_rgb(atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), atoll(argv[11]), (size_t)atoll(argv[12]), w, h, in_bd, R)) return 3;
  const size_t skew = (size_t)atoll(argv[13]);
  FILE* fi = fopen(argv[14], "rb");
  FILE* fo = fopen(argv[15], "wb");
  if (!fi || !fo) return fprintf(stderr, "cannot open files\n"), 2;
  int rc;
  if (bd == 8) rc = R.sbytes == 1 ? run<uint8_t, uint8_t>(w, h, in_bd, bd, R, skew, fi, fo) : run<uint16_t, uint8_t>(w, h, in_bd, bd, R, skew, fi, fo);
  else rc = R.sbytes == 1 ? run<uint8_t, uint16_t>(w, h, in_bd, bd, R, skew, fi, fo) : run<uint16_t, uint16_t>(w, h, in_bd, bd, R, skew, fi, fo);
  fclose(fi); fclose(fo);
  return rc;
}
