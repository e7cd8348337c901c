// unit_scale.cpp - TEST INFRASTRUCTURE ONLY.
// The host build of what stages a frame of another size (thor_amd/csrc/tk_scale.h: resolve_scale and the TK_DEV pieces k_scale_in is made of) on a
// buffer tests/test_scale_format.py makes and checks against tests/scale_format.py.  Stand-alone: it has its own main.  The planes are allocated like
// DevFrame's (16-sample strides, 16-byte aligned, padding 0xff); the source buffer is allocated exactly (no byte after the frame), SKEW bytes off a
// 16-byte boundary, so the caller chooses between the vector and the sample-by-sample path and a sanitizer sees any read outside the frame.
//   unit_scale SRC_W SRC_H W H INPUT_BITDEPTH BITDEPTH FILTER SITE CHROMA MSB PITCH_Y PITCH_C SKEW IN OUT
// IN:  a source frame (resolve_scale's layout `bytes`).   OUT: the planes (packed, engine-depth samples).
// The frame is resampled twice - with one lane, as the Engine's host path does, and as 4 wavefronts x 64 lanes, the way a workgroup splits a tile -
// and both results must agree.  Exit status 3: resolve_scale refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../thor_amd/csrc/tk_scale.h"

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
  void to_packed(PIX* d) const {
    const int cw = w / 2, ch = h / 2;
    for (int i = 0; i < h; i++) memcpy(d + (size_t)i * w, p.y + (size_t)i * p.sy, w * sizeof(PIX));
    PIX* cu = d + (size_t)w * h; PIX* cv = cu + (size_t)cw * ch;
    for (int i = 0; i < ch; i++) { memcpy(cu + (size_t)i * cw, p.u + (size_t)i * p.sc, cw * sizeof(PIX)); memcpy(cv + (size_t)i * cw, p.v + (size_t)i * p.sc, cw * sizeof(PIX)); }
  }
  bool padding_untouched() const {  // nothing outside the picture's samples was written
    for (int i = 0; i < h; i++) for (int x = w; x < p.sy; x++) if (p.y[(size_t)i * p.sy + x] != (PIX)~(PIX)0) return false;
    for (int i = 0; i < h / 2; i++) for (int x = w / 2; x < p.sc; x++) if (p.u[(size_t)i * p.sc + x] != (PIX)~(PIX)0 || p.v[(size_t)i * p.sc + x] != (PIX)~(PIX)0) return false;
    return true;
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

template <typename S, typename PIX> static int run(const ScalePlan& P, int in_bd, int bd, size_t skew, FILE* fi, FILE* fo) {
  const int w = P.width, h = P.height;
  const size_t n = (size_t)w * h * 3 / 2;
  Skewed src(P.L.bytes, skew);
  if (fread(src.p, 1, P.L.bytes, fi) != P.L.bytes) return fprintf(stderr, "short input\n"), 2;
  const ScaleTables tab = P.host_tables();
  Frame<PIX> a1(w, h), a2(w, h);
  scale_in_host<S, PIX>(src.p, P.L, tab, a1.p, P.src_w, w, h, in_bd, bd - in_bd, 1, 1);
  scale_in_host<S, PIX>(src.p, P.L, tab, a2.p, P.src_w, w, h, in_bd, bd - in_bd, SCALE_WAVES, 64);
  std::vector<PIX> o1(n), o2(n);
  a1.to_packed(o1.data()); a2.to_packed(o2.data());
  if (o1 != o2) return fprintf(stderr, "scale_in_host: the split run differs\n"), 1;
  if (!a1.padding_untouched() || !a2.padding_untouched()) return fprintf(stderr, "scale_in_host: wrote outside the picture\n"), 1;
  fwrite(o1.data(), sizeof(PIX), n, fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 16) return fprintf(stderr, "usage: %s SRC_W SRC_H W H INPUT_BITDEPTH BITDEPTH FILTER SITE CHROMA MSB PITCH_Y PITCH_C SKEW IN OUT\n", argv[0]), 2;
  const int sw = atoi(argv[1]), sh = atoi(argv[2]), w = atoi(argv[3]), h = atoi(argv[4]), in_bd = atoi(argv[5]), bd = atoi(argv[6]);
  if (in_bd > bd) return fprintf(stderr, "bad depths\n"), 2;
  ScalePlan P;
  if (!resolve_scale(sw, sh, atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), atoll(argv[11]), atoll(argv[12]), 0, 0, w, h, in_bd, P)) return 3;
  const size_t skew = (size_t)atoll(argv[13]);
  FILE* fi = fopen(argv[14], "rb");
  FILE* fo = fopen(argv[15], "wb");
  if (!fi || !fo) return fprintf(stderr, "cannot open files\n"), 2;
  int rc;
  if (bd == 8) rc = run<uint8_t, uint8_t>(P, in_bd, bd, skew, fi, fo);
  else if (in_bd == 8) rc = run<uint8_t, uint16_t>(P, in_bd, bd, skew, fi, fo);
  else rc = run<uint16_t, uint16_t>(P, in_bd, bd, skew, fi, fo);
  fclose(fi); fclose(fo);
  return rc;
}
