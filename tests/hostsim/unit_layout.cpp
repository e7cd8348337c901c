// unit_layout.cpp - TEST INFRASTRUCTURE ONLY.
// The two row functions behind frames in a caller's layout (thor_amd/csrc/tk_filters.h: layout_in_rows, layout_out_rows) on the host, on buffers
// tests/test_frame_layout.py makes and checks against a few lines of numpy.  Stand-alone: it has its own main.  The planes are allocated like
// DevFrame's (16-sample strides, 16-byte aligned, padding 0xff), the layout buffers exactly, SKEW bytes off a 16-byte boundary, so the caller
// chooses between the vector and the sample-by-sample path.
//   unit_layout W H INPUT_BITDEPTH BITDEPTH CHROMA MSB PITCH_Y PITCH_C OFFSET_U OFFSET_V SKEW IN OUT
// IN:  a frame in the layout (resolve_layout's `bytes`), a packed planar frame of engine-depth samples, the destination of layout_out_rows as it is
//      before the call (`bytes` + 64 guard bytes).
// OUT: the planes layout_in_rows made of the first (packed, engine-depth samples), the destination after layout_out_rows wrote the second into it.
// Every function runs twice - as one work item with one lane, and split over 3 row items x 64 lanes the way a launch splits it - and both results
// must agree.  Exit status 3: resolve_layout refused the layout.
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

// n bytes that start `skew` bytes after a 16-byte boundary
struct Skewed {
  uint8_t* m;
  uint8_t* p;
  Skewed(size_t n, size_t skew) : m((uint8_t*)aligned_alloc(16, (n + skew + 15) & ~(size_t)15)), p(m + skew) {}
  ~Skewed() { free(m); }
};

template <class F> static void split(F f) { for (int g = 0; g < 3; g++) for (int l = 0; l < 64; l++) f(g, 3, l, 64); }

static const size_t kGuard = 64;

template <typename S, typename PIX> static int run(int w, int h, int in_bd, int bd, const PixLayout& L, size_t skew, FILE* fi, FILE* fo) {
  const size_t n = (size_t)w * h * 3 / 2;
  Skewed src(L.bytes, skew), d1(L.bytes + kGuard, skew), d2(L.bytes + kGuard, skew);
  std::vector<PIX> planar(n);
  if (fread(src.p, 1, L.bytes, fi) != L.bytes || fread(planar.data(), sizeof(PIX), n, fi) != n || fread(d1.p, 1, L.bytes + kGuard, fi) != L.bytes + kGuard)
    return fprintf(stderr, "short input\n"), 2;
  memcpy(d2.p, d1.p, L.bytes + kGuard);
  // layout -> planes
  Frame<PIX> a1(w, h), a2(w, h);
  layout_in_rows<S, PIX>(src.p, L, a1.p, w, h, bd - in_bd, 0, 1, 0, 1);
  split([&](int g, int gs, int l, int nl) { layout_in_rows<S, PIX>(src.p, L, a2.p, w, h, bd - in_bd, g, gs, l, nl); });
  std::vector<PIX> o1(n), o2(n);
  a1.to_packed(o1.data()); a2.to_packed(o2.data());
  if (o1 != o2) return fprintf(stderr, "layout_in_rows: the split run differs\n"), 1;
  fwrite(o1.data(), sizeof(PIX), n, fo);
  // planes -> layout
  Frame<PIX> f(w, h);
  f.from_packed(planar.data());
  layout_out_rows<PIX, S>(f.p, d1.p, L, w, h, bd - in_bd, in_bd, 0, 1, 0, 1);
  split([&](int g, int gs, int l, int nl) { layout_out_rows<PIX, S>(f.p, d2.p, L, w, h, bd - in_bd, in_bd, g, gs, l, nl); });
  if (memcmp(d1.p, d2.p, L.bytes + kGuard)) return fprintf(stderr, "layout_out_rows: the split run differs\n"), 1;
  fwrite(d1.p, 1, L.bytes + kGuard, fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 14) return fprintf(stderr, "usage: %s W H INPUT_BITDEPTH BITDEPTH CHROMA MSB PITCH_Y PITCH_C OFFSET_U OFFSET_V SKEW IN OUT\n", argv[0]), 2;
  const int w = atoi(argv[1]), h = atoi(argv[2]), in_bd = atoi(argv[3]), bd = atoi(argv[4]);
  if (w % 8 || h % 8 || w < 16 || h < 16 || in_bd > bd) return fprintf(stderr, "bad geometry or depths\n"), 2;
  PixLayout L;
  if (!resolve_layout(atoi(argv[5]), atoi(argv[6]), atoll(argv[7]), atoll(argv[8]), (size_t)atoll(argv[9]), (size_t)atoll(argv[10]), w, h, in_bd, L)) return 3;
  const size_t skew = (size_t)atoll(argv[11]);
  FILE* fi = fopen(argv[12], "rb");
  FILE* fo = fopen(argv[13], "wb");
  if (!fi || !fo) return fprintf(stderr, "cannot open files\n"), 2;
  int rc;
  if (bd == 8) rc = run<uint8_t, uint8_t>(w, h, in_bd, bd, L, skew, fi, fo);
  else if (in_bd == 8) rc = run<uint8_t, uint16_t>(w, h, in_bd, bd, L, skew, fi, fo);
  else rc = run<uint16_t, uint16_t>(w, h, in_bd, bd, L, skew, fi, fo);
  fclose(fi); fclose(fo);
  return rc;
}
