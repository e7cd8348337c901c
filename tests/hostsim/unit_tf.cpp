// unit_tf.cpp - TEST INFRASTRUCTURE ONLY.
// The temporal filter (thor_amd/csrc/tk_tf.h: the TK_DEV block functions k_tf_search / k_tf_blend run) compiled for the host with one lane.
//   unit_tf filter <w> <h> <bitdepth> <strength> <nrefs> <dist...> <in> <out>
//     in: the current frame, then the neighbours: packed planar 4:2:0, w x h (bytes for bitdepth 8, uint16_t above).
//     out: the filtered frame, then per neighbour and 8x8 block (raster order) dx, dy, wb as three int32_t.
//   unit_tf requests <num_streams> <staged> <n> <12 ints per request: stream dst_slot slot nrefs ref_slot[4] ref_dist[4]>
//     prints 0 when tf_requests_ok accepts the call with slots 0 .. staged - 1 of every stream staged, else 1.
#include "../../thor_amd/csrc/tk_tf.h"
#include <vector>

template <typename PIX> static tk::Plane3<PIX> planes(std::vector<PIX>& v, int w, int h) {
  tk::Plane3<PIX> p;
  p.y = v.data(); p.u = p.y + (size_t)w * h; p.v = p.u + (size_t)(w / 2) * (h / 2);
  p.sy = w; p.sc = w / 2;
  return p;
}

template <typename PIX> static int run(int w, int h, int bd, int strength, int nrefs, const int* dist, FILE* fi, FILE* fo) {
  const size_t fsz = (size_t)w * h * 3 / 2, nb = (size_t)(w / 8) * (h / 8);
  std::vector<PIX> cur(fsz), out(fsz);
  std::vector<std::vector<PIX>> refs(nrefs, std::vector<PIX>(fsz));
  if (fread(cur.data(), sizeof(PIX), fsz, fi) != fsz) return 3;
  for (auto& r : refs)
    if (fread(r.data(), sizeof(PIX), fsz, fi) != fsz) return 3;
  std::vector<tk::TfBlock> blk(nb * tk::TF_MAX_REFS);
  tk::TfJob<PIX> J;
  J.cur = planes(cur, w, h); J.dst = planes(out, w, h);
  for (int k = 0; k < nrefs; k++) { J.ref[k] = planes(refs[k], w, h); J.dist[k] = dist[k]; }
  J.nrefs = nrefs; J.width = w; J.height = h; J.strength = strength; J.sh = bd - 8; J.blk = blk.data();
  tk::tf_filter_frame(J);
  fwrite(out.data(), sizeof(PIX), fsz, fo);
  for (size_t i = 0; i < nb * nrefs; i++) {
    const int32_t rec[3] = {blk[i].dx, blk[i].dy, blk[i].wb};
    fwrite(rec, sizeof rec, 1, fo);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 5 && !strcmp(argv[1], "requests")) {
    const int S = atoi(argv[2]), staged = atoi(argv[3]), n = atoi(argv[4]);
    if (n < 0 || argc != 5 + 12 * n) return 2;
    std::vector<tk::TfRequest> req(n);
    for (int i = 0; i < n; i++) {
      int v[12];
      for (int k = 0; k < 12; k++) v[k] = atoi(argv[5 + 12 * i + k]);
      req[i].stream = v[0]; req[i].dst_slot = v[1]; req[i].slot = v[2]; req[i].nrefs = v[3];
      for (int k = 0; k < 4; k++) { req[i].ref_slot[k] = v[4 + k]; req[i].ref_dist[k] = v[8 + k]; }
    }
    printf("%d\n", tk::tf_requests_ok(req.data(), n, S, [&](int, int slot) { return slot >= 0 && slot < staged; }) ? 0 : 1);
    return 0;
  }
  if (argc < 9 || strcmp(argv[1], "filter")) { fprintf(stderr, "usage: %s filter w h bitdepth strength nrefs dist... in out | requests ...\n", argv[0]); return 2; }
  const int w = atoi(argv[2]), h = atoi(argv[3]), bd = atoi(argv[4]), strength = atoi(argv[5]), nrefs = atoi(argv[6]);
  if (w % 8 || h % 8 || w < 16 || h < 16 || (bd != 8 && bd != 10 && bd != 12) || !tk::tf_strength_ok(strength) || nrefs < 0 || nrefs > tk::TF_MAX_REFS || argc != 9 + nrefs) return 2;
  int dist[tk::TF_MAX_REFS] = {1, 1, 1, 1};
  for (int k = 0; k < nrefs; k++) dist[k] = atoi(argv[7 + k]);
  FILE* fi = fopen(argv[7 + nrefs], "rb");
  FILE* fo = fopen(argv[8 + nrefs], "wb");
  if (!fi || !fo) return 2;
  const int rc = bd == 8 ? run<uint8_t>(w, h, bd, strength, nrefs, dist, fi, fo) : run<uint16_t>(w, h, bd, strength, nrefs, dist, fi, fo);
  fclose(fi);
  fclose(fo);
  return rc;
}
