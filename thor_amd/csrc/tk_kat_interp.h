// tk_kat_interp.h - TEST ENTRY.  The temporally interpolated reference of `S` streams of one geometry through Engine::make_interp_frames (one
// backend::run_interp call for all of them), with what every stage leaves in the engine's memory copied back: the pyramid planes of both references with
// their padding, the final vector fields nmv[0] / nmv[1] of every level, the whole padded output.  Host-side plumbing over the backend interface only, so
// that the device library (thor_hip_kat_interp_stages, hip_kat.h) and the host build (tests/hostsim/kat_host_interp.cpp) run the same statements.
// Known answers: tests/golden/gen_kat12.py -> kat12*.npz.
#pragma once
#include "tk_encoder.h"

namespace tk {

// a padded plane (rows of `stride` samples around `origin` = picture sample (0, 0)) as tight rows of w + 2 * pad samples
template <typename PIX> PIX* kat_fetch_padded(const PIX* origin, int stride, int w, int h, int pad, PIX* dst) {
  const int rows = h + 2 * pad, cols = w + 2 * pad;
  std::vector<PIX> tmp((size_t)(rows - 1) * stride + cols);
  backend::d2h(tmp.data(), origin - (ptrdiff_t)pad * stride - pad, tmp.size() * sizeof(PIX));
  for (int i = 0; i < rows; i++, dst += cols) memcpy(dst, tmp.data() + (size_t)i * stride, cols * sizeof(PIX));
  return dst;
}
// a packed planar 4:2:0 frame into an unpadded device frame
template <typename PIX> void kat_store_frame(const DevFrame<PIX>& f, const PIX* yuv, int w, int h) {
  PIX* pl[3] = {f.p.y, f.p.u, f.p.v};
  for (int k = 0; k < 3; k++) {
    const int pw = k ? w / 2 : w, ph = k ? h / 2 : h, st = k ? f.p.sc : f.p.sy;
    std::vector<PIX> tmp((size_t)(ph - 1) * st + pw);
    for (int i = 0; i < ph; i++, yuv += pw) memcpy(tmp.data() + (size_t)i * st, yuv, pw * sizeof(PIX));
    backend::h2d(pl[k], tmp.data(), tmp.size() * sizeof(PIX));
  }
}

// Per stream: yuv0 / yuv1 one packed planar frame each; pyr: reference 0 then 1, levels 1 .. levels-1, (h >> l) + 64 rows of (w >> l) + 64 samples; nmv: per
// level nmv[0] then nmv[1], bw * bh (x, y) pairs each; out: Y with kPadY, U and V with kPadY / 2.  `levels` is the caller's count (it sized the buffers).
template <typename PIX>
int kat_interp_stages(int S, const PIX* yuv0, const PIX* yuv1, int width, int height, int bitdepth, int levels, PIX* pyr, int16_t* nmv, PIX* out) {
  if (!yuv0 || !yuv1 || !pyr || !nmv || !out || S < 1 || S > 4 || width % 8 || height % 8 || width < 64 || height < 64 || width > 8192 || height > 8192) return 1;
  if (levels < 1 || levels > idev::kMaxLevels) return 1;
  SeqParams sp;
  sp.width = width; sp.height = height; sp.bitdepth = bitdepth; sp.input_bitdepth = bitdepth;
  sp.num_reorder_pics = 7; sp.interp_ref = 1; sp.max_num_ref = 2; sp.HQperiod = 8; sp.cdef = 0; sp.clpf = 0;
  Engine<PIX>* eng = new Engine<PIX>();
  eng->open(sp, S);
  int rc = eng->st[0].ip_levels == levels ? 0 : 2;
  const size_t fsz = (size_t)width * height * 3 / 2;
  if (!rc) {
    for (int s = 0; s < S; s++)
      for (int k = 0; k < 2; k++) {
        Stream<PIX>& q = eng->st[s];
        kat_store_frame(q.rec, (k ? yuv1 : yuv0) + fsz * s, width, height);
        FrameJob<PIX> J;
        memset(&J, 0, sizeof(J));
        J.cfg.width = width; J.cfg.height = height; J.rec = q.rec.p;
        backend::run_make_ref<PIX>(&J, &q.ring[k].p, 1);
        backend::dev_sync();
      }
    std::vector<FrameParams> fp(S);
    for (int s = 0; s < S; s++) { fp[s].interp_ref = 1; fp[s].interp_src[0] = 0; fp[s].interp_src[1] = 1; fp[s].frame_num = 1; }
    eng->make_interp_frames(fp, 0, S);
    backend::dev_sync();
    for (int s = 0; s < S; s++) {
      const Stream<PIX>& q = eng->st[s];
      for (int r = 0; r < 2; r++)
        for (int l = 1; l < levels; l++)
          pyr = kat_fetch_padded(q.ip_pic[r][l] + (size_t)32 * q.ip_stride[l] + 32, q.ip_stride[l], width >> l, height >> l, 32, pyr);
      for (int l = 0; l < levels; l++) {
        const size_t n = (size_t)eng->h_ijobs[s].lv[l].bw * eng->h_ijobs[s].lv[l].bh;
        for (int k = 2; k < 4; k++, nmv += 2 * n) backend::d2h(nmv, q.ip_mv[l][k], n * sizeof(idev::imv));
      }
      out = kat_fetch_padded(q.interp.p.y, q.interp.p.sy, width, height, kPadY, out);
      out = kat_fetch_padded(q.interp.p.u, q.interp.p.sc, width / 2, height / 2, kPadY / 2, out);
      out = kat_fetch_padded(q.interp.p.v, q.interp.p.sc, width / 2, height / 2, kPadY / 2, out);
    }
  }
  eng->close();
  delete eng;
  return rc;
}

}  // namespace tk
