// hip_kat.h - C ABI, kernel-level batch entry points for the known-answer tests ("KAT"), and thor_hip_superblock_kernel_info / _in_use (part of the
// translation unit thor_hip.cpp: the kernels here run the very device functions the superblock kernel calls).
#pragma once
#include "tk_kat_bits.h"
#include "tk_kat_interp.h"
namespace tk {
// The kernels behind the known-answer entry points run the product's device code on one block / transform unit per workgroup of
// one wavefront; PIX = uint8_t (the reference's _lbd functions) or uint16_t (_hbd, bitdepth 9..12).
template <typename PIX>
__global__ __launch_bounds__(64) void k_kat_sad(const PIX* org, int w, int h, const PIX* refp, int rstride, int bx, int by, const int* cand, int n,
                                               uint32_t* out) {
  // the product's full-pel evaluator (tk_me_seg.h:seg_sads, row segment per lane), plane reads only (no search window)
  const Team t = mk_team((int)threadIdx.x, 64);
  struct KC { const PIX* p; int dx, dy; };
  MeWin win;
  win.on = 0; win.w32 = nullptr; win.ox = win.oy = win.Ww = win.Wh = win.pitch = 0;
  auto cnd = [&](int c) -> KC {
    KC x;
    x.dx = cand[2 * c]; x.dy = cand[2 * c + 1];
    x.p = refp + (size_t)(by + x.dy) * rstride + bx + x.dx;
    return x;
  };
  seg_sads<SP_GLOBAL>(t, n, org, w, rstride, w, h, win, cnd, [&](int c, const KC&, int sad, int mine) { if (mine) out[c] = (uint32_t)sad; });
}
template <typename PIX>
__global__ __launch_bounds__(64) void k_kat_interp(const PIX* ref0, int rstride, int pic_w, int pic_h, int bx, int by, int w, int h,
                                                  const int16_t* mv, int bipred, int bitdepth, PIX* out) {
  const Team t = mk_team((int)threadIdx.x, 64);
  const int i = blockIdx.x;
  pred_luma<SP_GLOBAL>(t, out + (size_t)i * w * h, w, ref0 + (size_t)by * rstride + bx, rstride, w, h, mk_mv(mv[2 * i], mv[2 * i + 1]), 0,
            bipred, pic_w, pic_h, bx, by, bitdepth);
}
template <typename PIX>
__global__ __launch_bounds__(64) void k_kat_tu(const PIX* org, const PIX* pred, int size, int qp, int coeff_type, int fast, int bitdepth,
                                              int16_t* coefq, PIX* rec, int* cbp) {
  __shared__ XformWs xf;
  __shared__ XformTabs tabs;
  __shared__ int16_t cq[256];
  const Team t = mk_team((int)threadIdx.x, 64, tabs.izz);
  xf.prof = nullptr;
  xf.tabs = &tabs;
  xform_tables_fill(&tabs, (int)threadIdx.x, 64);
  t.sync();
  const int i = blockIdx.x, qs = size < 16 ? size : 16;
  const size_t o = (size_t)i * size * size;
  int c = code_tu(t, &xf, org + o, size, pred + o, size, rec + o, size, size, qp, coeff_type, fast, cq, bitdepth);
  for (int k = threadIdx.x; k < qs * qs; k += 64) coefq[(size_t)i * qs * qs + k] = cq[k];
  if (threadIdx.x == 0) cbp[i] = c;
}

// ---- round 6: known-answer kernels for the sample kernels that were only covered by whole-stream hashes -------------------------
// One wavefront per item, running exactly the device functions the encoder calls.
template <typename PIX>
__global__ __launch_bounds__(64) void k_kat_intra(const PIX* plane, int stride, int bitdepth, int size, int tb_split, const int* par, const PIX* rblocks,
                                                 PIX* out) {
  __shared__ IntraEdge<PIX> edge;
  const Team t = mk_team((int)threadIdx.x, 64);
  const int it = blockIdx.x;
  const int* q = par + 7 * it;   // ypos, xpos (coding block), upright, downleft, mode, i, j (transform unit inside the block)
  const int cbs = tb_split ? 2 * size : size;
  const PIX* rblock = tb_split ? rblocks + (size_t)it * cbs * cbs + q[5] * cbs + q[6] : nullptr;
  make_edges<SP_GLOBAL>(t, &edge, plane + (size_t)q[0] * stride + q[1], stride, rblock, cbs, q[5], q[6], q[0], q[1], size, q[2], q[3], tb_split, bitdepth);
  pred_intra<SP_GLOBAL>(t, &edge, q[0] + q[5], q[1] + q[6], size, out + (size_t)it * size * size, size, q[4], bitdepth);
}
// (pred_inter_yuv / improve_uv are __noinline__ functions the superblock kernel calls too: a kernel with a larger register budget calling them would raise
// THEIR budget and with it the superblock kernel's VGPR count - 227 instead of 168, two workgroups per CU instead of three, measured in round 6 - so these two
// kernels carry the superblock kernel's launch bounds)
template <typename PIX>
__global__ __launch_bounds__(kWgThreads, (sizeof(PIX) == 1 ? (int)kOcc : 2)) void k_kat_inter_yuv(Plane3<PIX> ref, int width, int height, int bitdepth, int size, const int* par, const int16_t* mv, PIX* out) {
  const Team t = mk_team((int)threadIdx.x, 64);
  const int it = blockIdx.x;
  const int* q = par + 5 * it;   // ypos, xpos, sign, enable_bipred, split
  mv_t m[4];
  for (int k = 0; k < 4; k++) m[k] = mk_mv(mv[(it * 4 + k) * 2], mv[(it * 4 + k) * 2 + 1]);
  PIX* o = out + (size_t)it * (size * size * 3 / 2);
  pred_inter_yuv<SP_GLOBAL>(t, ref, o, o + size * size, o + size * size * 5 / 4, q[0], q[1], size, size, size, m, q[2], width, height, q[3], q[4], bitdepth);
}
template <typename PIX> __global__ __launch_bounds__(64) void k_kat_average(const PIX* a, const PIX* b, int size, PIX* out) {
  const Team t = mk_team((int)threadIdx.x, 64);
  const size_t o = (size_t)blockIdx.x * (size * size * 3 / 2);
  const int n = size * size, c = n / 4;
  average_yuv<SP_GLOBAL>(t, out + o, out + o + n, out + o + n + c, a + o, a + o + n, a + o + n + c, b + o, b + o + n, b + o + n + c, size, size, size);
}
template <typename PIX>
__global__ __launch_bounds__(kWgThreads, (sizeof(PIX) == 1 ? (int)kOcc : 2)) void k_kat_cfl(const PIX* y, PIX* uv, const PIX* ry, int n, int bitdepth) {
  const Team t = mk_team((int)threadIdx.x, 64);
  const int it = blockIdx.x, c = (n / 2) * (n / 2);
  improve_uv<PIX, SP_GLOBAL>(t, nullptr, y + (size_t)it * n * n, uv + (size_t)it * 2 * c, uv + (size_t)it * 2 * c + c, ry + (size_t)it * n * n, n, n, n, bitdepth);
}
template <typename PIX> __global__ void k_kat_cdef_dir(const PIX* blocks, int n, int cs, int* dir, int* var) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  int v = 0;
  dir[i] = cdef_find_dir(blocks + (size_t)i * 64, 8, &v, cs);
  var[i] = v;
}
template <typename PIX>
__global__ __launch_bounds__(64) void k_kat_cdef_filter(const PIX* plane, int w, int h, int stride, int bsize, int cs, const int* par, PIX* out) {
  const int it = blockIdx.x, k = threadIdx.x;
  if (k >= bsize * bsize) return;
  const int* q = par + 7 * it;   // x0, y0, pri, sec, dir, pri_damping, sec_damping
  const int x = q[0] + k % bsize, y = q[1] + k / bsize;
  out[(size_t)it * bsize * bsize + k] = (PIX)cdef_filter_px(plane, stride, x, y, w, h, q[2], q[3], q[4], q[5], q[6], cs);
}
// ---- the motion search and the early-skip sub-block tests: one workgroup of one wavefront per item, the workspace built as the superblock kernel builds it
// (make_ws: WgShared + SmallWs in LDS, the search window in the transform workspace + win_extra with the product's win_cap).  motion_estimate /
// motion_estimate_bi are __noinline__ functions the superblock kernel calls too, so these kernels carry its launch bounds (see k_kat_inter_yuv above).
// par[kKatMePar * i ..]: cb_x, cb_y, cb, pu_dx, pu_dy, pw, ph, mvc.x, mvc.y, mvp.x, mvp.y, sign, enable_bipred, encoder_speed, ncand, cand_off, stage
enum { kKatMePar = 17 };
template <typename PIX>
__global__ __launch_bounds__(kWgThreads, (sizeof(PIX) == 1 ? (int)kOcc : 2)) void k_kat_me(int bi, Plane3<PIX> cur, Plane3<PIX> ref0, Plane3<PIX> ref1, int fw, int fh, int bitdepth,
                                                                                           const int* par, const double* lam, const int16_t* cand, unsigned char* big, int* out,
                                                                                           int16_t* list_out) {
  __shared__ WgShared sh;
  __shared__ SmallWs<PIX> sws;
  const int lane = (int)threadIdx.x, it = (int)blockIdx.x;
  TeamWs<PIX> ws = make_ws(&sws, &sh, (BigWs<PIX>*)big);
  const Team t = mk_team(lane, 64, sh.tabs.izz);
  xform_tables_fill(&sh.tabs, lane, 64);
  const int* q = par + kKatMePar * it;
  const int cbx = q[0], cby = q[1], cb = q[2], pux = cbx + q[3], puy = cby + q[4];
  MeLists* lists = &sh.lists;
  const int nl = bi ? 6 : q[14];
  for (int c = lane; c < nl; c += 64) { lists->mvcand[0][c].x = cand[2 * (q[15] + c)]; lists->mvcand[0][c].y = cand[2 * (q[15] + c) + 1]; }
  if (lane == 0) { lists->mvcand_num[0] = q[14]; lists->mvcand_mask[0] = 0; lists->best_ref = 0; }
  // the original block: the workgroup's LDS copy (stride = CB size) for CBs up to kLdsBlk, the frame plane above (org_select)
  const int lds_blk = __builtin_amdgcn_readfirstlane(cb <= kLdsBlk);
  PIX* orgc = (PIX*)sh.org_raw;
  if (lds_blk)
    for (int k = lane; k < cb * cb; k += 64) orgc[k] = cur.y[(size_t)(cby + k / cb) * cur.sy + cbx + k % cb];
  __syncthreads();
  MeArgs a;
  a.cb_size = cb; a.ostride = lds_blk ? cb : cur.sy; a.width = q[5]; a.height = q[6]; a.rstride = ref0.sy; a.sign = q[11]; a.fwidth = fw; a.fheight = fh;
  a.xpos = cbx; a.ypos = cby; a.pu_x = pux; a.pu_y = puy; a.enable_bipred = q[12]; a.bitdepth = bitdepth; a.speed = q[13]; a.lam = lam[it];
  const mv_t mvc = mk_mv(q[7], q[8]), mvp = mk_mv(q[9], q[10]);
  const PIX* org = lds_blk ? orgc + q[4] * cb + q[3] : cur.y + (size_t)puy * cur.sy + pux;
  mv_t mv = mk_mv(0, 0);
  unsigned cost;
  if (bi) {
    const PIX* r0 = ref0.y + (size_t)cby * ref0.sy + cbx;
    const PIX* r1 = ref1.y + (size_t)cby * ref1.sy + cbx;
    cost = lds_blk ? motion_estimate_bi<PIX, SP_LDS>(t, ws.mep, org, r0, r1, a, mvc, mvp, 0, &mv) : motion_estimate_bi<PIX, SP_GLOBAL>(t, ws.mep, org, r0, r1, a, mvc, mvp, 0, &mv);
  } else {
    if (q[16]) me_stage_cb_window<PIX>(t, ws.mep, ref0.y + (size_t)cby * ref0.sy + cbx, ref0.sy, cbx, cby, cb, mvc, a.sign, fw, fh, 0);
    const PIX* rp = ref0.y + (size_t)puy * ref0.sy + pux;
    cost = lds_blk ? motion_estimate<PIX, SP_LDS>(t, ws.mep, org, rp, a, mvc, mvp, 0, &mv) : motion_estimate<PIX, SP_GLOBAL>(t, ws.mep, org, rp, a, mvc, mvp, 0, &mv);
  }
  __syncthreads();
  if (lane == 0) { out[3 * it] = mv.x; out[3 * it + 1] = mv.y; out[3 * it + 2] = (int)cost; }
  if (bi && lane < 6) { list_out[12 * it + 2 * lane] = lists->mvcand[0][lane].x; list_out[12 * it + 2 * lane + 1] = lists->mvcand[0][lane].y; }
}
// early_skip_sub / early_skip_subC (tk_block.h) on item blockIdx.x: org / pred are blocks of 32x32 samples with the size x size block in their top-left corner;
// blocks the product keeps in LDS (luma up to kLdsBlk, chroma up to kLdsBlk / 2) are copied there and take the SP_LDS instance, as in check_early_skip
template <typename PIX>
__global__ __launch_bounds__(kWgThreads, (sizeof(PIX) == 1 ? (int)kOcc : 2)) void k_kat_early_skip(const int* chroma, const PIX* org, const PIX* pred, const int* size, const int* qp,
                                                                                                   const float* thr, int bitdepth, unsigned char* big, int* out) {
  __shared__ FrameJob<PIX> sJ;
  __shared__ WgShared sh;
  __shared__ SmallWs<PIX> sws;
  __shared__ TeamWs<PIX> s_view;
  const int lane = (int)threadIdx.x, it = (int)blockIdx.x;
  lds_st(&s_view, make_ws(&sws, &sh, (BigWs<PIX>*)big));
  WsP<PIX> ws = ldsc(&s_view);
  JobR<PIX> J = *ldsc(&sJ);
  const Team t = mk_team(lane, 64, sh.tabs.izz);
  xform_tables_fill(&sh.tabs, lane, 64);
  if (lane == 0) sJ.cfg.bitdepth = bitdepth;
  const int ch = __builtin_amdgcn_readfirstlane(chroma[it]), n = __builtin_amdgcn_readfirstlane(size[it]), qpi = __builtin_amdgcn_readfirstlane(qp[it]);
  const float th = thr[it];
  const PIX* o = org + (size_t)it * 1024;
  const PIX* p = pred + (size_t)it * 1024;
  const int lds_blk = n <= (ch ? kLdsBlk / 2 : kLdsBlk);
  PIX* lo = sws.lbuf;
  PIX* lp = sws.lbuf + kLdsBlk * kLdsBlk;
  if (lds_blk)
    for (int k = lane; k < n * n; k += 64) { lo[k] = o[(k / n) * 32 + k % n]; lp[k] = p[(k / n) * 32 + k % n]; }
  __syncthreads();
  int r;
  if (ch) r = lds_blk ? early_skip_subC<PIX, SP_LDS>(t, J, ws, lo, n, lp, n, n, qpi, th) : early_skip_subC<PIX, SP_GLOBAL>(t, J, ws, o, 32, p, 32, n, qpi, th);
  else r = lds_blk ? early_skip_sub<PIX, SP_LDS>(t, J, ws, lo, n, lp, n, n, qpi, th) : early_skip_sub<PIX, SP_GLOBAL>(t, J, ws, o, 32, p, 32, n, qpi, th);
  if (lane == 0) out[it] = r;
}
}  // namespace tk

template <typename PIX>
static int kat_sad_batch(const PIX* org, int w, int h, const PIX* ref_plane, int plane_w, int plane_h, int rstride, int bx, int by, const int* cand,
                         int n, uint32_t* out) {
  if (!org || !ref_plane || !cand || !out || n <= 0 || w < 4 || h < 4 || (w & (w - 1)) || (h & (h - 1))) return 1;
  for (int i = 0; i < n; i++) {
    int x = bx + cand[2 * i], y = by + cand[2 * i + 1];
    if (x < 0 || y < 0 || x + w > plane_w || y + h > plane_h) return 2;
  }
  if (!ensure_init_any()) return 3;
  DevBuf<PIX> d_org((size_t)w * h, org);
  // the evaluator reads whole 16-byte row segments: 16 zeroed samples of slack behind the plane on the device (dev_alloc clears);
  // only the caller's rstride * plane_h samples are read from the host buffer
  DevBuf<PIX> d_ref((size_t)rstride * plane_h + 16);
  backend::h2d(d_ref, ref_plane, (size_t)rstride * plane_h * sizeof(PIX));
  DevBuf<int> d_c((size_t)2 * n, cand);
  DevBuf<uint32_t> d_o(n);
  hipLaunchKernelGGL(k_kat_sad<PIX>, dim3(1), dim3(64), 0, g_stream, d_org, w, h, d_ref, rstride, bx, by, d_c, n, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)n * 4);
  return 0;
}
extern "C" int thor_hip_sad_batch(const uint8_t* org, int w, int h, const uint8_t* ref_plane, int plane_w, int plane_h, int rstride,
                                  int bx, int by, const int* cand, int n, uint32_t* out) {
  return kat_sad_batch<uint8_t>(org, w, h, ref_plane, plane_w, plane_h, rstride, bx, by, cand, n, out);
}
extern "C" int thor_hip_sad_batch_hbd(const uint16_t* org, int w, int h, const uint16_t* ref_plane, int plane_w, int plane_h, int rstride,
                                      int bx, int by, const int* cand, int n, uint32_t* out) {
  return kat_sad_batch<uint16_t>(org, w, h, ref_plane, plane_w, plane_h, rstride, bx, by, cand, n, out);
}

template <typename PIX>
static int kat_interp_luma(const PIX* ref_plane, int plane_w, int plane_h, int rstride, int pad, int bx, int by, int w, int h, const int16_t* mv,
                           int n, int bipred, int bitdepth, PIX* out) {
  if (!ref_plane || !mv || !out || n <= 0) return 1;
  if (!ensure_init_any()) return 3;
  DevBuf<PIX> d_ref((size_t)rstride * (plane_h + 2 * pad), ref_plane);
  DevBuf<int16_t> d_mv((size_t)2 * n, mv);
  DevBuf<PIX> d_o((size_t)n * w * h);
  hipLaunchKernelGGL(k_kat_interp<PIX>, dim3(n), dim3(64), 0, g_stream, d_ref.get() + (size_t)pad * rstride + pad, rstride, plane_w, plane_h, bx,
                     by, w, h, d_mv, bipred, bitdepth, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)n * w * h * sizeof(PIX));
  return 0;
}
extern "C" int thor_hip_interp_luma(const uint8_t* ref_plane, int plane_w, int plane_h, int rstride, int pad, int bx, int by, int w,
                                    int h, const int16_t* mv, int n, int bipred, uint8_t* out) {
  return kat_interp_luma<uint8_t>(ref_plane, plane_w, plane_h, rstride, pad, bx, by, w, h, mv, n, bipred, 8, out);
}
extern "C" int thor_hip_interp_luma_hbd(const uint16_t* ref_plane, int plane_w, int plane_h, int rstride, int pad, int bx, int by, int w,
                                        int h, const int16_t* mv, int n, int bipred, int bitdepth, uint16_t* out) {
  if (bitdepth < 9 || bitdepth > 12) return 1;
  return kat_interp_luma<uint16_t>(ref_plane, plane_w, plane_h, rstride, pad, bx, by, w, h, mv, n, bipred, bitdepth, out);
}

template <typename PIX>
static int kat_code_tu_batch(const PIX* org, const PIX* pred, int size, int qp, int coeff_type, int fast, int n, int bitdepth, int16_t* coefq,
                             PIX* rec, int* cbp) {
  if (!org || !pred || !coefq || !rec || !cbp || n <= 0) return 1;
  if (size != 4 && size != 8 && size != 16 && size != 32 && size != 64 && size != 128) return 2;
  if (!ensure_init_any()) return 3;
  const size_t px = (size_t)n * size * size;
  const int qs = size < 16 ? size : 16;
  DevBuf<PIX> d_org(px, org), d_pred(px, pred), d_rec(px);
  DevBuf<int16_t> d_cq((size_t)n * qs * qs);
  DevBuf<int> d_cbp(n);
  hipLaunchKernelGGL(k_kat_tu<PIX>, dim3(n), dim3(64), 0, g_stream, d_org, d_pred, size, qp, coeff_type, fast, bitdepth, d_cq, d_rec,
                     d_cbp);
  HIPCHECK(hipGetLastError());
  backend::d2h(coefq, d_cq, (size_t)n * qs * qs * 2);
  backend::d2h(rec, d_rec, px * sizeof(PIX));
  backend::d2h(cbp, d_cbp, (size_t)n * 4);
  return 0;
}
extern "C" int thor_hip_code_tu_batch(const uint8_t* org, const uint8_t* pred, int size, int qp, int coeff_type, int fast, int n,
                                      int16_t* coefq, uint8_t* rec, int* cbp) {
  return kat_code_tu_batch<uint8_t>(org, pred, size, qp, coeff_type, fast, n, 8, coefq, rec, cbp);
}
extern "C" int thor_hip_code_tu_batch_hbd(const uint16_t* org, const uint16_t* pred, int size, int qp, int coeff_type, int fast, int n,
                                          int bitdepth, int16_t* coefq, uint16_t* rec, int* cbp) {
  if (bitdepth < 9 || bitdepth > 12) return 1;
  return kat_code_tu_batch<uint16_t>(org, pred, size, qp, coeff_type, fast, n, bitdepth, coefq, rec, cbp);
}

template <typename PIX> static int kat_deblock_frame(PIX* yuv, int width, int height, int qp, int bitdepth, const thor_hip_cell* cells) {
  static_assert(sizeof(thor_hip_cell) == sizeof(DbCell), "thor_hip_cell must mirror tk::DbCell");
  if (!yuv || !cells || width % 8 || height % 8 || width < 16 || height < 16 || qp < 0 || qp > 51) return 1;
  if (!ensure_init_any()) return 3;
  DevFrame<PIX> f;
  f.alloc(width, height, 0);
  DevBuf<DbCell> d_cells((size_t)(width / 4) * (height / 4), (const DbCell*)cells);
  upload_yuv(f, yuv, width, height);
  FrameJob<PIX> J;
  memset(&J, 0, sizeof(J));
  J.cfg.width = width; J.cfg.height = height; J.cfg.bitdepth = bitdepth;
  J.qp = qp; J.rec = f.p; J.cells = d_cells; J.cell_stride = width / 4;
  DevBuf<FrameJob<PIX>> d_job(1, &J);
  backend::run_deblock<PIX>(d_job, &J, 1);
  backend::dev_sync();
  download_yuv(f, yuv, width, height);
  f.release();
  return 0;
}
extern "C" int thor_hip_deblock_frame(uint8_t* yuv, int width, int height, int qp, const thor_hip_cell* cells) {
  return kat_deblock_frame<uint8_t>(yuv, width, height, qp, 8, cells);
}
extern "C" int thor_hip_deblock_frame_hbd(uint16_t* yuv, int width, int height, int qp, int bitdepth, const thor_hip_cell* cells) {
  if (bitdepth < 9 || bitdepth > 12) return 1;
  return kat_deblock_frame<uint16_t>(yuv, width, height, qp, bitdepth, cells);
}

// ---- round 6: known-answer entry points for intra prediction, inter prediction of a whole block (luma + chroma, quadrant split), the
// bi-prediction average, chroma-from-luma, the CDEF direction search / filter, CLPF and the temporally interpolated reference --------------
namespace {
template <typename PIX>
int kat_intra(const PIX* plane, int width, int height, int stride, int bitdepth, int size, int tb_split, int n, const int* par, const PIX* rblocks, PIX* out) {
  if (!plane || !par || !out || n <= 0 || size < 4 || size > 64 || (size & (size - 1)) || (tb_split && !rblocks) || stride < width) return 1;
  const int cbs = tb_split ? 2 * size : size;
  for (int i = 0; i < n; i++) {
    const int* q = par + 7 * i;
    if (q[0] < 0 || q[1] < 0 || q[0] + cbs > height || q[1] + cbs > width || q[4] < 0 || q[5] < 0 || q[6] < 0 || q[5] + size > cbs || q[6] + size > cbs) return 2;
    if ((q[2] && q[1] + 2 * cbs > width) || (q[3] && q[0] + 2 * cbs > height)) return 2;   // up-right / down-left samples must exist
  }
  if (!ensure_init_any()) return 3;
  DevBuf<PIX> d_p((size_t)stride * height, plane);
  DevBuf<int> d_par((size_t)7 * n, par);
  DevBuf<PIX> d_rb(tb_split ? (size_t)n * cbs * cbs : 0, tb_split ? rblocks : nullptr);   // without tb_split the kernel does not read it
  DevBuf<PIX> d_o((size_t)n * size * size);
  hipLaunchKernelGGL(k_kat_intra<PIX>, dim3(n), dim3(64), 0, g_stream, d_p, stride, bitdepth, size, tb_split, d_par, d_rb, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)n * size * size * sizeof(PIX));
  return 0;
}
// frame with the reference windows' replicate padding (what k_make_ref produces from a reconstruction)
template <typename PIX> DevFrame<PIX> kat_padded_ref(const PIX* yuv, int width, int height) {
  DevFrame<PIX> rec, ref;
  rec.alloc(width, height, 0);
  ref.alloc(width, height, kPadY);
  upload_yuv(rec, yuv, width, height);
  FrameJob<PIX> J;
  memset(&J, 0, sizeof(J));
  J.cfg.width = width; J.cfg.height = height; J.rec = rec.p;
  backend::run_make_ref<PIX>(&J, &ref.p, 1);
  backend::dev_sync();
  rec.release();
  return ref;
}
template <typename PIX>
int kat_inter_yuv(const PIX* yuv, int width, int height, int bitdepth, int size, int n, const int* par, const int16_t* mv, PIX* out) {
  if (!yuv || !par || !mv || !out || n <= 0 || size < 8 || size > 128 || (size & (size - 1)) || width % 8 || height % 8) return 1;
  for (int i = 0; i < n; i++) {
    const int* q = par + 5 * i;
    if (q[0] < 0 || q[1] < 0 || q[0] + size > height || q[1] + size > width || (q[4] && size < 16)) return 2;
  }
  if (!ensure_init_any()) return 3;
  DevFrame<PIX> ref = kat_padded_ref(yuv, width, height);
  DevBuf<int> d_par((size_t)5 * n, par);
  DevBuf<int16_t> d_mv((size_t)8 * n, mv);
  const size_t per = (size_t)size * size * 3 / 2;
  DevBuf<PIX> d_o(per * n);
  hipLaunchKernelGGL(k_kat_inter_yuv<PIX>, dim3(n), dim3(64), 0, g_stream, ref.p, width, height, bitdepth, size, d_par, d_mv, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, per * n * sizeof(PIX));
  ref.release();
  return 0;
}
template <typename PIX> int kat_average(const PIX* a, const PIX* b, int size, int n, PIX* out) {
  if (!a || !b || !out || n <= 0 || size < 8 || size > 128 || (size & (size - 1))) return 1;
  if (!ensure_init_any()) return 3;
  const size_t tot = (size_t)n * size * size * 3 / 2;
  DevBuf<PIX> d_a(tot, a), d_b(tot, b), d_o(tot);
  hipLaunchKernelGGL(k_kat_average<PIX>, dim3(n), dim3(64), 0, g_stream, d_a, d_b, size, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, tot * sizeof(PIX));
  return 0;
}
template <typename PIX> int kat_cfl(const PIX* y, PIX* uv, const PIX* ry, int nl, int bitdepth, int n) {
  if (!y || !uv || !ry || n <= 0 || nl < 8 || nl > 128 || (nl & (nl - 1))) return 1;
  if (!ensure_init_any()) return 3;
  const size_t ny = (size_t)n * nl * nl, nc = (size_t)n * 2 * (nl / 2) * (nl / 2);
  DevBuf<PIX> d_y(ny, y), d_r(ny, ry), d_uv(nc, uv);
  hipLaunchKernelGGL(k_kat_cfl<PIX>, dim3(n), dim3(64), 0, g_stream, d_y, d_uv, d_r, nl, bitdepth);
  HIPCHECK(hipGetLastError());
  backend::d2h(uv, d_uv, nc * sizeof(PIX));
  return 0;
}
template <typename PIX> int kat_cdef_dir(const PIX* blocks, int bitdepth, int n, int* dir, int* var) {
  if (!blocks || !dir || !var || n <= 0) return 1;
  if (!ensure_init_any()) return 3;
  DevBuf<PIX> d_b((size_t)n * 64, blocks);
  DevBuf<int> d_d(n), d_v(n);
  hipLaunchKernelGGL(k_kat_cdef_dir<PIX>, dim3((n + 63) / 64), dim3(64), 0, g_stream, d_b, n, bitdepth - 8, d_d, d_v);
  HIPCHECK(hipGetLastError());
  backend::d2h(dir, d_d, (size_t)n * 4); backend::d2h(var, d_v, (size_t)n * 4);
  return 0;
}
template <typename PIX> int kat_cdef_filter(const PIX* plane, int w, int h, int stride, int bitdepth, int bsize, int n, const int* par, PIX* out) {
  if (!plane || !par || !out || n <= 0 || (bsize != 4 && bsize != 8) || stride < w) return 1;
  for (int i = 0; i < n; i++) {
    const int* q = par + 7 * i;
    if (q[0] < 0 || q[1] < 0 || q[0] + bsize > w || q[1] + bsize > h || q[4] < 0 || q[4] > 7) return 2;
  }
  if (!ensure_init_any()) return 3;
  DevBuf<PIX> d_p((size_t)stride * h, plane);
  DevBuf<int> d_par((size_t)7 * n, par);
  DevBuf<PIX> d_o((size_t)n * bsize * bsize);
  hipLaunchKernelGGL(k_kat_cdef_filter<PIX>, dim3(n), dim3(64), 0, g_stream, d_p, w, h, stride, bsize, bitdepth - 8, d_par, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)n * bsize * bsize * sizeof(PIX));
  return 0;
}
// CLPF: the two device passes of the product (statistics per 8x8 block, filter per 8x8 luma / 4x4 chroma unit) on one frame.
template <typename PIX>
int kat_clpf(const PIX* rec_yuv, const PIX* org_yuv, int width, int height, int bitdepth, int qp, const thor_hip_cell* cells, const int* strength, int fb_log2,
             const uint8_t* fb_on, uint32_t* stats, PIX* out_yuv) {
  if (!rec_yuv || !org_yuv || !cells || !strength || !fb_on || !stats || !out_yuv || width % 16 || height % 16 || fb_log2 < 5 || fb_log2 > 7) return 1;
  if (!ensure_init_any()) return 3;
  DevFrame<PIX> rec, src, org;
  rec.alloc(width, height, 0); src.alloc(width, height, 0); org.alloc(width, height, 0);
  upload_yuv(rec, rec_yuv, width, height); upload_yuv(src, rec_yuv, width, height); upload_yuv(org, org_yuv, width, height);
  DevBuf<DbCell> d_cells((size_t)(width / 4) * (height / 4), (const DbCell*)cells);
  const int nblk = (width / 8) * (height / 8) + 2 * (width / 16) * (height / 16);
  const int nfb = ((width + (1 << fb_log2) - 1) >> fb_log2) * ((height + (1 << fb_log2) - 1) >> fb_log2);
  DevBuf<uint32_t> d_stats((size_t)4 * nblk);
  DevBuf<uint8_t> d_on((size_t)nfb, fb_on);
  ClpfJob<PIX> J;
  memset(&J, 0, sizeof(J));
  J.rec = rec.p; J.src = src.p; J.org = org.p; J.width = width; J.height = height; J.bitdepth = bitdepth; J.qp = qp;
  J.cells = d_cells; J.cs = width / 4; J.stats = d_stats;
  for (int k = 0; k < 3; k++) J.strength[k] = strength[k];
  J.fb_log2 = fb_log2; J.fb_on = d_on;
  DevBuf<ClpfJob<PIX>> d_job(1, &J);
  backend::run_clpf_stats<PIX>(d_job, &J, 1);
  backend::run_clpf_apply<PIX>(d_job, &J, 1);
  backend::dev_sync();
  backend::d2h(stats, d_stats, (size_t)4 * nblk * 4);
  download_yuv(rec, out_yuv, width, height);
  rec.release(); src.release(); org.release();
  return 0;
}
// The CDEF strength search and frame filter of `S` frames of one size through the product's launch sequence: CdefJobs filled as Engine::finish_frames fills
// them (qp, speed and the cdef_bits guess per job), one backend::run_cdef call (copy + the five passes), everything the passes left behind copied back.
template <typename PIX>
int kat_cdef_frame(int S, const PIX* rec_yuv, const PIX* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, const int* qp, const int* speed, const int* cdef_bits,
                   int8_t* dir, int* var, int* fb_compact, unsigned long long* mse, int* res, int* fb_sel, PIX* out_yuv) {
  if (!rec_yuv || !org_yuv || !mode || !qp || !speed || !cdef_bits || !dir || !var || !fb_compact || !mse || !res || !fb_sel || !out_yuv) return 1;
  if (S <= 0 || S > 64 || width < 8 || height < 8 || width % 8 || height % 8 || width > 8192 || height > 8192) return 1;
  for (int s = 0; s < S; s++)
    if (speed[s] < 0 || speed[s] > 2 || cdef_bits[s] < 0 || cdef_bits[s] > 3 || qp[s] < 0 || qp[s] > 51) return 1;
  if (!ensure_init_any()) return 3;
  static_assert(sizeof(CdefResult) % sizeof(int) == 0, "CdefResult is returned as ints");
  const int nfb_h = (width + 63) / 64, nfb_v = (height + 63) / 64, nfb = nfb_h * nfb_v, nb8 = (width / 8) * (height / 8);
  const size_t fsz = (size_t)width * height * 3 / 2, ncell = (size_t)(width / 4) * (height / 4);
  std::vector<DevFrame<PIX>> rec(S), src(S), org(S);
  std::vector<DbCell> cells(ncell * S);
  memset(cells.data(), 0, cells.size() * sizeof(DbCell));
  for (size_t i = 0; i < cells.size(); i++) { cells[i].mode = mode[i]; cells[i].size = 8; }
  DevBuf<DbCell> d_cells(cells.size(), cells.data());
  DevBuf<int8_t> d_dir((size_t)nb8 * S);
  DevBuf<int> d_var((size_t)nb8 * S), d_fbc((size_t)nfb * S), d_sel((size_t)nfb * S), d_fbsel((size_t)nfb * S);
  DevBuf<unsigned long long> d_mse((size_t)2 * nfb * kCdefMaxStr * S), d_tot(((size_t)kCdefMaxStr * kCdefMaxStr + nfb) * S);
  DevBuf<CdefResult> d_res(S);
  backend::dev_memset(d_dir, 0, (size_t)nb8 * S); backend::dev_memset(d_var, 0, (size_t)nb8 * S * sizeof(int));
  backend::dev_memset(d_sel, 0, (size_t)nfb * S * sizeof(int)); backend::dev_memset(d_res, 0, sizeof(CdefResult) * S);
  std::vector<CdefJob<PIX>> J(S);
  for (int s = 0; s < S; s++) {
    rec[s].alloc(width, height, 0); src[s].alloc(width, height, 0); org[s].alloc(width, height, 0);
    upload_yuv(rec[s], rec_yuv + fsz * s, width, height); upload_yuv(org[s], org_yuv + fsz * s, width, height);
    CdefJob<PIX>& C = J[s];
    memset(&C, 0, sizeof(C));
    C.rec = rec[s].p; C.src = src[s].p; C.org = org[s].p;
    C.width = width; C.height = height; C.bitdepth = bitdepth;
    C.cells = d_cells + ncell * s; C.cs = width / 4; C.nfb_h = nfb_h; C.nfb_v = nfb_v;
    C.speed = speed[s]; C.damping = 5; C.cdef_bits = cdef_bits[s]; C.qp = qp[s];
    C.dir = d_dir + (size_t)nb8 * s; C.var = d_var + (size_t)nb8 * s; C.fb_compact = d_fbc + (size_t)nfb * s;
    C.mse = d_mse + (size_t)2 * nfb * kCdefMaxStr * s; C.sel = d_sel + (size_t)nfb * s; C.fb_sel = d_fbsel + (size_t)nfb * s;
    C.res = d_res + s; C.tot = d_tot + ((size_t)kCdefMaxStr * kCdefMaxStr + nfb) * s;
  }
  {
    DevBuf<CdefJob<PIX>> d_jobs(S, J.data());
    backend::run_cdef<PIX>(d_jobs, J.data(), S);
    HIPCHECK(hipGetLastError());
    backend::dev_sync();
  }
  backend::d2h(dir, d_dir, (size_t)nb8 * S); backend::d2h(var, d_var, (size_t)nb8 * S * sizeof(int));
  backend::d2h(fb_compact, d_fbc, (size_t)nfb * S * sizeof(int)); backend::d2h(fb_sel, d_fbsel, (size_t)nfb * S * sizeof(int));
  backend::d2h(mse, d_mse, (size_t)2 * nfb * kCdefMaxStr * S * 8); backend::d2h(res, d_res, sizeof(CdefResult) * S);
  for (int s = 0; s < S; s++) {
    download_yuv(rec[s], out_yuv + fsz * s, width, height);
    rec[s].release(); src[s].release(); org[s].release();
  }
  return 0;
}
// interpolate_frames(new, ref0, ref1, 2, 1) (common/temporal_interp.c:909) through the engine's own path (Engine::make_interp_frames, tk_interp_dev.h)
template <typename PIX> int kat_interpolate(const PIX* yuv0, const PIX* yuv1, int width, int height, int bitdepth, PIX* out_yuv) {
  if (!yuv0 || !yuv1 || !out_yuv || width % 8 || height % 8 || width < 64 || height < 64) return 1;
  if (!ensure_init_any()) return 3;
  SeqParams sp;
  sp.width = width; sp.height = height; sp.bitdepth = bitdepth; sp.input_bitdepth = bitdepth;
  sp.num_reorder_pics = 7; sp.interp_ref = 1; sp.max_num_ref = 2; sp.HQperiod = 8; sp.cdef = 0; sp.clpf = 0;
  Engine<PIX>* eng = new Engine<PIX>();
  eng->open(sp, 1);
  Stream<PIX>& q = eng->st[0];
  for (int k = 0; k < 2; k++) {
    upload_yuv(q.rec, k ? yuv1 : yuv0, width, height);
    FrameJob<PIX> J;
    memset(&J, 0, sizeof(J));
    J.cfg.width = width; J.cfg.height = height; J.rec = q.rec.p;
    backend::run_make_ref<PIX>(&J, &q.ring[k].p, 1);
    backend::dev_sync();
  }
  std::vector<FrameParams> fp(1);
  fp[0].interp_ref = 1; fp[0].interp_src[0] = 0; fp[0].interp_src[1] = 1; fp[0].frame_num = 1;
  eng->make_interp_frames(fp, 0, 1);
  backend::dev_sync();
  download_yuv(q.interp, out_yuv, width, height);
  eng->close();
  delete eng;
  return 0;
}
// motion_estimate / motion_estimate_bi / me_stage_cb_window (tk_me.h) on `n` items of one current / reference luma frame pair (bi: two references)
template <typename PIX> DevFrame<PIX> kat_luma_frame(const PIX* luma, int width, int height, int pad_ref) {
  std::vector<PIX> yuv((size_t)width * height * 3 / 2, (PIX)0);
  memcpy(yuv.data(), luma, (size_t)width * height * sizeof(PIX));
  if (pad_ref) return kat_padded_ref(yuv.data(), width, height);
  DevFrame<PIX> f;
  f.alloc(width, height, 0);
  upload_yuv(f, yuv.data(), width, height);
  return f;
}
template <typename PIX>
int kat_me(int bi, const PIX* cur, const PIX* ref0, const PIX* ref1, int width, int height, int bitdepth, int n, const int* par, const double* lam, const int16_t* cand,
           int ncand_total, int* out, int16_t* list_out) {
  if (!cur || !ref0 || (bi && (!ref1 || !list_out)) || !par || !lam || !out || n <= 0 || ncand_total < 0 || (ncand_total && !cand) || width % 8 || height % 8 || width < 16 ||
      height < 16 || width > 8192 || height > 8192)
    return 1;
  auto pow2 = [](int v, int lo, int hi) { return v >= lo && v <= hi && !(v & (v - 1)); };
  for (int i = 0; i < n; i++) {
    const int* q = par + kKatMePar * i;
    if (!pow2(q[2], 8, kMaxSb) || !pow2(q[5], 4, q[2]) || !pow2(q[6], 4, q[2]) || (q[11] & ~1) || (q[12] & ~1) || q[13] < 0 || q[13] > 2 || !(lam[i] >= 0.0 && lam[i] <= 1e6)) return 1;
    if (q[0] < 0 || q[1] < 0 || q[0] + q[2] > width || q[1] + q[2] > height || q[3] < 0 || q[4] < 0 || q[3] + q[5] > q[2] || q[4] + q[6] > q[2] || q[3] % 4 || q[4] % 4) return 2;
    for (int k = 7; k <= 10; k++) if (q[k] < -8192 || q[k] > 8192) return 1;   // vectors are int16 quarter-pels; the search adds up to +-128 to them
    const int slots = bi ? 6 : q[14];
    if (q[14] < 0 || q[14] > (bi ? 6 : 64) || q[15] < 0 || q[15] + slots > ncand_total) return 2;
    if (bi && (q[3] || q[4] || q[5] != q[2] || q[6] != q[2])) return 1;
    for (int c = 0; c < slots; c++) if (cand[2 * (q[15] + c)] < -2047 || cand[2 * (q[15] + c)] > 2047 || cand[2 * (q[15] + c) + 1] < -2047 || cand[2 * (q[15] + c) + 1] > 2047) return 1;
  }
  if (!ensure_init_any()) return 3;
  DevFrame<PIX> fc = kat_luma_frame(cur, width, height, 0), f0 = kat_luma_frame(ref0, width, height, 1), f1 = bi ? kat_luma_frame(ref1, width, height, 1) : DevFrame<PIX>();
  {
    DevBuf<int> d_par((size_t)kKatMePar * n, par);
    DevBuf<double> d_lam(n, lam);
    DevBuf<int16_t> d_cand((size_t)2 * (ncand_total ? ncand_total : 1));
    if (ncand_total) backend::h2d(d_cand, cand, (size_t)4 * ncand_total);
    DevBuf<unsigned char> d_big(sizeof(BigWs<PIX>));   // the per-wave global scratch make_ws points at; the searches do not touch it
    DevBuf<int> d_o((size_t)3 * n);
    DevBuf<int16_t> d_l((size_t)12 * n);
    hipLaunchKernelGGL(k_kat_me<PIX>, dim3(n), dim3(64), 0, g_stream, bi, fc.p, f0.p, bi ? f1.p : f0.p, width, height, bitdepth, d_par, d_lam, d_cand, d_big, d_o, d_l);
    HIPCHECK(hipGetLastError());
    backend::d2h(out, d_o, (size_t)3 * n * 4);
    if (bi) backend::d2h(list_out, d_l, (size_t)12 * n * 2);
  }
  fc.release(); f0.release();
  if (bi) f1.release();
  return 0;
}
template <typename PIX>
int kat_early_skip(const int* chroma, const PIX* org, const PIX* pred, const int* size, const int* qp, const float* thr, int bitdepth, int n, int* out) {
  if (!chroma || !org || !pred || !size || !qp || !thr || !out || n <= 0) return 1;
  for (int i = 0; i < n; i++) {
    const int s = size[i];
    if ((chroma[i] & ~1) || qp[i] < 0 || qp[i] > 51 || !(thr[i] >= 0.0f && thr[i] <= 1e3f)) return 1;
    if (chroma[i] ? (s != 4 && s != 8 && s != 16) : (s != 8 && s != 16 && s != 32)) return 2;
  }
  if (!ensure_init_any()) return 3;
  DevBuf<PIX> d_org((size_t)n * 1024, org), d_pred((size_t)n * 1024, pred);
  DevBuf<int> d_ch(n, chroma), d_size(n, size), d_qp(n, qp), d_o(n);
  DevBuf<float> d_thr(n, thr);
  DevBuf<unsigned char> d_big(sizeof(BigWs<PIX>));
  hipLaunchKernelGGL(k_kat_early_skip<PIX>, dim3(n), dim3(64), 0, g_stream, d_ch, d_org, d_pred, d_size, d_qp, d_thr, bitdepth, d_big, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)n * 4);
  return 0;
}
}  // namespace
#define KAT_BD(call8, call16) do { if (bitdepth == 8) return call8; if (bitdepth >= 9 && bitdepth <= 12) return call16; return 1; } while (0)
extern "C" int thor_hip_kat_intra(const void* plane, int width, int height, int stride, int bitdepth, int size, int tb_split, int n, const int* par,
                                  const void* rblocks, void* out) {
  KAT_BD(kat_intra<uint8_t>((const uint8_t*)plane, width, height, stride, 8, size, tb_split, n, par, (const uint8_t*)rblocks, (uint8_t*)out),
         kat_intra<uint16_t>((const uint16_t*)plane, width, height, stride, bitdepth, size, tb_split, n, par, (const uint16_t*)rblocks, (uint16_t*)out));
}
extern "C" int thor_hip_kat_inter_yuv(const void* yuv, int width, int height, int bitdepth, int size, int n, const int* par, const int16_t* mv, void* out) {
  KAT_BD(kat_inter_yuv<uint8_t>((const uint8_t*)yuv, width, height, 8, size, n, par, mv, (uint8_t*)out),
         kat_inter_yuv<uint16_t>((const uint16_t*)yuv, width, height, bitdepth, size, n, par, mv, (uint16_t*)out));
}
extern "C" int thor_hip_kat_average(const void* a, const void* b, int size, int bitdepth, int n, void* out) {
  KAT_BD(kat_average<uint8_t>((const uint8_t*)a, (const uint8_t*)b, size, n, (uint8_t*)out),
         kat_average<uint16_t>((const uint16_t*)a, (const uint16_t*)b, size, n, (uint16_t*)out));
}
extern "C" int thor_hip_kat_cfl(const void* y, void* uv, const void* ry, int n_luma, int bitdepth, int n) {
  KAT_BD(kat_cfl<uint8_t>((const uint8_t*)y, (uint8_t*)uv, (const uint8_t*)ry, n_luma, 8, n),
         kat_cfl<uint16_t>((const uint16_t*)y, (uint16_t*)uv, (const uint16_t*)ry, n_luma, bitdepth, n));
}
extern "C" int thor_hip_kat_cdef_dir(const void* blocks, int bitdepth, int n, int* dir, int* var) {
  KAT_BD(kat_cdef_dir<uint8_t>((const uint8_t*)blocks, 8, n, dir, var), kat_cdef_dir<uint16_t>((const uint16_t*)blocks, bitdepth, n, dir, var));
}
extern "C" int thor_hip_kat_cdef_filter(const void* plane, int width, int height, int stride, int bitdepth, int bsize, int n, const int* par, void* out) {
  KAT_BD(kat_cdef_filter<uint8_t>((const uint8_t*)plane, width, height, stride, 8, bsize, n, par, (uint8_t*)out),
         kat_cdef_filter<uint16_t>((const uint16_t*)plane, width, height, stride, bitdepth, bsize, n, par, (uint16_t*)out));
}
extern "C" int thor_hip_kat_clpf(const void* rec_yuv, const void* org_yuv, int width, int height, int bitdepth, int qp, const thor_hip_cell* cells,
                                 const int* strength, int fb_log2, const uint8_t* fb_on, uint32_t* stats, void* out_yuv) {
  KAT_BD(kat_clpf<uint8_t>((const uint8_t*)rec_yuv, (const uint8_t*)org_yuv, width, height, 8, qp, cells, strength, fb_log2, fb_on, stats, (uint8_t*)out_yuv),
         kat_clpf<uint16_t>((const uint16_t*)rec_yuv, (const uint16_t*)org_yuv, width, height, bitdepth, qp, cells, strength, fb_log2, fb_on, stats, (uint16_t*)out_yuv));
}
extern "C" int thor_hip_kat_cdef_frame(int n_jobs, const void* rec_yuv, const void* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, const int* qp,
                                       const int* speed, const int* cdef_bits, int8_t* dir, int* var, int* fb_compact, unsigned long long* mse, int* result, int* fb_sel, void* out_yuv) {
  KAT_BD(kat_cdef_frame<uint8_t>(n_jobs, (const uint8_t*)rec_yuv, (const uint8_t*)org_yuv, mode, width, height, 8, qp, speed, cdef_bits, dir, var, fb_compact, mse, result, fb_sel,
                                 (uint8_t*)out_yuv),
         kat_cdef_frame<uint16_t>(n_jobs, (const uint16_t*)rec_yuv, (const uint16_t*)org_yuv, mode, width, height, bitdepth, qp, speed, cdef_bits, dir, var, fb_compact, mse, result,
                                  fb_sel, (uint16_t*)out_yuv));
}
extern "C" int thor_hip_kat_motion_estimate(const void* cur, const void* ref, int width, int height, int bitdepth, int n, const int* par, const double* lambda,
                                            const int16_t* cand, int ncand_total, int* out) {
  KAT_BD(kat_me<uint8_t>(0, (const uint8_t*)cur, (const uint8_t*)ref, nullptr, width, height, 8, n, par, lambda, cand, ncand_total, out, nullptr),
         kat_me<uint16_t>(0, (const uint16_t*)cur, (const uint16_t*)ref, nullptr, width, height, bitdepth, n, par, lambda, cand, ncand_total, out, nullptr));
}
extern "C" int thor_hip_kat_motion_estimate_bi(const void* cur, const void* ref0, const void* ref1, int width, int height, int bitdepth, int n, const int* par,
                                               const double* lambda, const int16_t* cand, int* out, int16_t* list_out) {
  KAT_BD(kat_me<uint8_t>(1, (const uint8_t*)cur, (const uint8_t*)ref0, (const uint8_t*)ref1, width, height, 8, n, par, lambda, cand, 6 * n, out, list_out),
         kat_me<uint16_t>(1, (const uint16_t*)cur, (const uint16_t*)ref0, (const uint16_t*)ref1, width, height, bitdepth, n, par, lambda, cand, 6 * n, out, list_out));
}
extern "C" int thor_hip_kat_early_skip(const int* chroma, const void* org, const void* pred, const int* size, const int* qp, const float* thr, int bitdepth, int n, int* out) {
  KAT_BD(kat_early_skip<uint8_t>(chroma, (const uint8_t*)org, (const uint8_t*)pred, size, qp, thr, 8, n, out),
         kat_early_skip<uint16_t>(chroma, (const uint16_t*)org, (const uint16_t*)pred, size, qp, thr, bitdepth, n, out));
}
// ---- the block syntax (tk_bits.h) against the reference's bit strings: tests/golden/gen_kat9.py -> kat9.npz.  The two kernels live in a translation unit of
// their own (thor_hip_katbits.cpp says why); k_gather_bits is the throughput build's ------------------------------------------------------------------------
extern "C" int thor_hip_kat_coeff_syntax(int n, const int* par, const int16_t* coef, int words, uint32_t* buf_single, uint32_t* buf_team, int* out) {
  if (n <= 0 || !par || !coef || words <= 0 || words > (1 << 16) || !buf_single || !buf_team || !out) return 1;
  for (int i = 0; i < n; i++) if (kat_coeff_check(par + kKatCoPar * i, words)) return 1;
  if (!ensure_init_any()) return 3;
  DevBuf<int> d_par((size_t)kKatCoPar * n, par), d_o((size_t)kKatCoOut * n);
  DevBuf<int16_t> d_c((size_t)256 * n, coef);
  DevBuf<uint32_t> d_1((size_t)words * n, buf_single), d_t((size_t)words * n, buf_team);
  if (thor_katbits_launch_coeff(g_stream, n, d_par, d_c, words, d_1, d_t, d_o)) return 3;
  backend::d2h(buf_single, d_1, (size_t)words * n * 4); backend::d2h(buf_team, d_t, (size_t)words * n * 4);
  backend::d2h(out, d_o, (size_t)kKatCoOut * n * 4);
  return 0;
}
extern "C" int thor_hip_kat_block_syntax(int n, const int* par, const int16_t* pool, int npool, int words, uint32_t* buf_coop, uint32_t* buf_single, int* out) {
  if (n <= 0 || !par || npool < 0 || (npool && !pool) || words <= 0 || words > (1 << 16) || !buf_coop || !buf_single || !out) return 1;
  std::vector<int16_t> coef((size_t)n * 3072);
  for (int i = 0; i < n; i++) if (kat_block_resolve(par + kKatBlPar * i, pool, npool, coef.data() + (size_t)i * 3072)) return 1;
  if (!ensure_init_any()) return 3;
  DevBuf<int> d_par((size_t)kKatBlPar * n, par), d_o((size_t)kKatBlOut * n);
  DevBuf<int16_t> d_c(coef.size(), coef.data());
  DevBuf<uint32_t> d_w((size_t)words * n, buf_coop), d_1((size_t)words * n, buf_single);
  if (thor_katbits_launch_block(g_stream, n, d_par, d_c, words, d_w, d_1, d_o)) return 3;
  backend::d2h(buf_coop, d_w, (size_t)words * n * 4); backend::d2h(buf_single, d_1, (size_t)words * n * 4);
  backend::d2h(out, d_o, (size_t)kKatBlOut * n * 4);
  return 0;
}
extern "C" int thor_hip_kat_gather_bits(int n, const uint32_t* src, int src_words, const int* src_off, const int* nbits, const long long* dst_bit, uint32_t* dst, int dst_words) {
  if (n <= 0 || !src || src_words <= 0 || !src_off || !nbits || !dst_bit || !dst || dst_words <= 0) return 1;
  for (int i = 0; i < n; i++) {
    if (nbits[i] < 0 || src_off[i] < 0 || dst_bit[i] < 0) return 1;
    if ((long long)src_off[i] + (nbits[i] + 31) / 32 > src_words || dst_bit[i] + nbits[i] > (long long)dst_words * 32) return 2;
  }
  if (!ensure_init_any()) return 3;
  std::vector<backend::GatherItem> items(n);
  DevBuf<uint32_t> d_src((size_t)src_words, src), d_dst((size_t)dst_words);   // destination zeroed (dev_alloc clears)
  for (int i = 0; i < n; i++) {
    items[i].src = d_src.get() + src_off[i]; items[i].nbits = nbits[i]; items[i].dst_bit = dst_bit[i];
  }
  DevBuf<backend::GatherItem> d_items((size_t)n, items.data());
  backend::run_gather(d_items, n, d_dst);
  backend::d2h(dst, d_dst, (size_t)dst_words * 4);
  return 0;
}
// Per-plane SSE of two host frames through k_frame_sse (the kernel the engine launches with frame distortion on).
template <typename PIX> int frame_sse_host(const PIX* a, const PIX* b, int width, int height, unsigned long long out[3]) {
  if (!a || !b || !out || width % 8 || height % 8 || width < 8 || height < 8) return 1;
  if (!ensure_init_any()) return 3;
  DevFrame<PIX> fa, fb;
  fa.alloc(width, height, 0); fb.alloc(width, height, 0);
  upload_yuv(fa, a, width, height); upload_yuv(fb, b, width, height);
  FrameJob<PIX> J;
  memset(&J, 0, sizeof(J));
  J.cfg.width = width; J.cfg.height = height; J.orig = fa.p; J.rec = fb.p;
  DevBuf<FrameJob<PIX>> dj(1, &J);
  DevBuf<unsigned long long> dout(4);  // zeroed
  launch_frame_sse<PIX>(dj, &J, 1, dout);
  backend::dev_sync();
  backend::d2h(out, dout, 3 * sizeof(unsigned long long));
  fa.release(); fb.release();
  return 0;
}
extern "C" int thor_hip_frame_sse(const void* a, const void* b, int w, int h, int bitdepth, unsigned long long out[3]) {
  KAT_BD(frame_sse_host<uint8_t>((const uint8_t*)a, (const uint8_t*)b, w, h, out),
         frame_sse_host<uint16_t>((const uint16_t*)a, (const uint16_t*)b, w, h, out));
}
// The three kernels of the mixed-depth path (bitdepth > input_bitdepth) on host frames: packed planar 4:2:0, input-depth samples one byte each for depth 8
// and two otherwise, engine-depth samples uint16_t.
static int kat_depth_args(const void* a, const void* b, int w, int h, int bitdepth, int input_bitdepth) {
  auto ok = [](int d) { return d == 8 || d == 10 || d == 12; };
  return !a || !b || w % 8 || h % 8 || w < 8 || h < 8 || !ok(bitdepth) || !ok(input_bitdepth) || input_bitdepth >= bitdepth;
}
extern "C" int thor_hip_kat_depth_up(const void* in, int w, int h, int bitdepth, int input_bitdepth, uint16_t* out) {
  if (kat_depth_args(in, out, w, h, bitdepth, input_bitdepth)) return 1;
  if (!ensure_init_any()) return 3;
  const size_t bytes = (size_t)w * h * 3 / 2 * (input_bitdepth > 8 ? 2 : 1);
  DevBuf<uint8_t> packed(bytes, (const uint8_t*)in);
  DevFrame<uint16_t> f;
  f.alloc(w, h, 0);
  launch_depth_up(packed, f.p, w, h, bitdepth, input_bitdepth);
  backend::dev_sync();
  download_yuv(f, out, w, h);
  f.release();
  return 0;
}
extern "C" int thor_hip_kat_depth_down(const uint16_t* in, int w, int h, int bitdepth, int input_bitdepth, void* out) {
  if (kat_depth_args(in, out, w, h, bitdepth, input_bitdepth)) return 1;
  if (!ensure_init_any()) return 3;
  const size_t bytes = (size_t)w * h * 3 / 2 * (input_bitdepth > 8 ? 2 : 1);
  DevBuf<uint8_t> packed(bytes);
  DevFrame<uint16_t> f;
  f.alloc(w, h, 0);
  upload_yuv(f, in, w, h);
  launch_depth_down(f.p, packed, w, h, bitdepth, input_bitdepth);
  backend::d2h(out, packed, bytes);
  f.release();
  return 0;
}
extern "C" int thor_hip_frame_sse_depth(const void* a, const void* b, int w, int h, int bitdepth, int input_bitdepth, unsigned long long out[3]) {
  if (bitdepth == input_bitdepth) return thor_hip_frame_sse(a, b, w, h, bitdepth, out);
  if (!out || kat_depth_args(a, b, w, h, bitdepth, input_bitdepth)) return 1;
  if (!ensure_init_any()) return 3;
  DevFrame<uint16_t> fa, fb;
  fa.alloc(w, h, 0); fb.alloc(w, h, 0);
  upload_yuv(fa, (const uint16_t*)a, w, h); upload_yuv(fb, (const uint16_t*)b, w, h);
  FrameJob<uint16_t> J;
  memset(&J, 0, sizeof(J));
  J.cfg.width = w; J.cfg.height = h; J.orig = fa.p; J.rec = fb.p;
  DevBuf<FrameJob<uint16_t>> dj(1, &J);
  DevBuf<unsigned long long> dout(4);  // zeroed
  launch_frame_sse_depth(dj, &J, 1, bitdepth, input_bitdepth, dout);
  backend::dev_sync();
  backend::d2h(out, dout, 3 * sizeof(unsigned long long));
  fa.release(); fb.release();
  return 0;
}
// The two kernels behind thor_hip_stage_frame_layout / thor_hip_get_recon_layout on host buffers.  The device copy of the layout buffer starts as far off a
// 16-byte boundary as the host buffer does, so the caller chooses between the kernels' vector and sample-by-sample paths with the pointer it passes.
static int kat_layout_args(const void* lay, const void* planar, const thor_hip_frame_layout* layout, int w, int h, int input_bitdepth, int bitdepth, PixLayout& L) {
  auto ok = [](int d) { return d == 8 || d == 10 || d == 12; };
  if (!lay || !planar || w % 8 || h % 8 || w < 16 || h < 16 || !ok(bitdepth) || !ok(input_bitdepth) || input_bitdepth > bitdepth) return 1;
  return !layout_resolved(layout, w, h, input_bitdepth, L) || (uintptr_t)lay % (input_bitdepth > 8 ? 2 : 1);
}
static const size_t kKatLayoutGuard = 64;  // bytes after the layout that travel with thor_hip_kat_layout_out's dst
template <typename PIX> static void kat_layout_in(const void* src, const PixLayout& L, int w, int h, int input_bitdepth, int bitdepth, PIX* out) {
  const size_t skew = (uintptr_t)src & 15;
  DevBuf<uint8_t> d(L.bytes + 16);
  backend::h2d(d.p + skew, src, L.bytes);
  DevFrame<PIX> f;
  f.alloc(w, h, 0);
  launch_layout_in<PIX>(d.p + skew, L, f.p, w, h, bitdepth, input_bitdepth);
  backend::dev_sync();
  download_yuv(f, out, w, h);
  f.release();
}
template <typename PIX> static void kat_layout_out(const PIX* in, const PixLayout& L, int w, int h, int input_bitdepth, int bitdepth, void* dst) {
  const size_t skew = (uintptr_t)dst & 15;
  DevBuf<uint8_t> d(L.bytes + kKatLayoutGuard + 16);
  backend::h2d(d.p + skew, dst, L.bytes + kKatLayoutGuard);
  DevFrame<PIX> f;
  f.alloc(w, h, 0);
  upload_yuv(f, in, w, h);
  launch_layout_out<PIX>(f.p, d.p + skew, L, w, h, bitdepth, input_bitdepth);
  backend::d2h(dst, d.p + skew, L.bytes + kKatLayoutGuard);
  f.release();
}
extern "C" int thor_hip_kat_layout_in(const void* src, const thor_hip_frame_layout* layout, int w, int h, int input_bitdepth, int bitdepth, void* planar_out) {
  PixLayout L;
  if (kat_layout_args(src, planar_out, layout, w, h, input_bitdepth, bitdepth, L)) return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_layout_in<uint8_t>(src, L, w, h, input_bitdepth, bitdepth, (uint8_t*)planar_out);
  else kat_layout_in<uint16_t>(src, L, w, h, input_bitdepth, bitdepth, (uint16_t*)planar_out);
  return 0;
}
extern "C" int thor_hip_kat_layout_out(const void* planar_in, const thor_hip_frame_layout* layout, int w, int h, int input_bitdepth, int bitdepth, void* dst) {
  PixLayout L;
  if (kat_layout_args(dst, planar_in, layout, w, h, input_bitdepth, bitdepth, L)) return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_layout_out<uint8_t>((const uint8_t*)planar_in, L, w, h, input_bitdepth, bitdepth, dst);
  else kat_layout_out<uint16_t>((const uint16_t*)planar_in, L, w, h, input_bitdepth, bitdepth, dst);
  return 0;
}
// k_scale_in on a host buffer, like thor_hip_kat_layout_in: `src` is a frame in `layout` (NULL = packed planar) at the source size; the device copy keeps
// the host pointer's offset from a 16-byte boundary.
template <typename PIX> static void kat_scale_in(const void* src, const ScalePlan& P, int w, int h, int input_bitdepth, int bitdepth, PIX* out) {
  const size_t skew = (uintptr_t)src & 15;
  DevBuf<uint8_t> d(P.L.bytes + 16);
  backend::h2d(d.p + skew, src, P.L.bytes);
  std::vector<uint8_t> hb(P.blob_bytes());
  DevBuf<uint8_t> tb(hb.size());
  const ScaleTables tab = P.pack(hb.data(), tb.p);
  backend::h2d(tb.p, hb.data(), hb.size());
  DevFrame<PIX> f;
  f.alloc(w, h, 0);
  launch_scale_in<PIX>(d.p + skew, P.L, tab, P.t[1].span > P.t[3].span ? P.t[1].span : P.t[3].span, f.p, P.src_w, w, h, bitdepth, input_bitdepth);
  backend::dev_sync();
  download_yuv(f, out, w, h);
  f.release();
}
extern "C" int thor_hip_kat_scale_in(const void* src, const thor_hip_scale* scale, const thor_hip_frame_layout* layout, int w, int h, int input_bitdepth, int bitdepth,
                                     void* planar_out) {
  auto ok = [](int d) { return d == 8 || d == 10 || d == 12; };
  PixLayout L;
  if (!src || !planar_out || !ok(bitdepth) || !ok(input_bitdepth) || input_bitdepth > bitdepth) return 1;
  if (!scale_args_resolved(scale, layout, w, h, input_bitdepth, L) || (uintptr_t)src % (input_bitdepth > 8 ? 2 : 1)) return 1;
  static const thor_hip_frame_layout packed = {sizeof(thor_hip_frame_layout), THOR_HIP_CHROMA_PLANAR, 0, 0, 0, 0, 0};
  const thor_hip_frame_layout* l = layout ? layout : &packed;
  ScalePlan P;
  if (!resolve_scale(scale->src_width, scale->src_height, scale->filter, scale->chroma_site, l->chroma, l->msb_aligned, l->pitch_y, l->pitch_c, l->offset_u, l->offset_v,
                     w, h, input_bitdepth, P))
    return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_scale_in<uint8_t>(src, P, w, h, input_bitdepth, bitdepth, (uint8_t*)planar_out);
  else kat_scale_in<uint16_t>(src, P, w, h, input_bitdepth, bitdepth, (uint16_t*)planar_out);
  return 0;
}
// k_rc_cost on host planes, in the engine's sequence for two consecutive frames: `prev` first, without a previous plane, then `cur` against what that wrote.
template <typename PIX> static void kat_rc_cost(const PIX* cur, const PIX* prev, int w, int h, unsigned long long out[3], PIX* half_out) {
  const int hw = w / 2, hh = h / 2;
  const size_t ny = (size_t)w * h, nh = (size_t)hw * hh;
  DevBuf<PIX> dy(ny), half0(nh), half1(nh);
  DevBuf<unsigned long long> sums(4);
  DevBuf<RcJob<PIX>> dj(1);
  RcJob<PIX> J;
  J.y = dy.p; J.sy = w; J.hw = hw; J.hh = hh; J.out = sums.p;
  if (prev) {
    backend::h2d(dy.p, prev, ny * sizeof(PIX));
    J.cur = half0.p; J.prev = nullptr;
    backend::h2d(dj.p, &J, sizeof(J));
    launch_rc_cost<PIX>(dj.p, &J, 1);
    backend::dev_sync();
    backend::dev_memset(sums.p, 0, 4 * sizeof(unsigned long long));
  }
  backend::h2d(dy.p, cur, ny * sizeof(PIX));
  J.cur = half1.p; J.prev = prev ? half0.p : nullptr;
  backend::h2d(dj.p, &J, sizeof(J));
  launch_rc_cost<PIX>(dj.p, &J, 1);
  backend::dev_sync();
  backend::d2h(out, sums.p, 3 * sizeof(unsigned long long));
  backend::d2h(half_out, half1.p, nh * sizeof(PIX));
}
extern "C" int thor_hip_kat_rc_cost(const void* cur, const void* prev_or_null, int w, int h, int bitdepth, unsigned long long out[3], void* half_out) {
  if (!cur || !out || !half_out || w % 8 || h % 8 || w < 16 || h < 16 || w > 8192 || h > 8192 || (bitdepth != 8 && bitdepth != 10 && bitdepth != 12)) return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_rc_cost<uint8_t>((const uint8_t*)cur, (const uint8_t*)prev_or_null, w, h, out, (uint8_t*)half_out);
  else kat_rc_cost<uint16_t>((const uint16_t*)cur, (const uint16_t*)prev_or_null, w, h, out, (uint16_t*)half_out);
  return 0;
}
// k_rc_cost<PIX, true> on host planes: both originals in device frames with a row pitch of a multiple of 16 samples, one launch.
template <typename PIX> static void kat_scene_cost(const PIX* cur, const PIX* prev, int w, int h, unsigned long long out[3]) {
  const int sy = (w + 15) & ~15;
  const size_t ny = (size_t)sy * h;
  DevBuf<PIX> dc(ny), dp(ny);
  DevBuf<unsigned long long> sums(4);
  DevBuf<RcJob<PIX>> dj(1);
  std::vector<PIX> tmp(ny, 0);
  auto up = [&](PIX* d, const PIX* src) {
    for (int r = 0; r < h; r++) memcpy(tmp.data() + (size_t)r * sy, src + (size_t)r * w, (size_t)w * sizeof(PIX));
    backend::h2d(d, tmp.data(), ny * sizeof(PIX));
  };
  up(dc.p, cur);
  if (prev) up(dp.p, prev);
  RcJob<PIX> J;
  J.y = dc.p; J.sy = sy; J.hw = w / 2; J.hh = h / 2; J.cur = nullptr; J.prev = nullptr; J.out = sums.p;
  J.prev_y = prev ? dp.p : nullptr; J.prev_sy = sy;
  backend::h2d(dj.p, &J, sizeof(J));
  launch_rc_cost_orig<PIX>(dj.p, &J, 1);
  backend::dev_sync();
  backend::d2h(out, sums.p, 3 * sizeof(unsigned long long));
}
extern "C" int thor_hip_kat_scene_cost(const void* cur, const void* prev_or_null, int w, int h, int bitdepth, unsigned long long out[3]) {
  if (!cur || !out || w % 8 || h % 8 || w < 16 || h < 16 || w > 8192 || h > 8192 || (bitdepth != 8 && bitdepth != 10 && bitdepth != 12)) return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_scene_cost<uint8_t>((const uint8_t*)cur, (const uint8_t*)prev_or_null, w, h, out);
  else kat_scene_cost<uint16_t>((const uint16_t*)cur, (const uint16_t*)prev_or_null, w, h, out);
  return 0;
}
// k_tf_search + k_tf_blend on host frames, as Engine::filter_frames launches them for one request: the frames in device frames laid out like staging slots.
template <typename PIX> static void kat_temporal_filter(const PIX* cur, const PIX* refs, const int* dists, int nrefs, int w, int h, int bitdepth, int strength, PIX* out,
                                                        int* mv, int* wb) {
  const size_t fsz = (size_t)w * h * 3 / 2, nb = (size_t)(w / TF_BLK) * (h / TF_BLK);
  DevFrame<PIX> fc, fo, fr[TF_MAX_REFS];
  fc.alloc(w, h, 0); fo.alloc(w, h, 0);
  upload_yuv(fc, cur, w, h);
  for (int k = 0; k < nrefs; k++) { fr[k].alloc(w, h, 0); upload_yuv(fr[k], refs + (size_t)k * fsz, w, h); }
  DevBuf<TfBlock> blk(nb * TF_MAX_REFS);
  DevBuf<TfJob<PIX>> dj(1);
  TfJob<PIX> J;
  J.cur = fc.p; J.dst = fo.p;
  for (int k = 0; k < TF_MAX_REFS; k++) { J.ref[k] = k < nrefs ? fr[k].p : fc.p; J.dist[k] = k < nrefs ? dists[k] : 1; }
  J.nrefs = nrefs; J.width = w; J.height = h; J.strength = strength; J.sh = bitdepth - 8; J.blk = blk.p;
  backend::h2d(dj.p, &J, sizeof(J));
  launch_tf<PIX>(dj.p, &J, 1);
  backend::dev_sync();
  download_yuv(fo, out, w, h);
  std::vector<TfBlock> hb(nb * TF_MAX_REFS);
  backend::d2h(hb.data(), blk.p, hb.size() * sizeof(TfBlock));
  for (size_t i = 0; i < nb * nrefs; i++) { mv[2 * i] = hb[i].dx; mv[2 * i + 1] = hb[i].dy; wb[i] = hb[i].wb; }
  fc.release(); fo.release();
  for (int k = 0; k < nrefs; k++) fr[k].release();
}
extern "C" int thor_hip_kat_temporal_filter(const void* cur, const void* refs, const int* dists, int nrefs, int w, int h, int bitdepth, int strength, void* out, int* mv,
                                            int* wb) {
  if (!cur || !out || !mv || !wb || nrefs < 0 || nrefs > TF_MAX_REFS || (nrefs && (!refs || !dists)) || !tf_strength_ok(strength)) return 1;
  if (w % 8 || h % 8 || w < 16 || h < 16 || w > 8192 || h > 8192 || (bitdepth != 8 && bitdepth != 10 && bitdepth != 12)) return 1;
  for (int k = 0; k < nrefs; k++)
    if (dists[k] != 1 && dists[k] != 2) return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_temporal_filter<uint8_t>((const uint8_t*)cur, (const uint8_t*)refs, dists, nrefs, w, h, bitdepth, strength, (uint8_t*)out, mv, wb);
  else kat_temporal_filter<uint16_t>((const uint16_t*)cur, (const uint16_t*)refs, dists, nrefs, w, h, bitdepth, strength, (uint16_t*)out, mv, wb);
  return 0;
}
// k_rgb_in / k_rgb_out on host buffers, like the two above: the device copy keeps the host pointer's offset from a 16-byte boundary.
static int kat_rgb_args(const void* rgb, const void* planar, const thor_hip_rgb_format* fmt, int w, int h, int input_bitdepth, int bitdepth, RgbFormat& R) {
  auto ok = [](int d) { return d == 8 || d == 10 || d == 12; };
  if (!rgb || !planar || w % 8 || h % 8 || w < 16 || h < 16 || !ok(bitdepth) || !ok(input_bitdepth) || input_bitdepth > bitdepth) return 1;
  return !rgb_resolved(fmt, w, h, input_bitdepth, R) || (uintptr_t)rgb % R.sbytes;
}
template <typename PIX> static void kat_rgb_in(const void* src, const RgbFormat& R, int w, int h, int input_bitdepth, int bitdepth, PIX* out) {
  const size_t skew = (uintptr_t)src & 15;
  DevBuf<uint8_t> d(R.bytes + 16);
  backend::h2d(d.p + skew, src, R.bytes);
  DevFrame<PIX> f;
  f.alloc(w, h, 0);
  launch_rgb_in<PIX>(d.p + skew, R, f.p, w, h, bitdepth, input_bitdepth);
  backend::dev_sync();
  download_yuv(f, out, w, h);
  f.release();
}
template <typename PIX> static void kat_rgb_out(const PIX* in, const RgbFormat& R, int w, int h, int input_bitdepth, int bitdepth, void* dst) {
  const size_t skew = (uintptr_t)dst & 15;
  DevBuf<uint8_t> d(R.bytes + kKatLayoutGuard + 16);
  backend::h2d(d.p + skew, dst, R.bytes + kKatLayoutGuard);
  DevFrame<PIX> f;
  f.alloc(w, h, 0);
  upload_yuv(f, in, w, h);
  launch_rgb_out<PIX>(f.p, d.p + skew, R, w, h, bitdepth, input_bitdepth);
  backend::d2h(dst, d.p + skew, R.bytes + kKatLayoutGuard);
  f.release();
}
extern "C" int thor_hip_kat_rgb_in(const void* src, const thor_hip_rgb_format* fmt, int w, int h, int input_bitdepth, int bitdepth, void* planar_out) {
  RgbFormat R;
  if (kat_rgb_args(src, planar_out, fmt, w, h, input_bitdepth, bitdepth, R)) return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_rgb_in<uint8_t>(src, R, w, h, input_bitdepth, bitdepth, (uint8_t*)planar_out);
  else kat_rgb_in<uint16_t>(src, R, w, h, input_bitdepth, bitdepth, (uint16_t*)planar_out);
  return 0;
}
extern "C" int thor_hip_kat_rgb_out(const void* planar_in, const thor_hip_rgb_format* fmt, int w, int h, int input_bitdepth, int bitdepth, void* dst) {
  RgbFormat R;
  if (kat_rgb_args(dst, planar_in, fmt, w, h, input_bitdepth, bitdepth, R)) return 1;
  if (!ensure_init_any()) return 3;
  if (bitdepth == 8) kat_rgb_out<uint8_t>((const uint8_t*)planar_in, R, w, h, input_bitdepth, bitdepth, dst);
  else kat_rgb_out<uint16_t>((const uint16_t*)planar_in, R, w, h, input_bitdepth, bitdepth, dst);
  return 0;
}
extern "C" int thor_hip_kat_interpolate(const void* yuv0, const void* yuv1, int width, int height, int bitdepth, void* out_yuv) {
  KAT_BD(kat_interpolate<uint8_t>((const uint8_t*)yuv0, (const uint8_t*)yuv1, width, height, 8, (uint8_t*)out_yuv),
         kat_interpolate<uint16_t>((const uint16_t*)yuv0, (const uint16_t*)yuv1, width, height, bitdepth, (uint16_t*)out_yuv));
}
// The same path for n_streams reference pairs in one make_interp_frames call, with every stage copied back (tk_kat_interp.h; tests/golden/gen_kat12.py)
extern "C" int thor_hip_kat_interp_stages(int n_streams, const void* yuv0, const void* yuv1, int width, int height, int bitdepth, int levels, void* pyramid,
                                          int16_t* nmv, void* out_padded) {
  if (bitdepth < 8 || bitdepth > 12) return 1;
  if (!ensure_init_any()) return 3;
  KAT_BD(kat_interp_stages<uint8_t>(n_streams, (const uint8_t*)yuv0, (const uint8_t*)yuv1, width, height, 8, levels, (uint8_t*)pyramid, nmv, (uint8_t*)out_padded),
         kat_interp_stages<uint16_t>(n_streams, (const uint16_t*)yuv0, (const uint16_t*)yuv1, width, height, bitdepth, levels, (uint16_t*)pyramid, nmv, (uint16_t*)out_padded));
}

// Resources of the superblock kernel as the runtime sees them (a guard against silent occupancy regressions: round 6 found the 8-bit kernel at 227 VGPRs =
// two workgroups per CU after an unrelated kernel had raised the register budget of a shared __noinline__ function).
extern "C" int thor_hip_superblock_kernel_info(int sample_bytes, int* num_regs, int* lds_bytes, int* private_bytes, int* workgroups_per_cu) {
  if (!ensure_init_any()) return 3;
  hipFuncAttributes a;
  int per_cu = 0;
  if (sample_bytes == 1) {
    HIPCHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_superblocks<uint8_t>)));
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_superblocks<uint8_t>, kWgThreads, 0));
  } else if (sample_bytes == 2) {
    HIPCHECK(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_superblocks<uint16_t>)));
    HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_superblocks<uint16_t>, kWgThreads, 0));
  } else if (sample_bytes == 0) {   // the latency build of the 8-bit kernel (thor_hip_lat.cpp)
    if (thor_lat_kernel_info(num_regs, lds_bytes, private_bytes)) return 2;
    if (workgroups_per_cu) *workgroups_per_cu = thor_lat_workgroups_per_cu();
    return 0;
  } else if (sample_bytes == 3) {   // the eight-wavefront build of the 8-bit kernel (thor_hip_wide.cpp)
    if (thor_wide_kernel_info(num_regs, lds_bytes, private_bytes)) return 2;
    if (workgroups_per_cu) *workgroups_per_cu = thor_wide_workgroups_per_cu();
    return 0;
  } else return 1;
  if (num_regs) *num_regs = a.numRegs;
  if (lds_bytes) *lds_bytes = (int)a.sharedSizeBytes;
  if (private_bytes) *private_bytes = (int)a.localSizeBytes;
  if (workgroups_per_cu) *workgroups_per_cu = per_cu;
  return 0;
}
// Which build of the 8-bit superblock kernel the engine configured last launches with: 0 throughput (thor_hip.cpp), 1 latency (thor_hip_lat.cpp), 2 eight
// wavefronts per workgroup (thor_hip_wide.cpp).  Decided at the engine's first launch from the number of streams and the geometry (run_superblocks).
extern "C" int thor_hip_superblock_kernel_in_use(void) { return tk::backend::g_last_kern; }
