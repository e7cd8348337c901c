// hip_kat_block.h - known-answer entry points of the layer between the sample kernels and the stream: the neighbour context of a coding block (tk_block_ctx.h:
// upright_avail, downleft_avail, get_mv_pred, get_mv_cands, find_contexts) the block cost (tk_block_rd.h: ssd_part, ssd_total, rd_cost) and the intra SAD search / build_org8 (tk_block_search.h) against the
// reference's own answers (tests/golden/gen_kat11.py -> kat11.npz, tests/test_gpu_kat.py).  Part of thor_hip.cpp (included after hip_kat.h): the kernels call the
// very device functions k_superblocks calls.
#pragma once
#include "tk_kat_block.h"
namespace tk {
// one wavefront per item; the context functions are wave-uniform inline code in the product too (every lane computes them, lane 0 keeps the result)
__global__ __launch_bounds__(64) void k_kat_block_ctx(const DbCell* cells, int cs, const int* par, int* out) {
  const int it = (int)blockIdx.x;
  int o[kKatCtxOut];
  kat_ctx_item(cells, cs, par + kKatCtxPar * it, o);
  if (threadIdx.x == 0)
    for (int k = 0; k < kKatCtxOut; k++) out[(size_t)kKatCtxOut * it + k] = o[k];
}
// rd_cost is a __noinline__ function the superblock kernel calls too, so this kernel carries its launch bounds (see k_kat_inter_yuv in hip_kat.h).  The workspace
// is built as k_kat_early_skip builds it and the blocks lie where the product has them: the original in the workgroup's LDS copy (stride = block size) with the
// trial reconstruction in the wave's LDS sample buffers for blocks up to kLdsBlk (org_select / ws_select: the SP_LDS instances), above that the original in a
// plane in global memory with the item's skew and stride and the reconstruction in a compact global block (the SP_GLOBAL instances).  The luma SSD alone also
// runs the SP_GLOBAL instance on the skewed plane for every size.
// lay[3 * i ..]: first sample of the item's Y, U, V rows in `orgp`
template <typename PIX>
__global__ __launch_bounds__(kWgThreads, (sizeof(PIX) == 1 ? (int)kOcc : 2)) void k_kat_block_cost(const int* par, const double* lam, const int* lay, const PIX* orgp, const PIX* recp,
                                                                                                   int bitdepth, unsigned char* big, unsigned long long* out) {
  __shared__ FrameJob<PIX> sJ;
  __shared__ WgShared sh;
  __shared__ SmallWs<PIX> sws;
  __shared__ TeamWs<PIX> s_view;
  const int lane = (int)threadIdx.x, it = (int)blockIdx.x;
  const Team t = mk_team(lane, 64, sh.tabs.izz);
  const int* q = par + kKatCostPar * it;
  const int size = __builtin_amdgcn_readfirstlane(q[0]), bw = __builtin_amdgcn_readfirstlane(q[1]), bh = __builtin_amdgcn_readfirstlane(q[2]);
  const int nbits = __builtin_amdgcn_readfirstlane(q[3]), off = __builtin_amdgcn_readfirstlane(q[4]), sy = __builtin_amdgcn_readfirstlane(q[6]);
  const int n = size * size, c = n >> 2, sc = size >> 1;
  const PIX* gy = orgp + lay[3 * it];
  const PIX* gu = orgp + lay[3 * it + 1];
  const PIX* gv = orgp + lay[3 * it + 2];
  const PIX* ry = recp + off;
  const int lds_blk = size <= kLdsBlk;
  TeamWs<PIX> w = make_ws(&sws, &sh, (BigWs<PIX>*)big);
  ws_select(&w, size);
  if (lds_blk) {
    PIX* ob = (PIX*)sh.org_raw;
    for (int k = lane; k < bw * bh; k += 64) ob[(k / bw) * size + k % bw] = gy[(k / bw) * sy + k % bw];
    for (int k = lane; k < (bw >> 1) * (bh >> 1); k += 64) {
      const int i = k / (bw >> 1), j = k % (bw >> 1);
      ob[n + i * sc + j] = gu[i * (sy >> 1) + j];
      ob[n + c + i * sc + j] = gv[i * (sy >> 1) + j];
    }
    for (int k = lane; k < n; k += 64) w.rec_y[k] = ry[k];
    for (int k = lane; k < c; k += 64) { w.rec_u[k] = ry[n + k]; w.rec_v[k] = ry[n + c + k]; }
    w.org_y = ob; w.org_u = ob + n; w.org_v = ob + n + c; w.org_sy = size; w.org_sc = sc;
  } else {
    w.rec_y = const_cast<PIX*>(ry); w.rec_u = const_cast<PIX*>(ry) + n; w.rec_v = const_cast<PIX*>(ry) + n + c;   // read only
    w.org_y = gy; w.org_u = gu; w.org_v = gv; w.org_sy = sy; w.org_sc = sy >> 1;
  }
  lds_st(&s_view, w);
  if (lane == 0) {
    sJ.cfg.bitdepth = bitdepth;
    sh.stack[0].size = size; sh.stack[0].bw = bw; sh.stack[0].bh = bh;
  }
  __syncthreads();
  WsP<PIX> ws = ldsc(&s_view);
  JobR<PIX> J = *ldsc(&sJ);
  const double lambda = lam[it];
  const unsigned long long ssd_g = ssd_total(t, ssd_part<SP_GLOBAL>(t, gy, sy, ry, size, bw, bh));
  unsigned long long ssd_l = ~0ull, cost, cost_y;
  if (lds_blk) {
    ssd_l = ssd_total(t, ssd_part<SP_LDS>(t, w.org_y, size, w.rec_y, size, bw, bh));
    cost = rd_cost<PIX, SP_LDS>(t, J, ws, sh.stack[0], nbits, lambda);
    cost_y = rd_cost<PIX, SP_LDS>(t, J, ws, sh.stack[0], nbits, lambda, (long long)ssd_l);
  } else {
    cost = rd_cost<PIX, SP_GLOBAL>(t, J, ws, sh.stack[0], nbits, lambda);
    cost_y = rd_cost<PIX, SP_GLOBAL>(t, J, ws, sh.stack[0], nbits, lambda, (long long)ssd_g);
  }
  if (lane == 0) {
    unsigned long long* o = out + (size_t)kKatCostOut * it;
    o[0] = ssd_g; o[1] = ssd_l; o[2] = cost; o[3] = cost_y;
  }
}
// intra_sad_search (tk_block_search.h) is a __noinline__ function of the superblock kernel too: its launch bounds.  The job holds what the search reads: the
// frame size, bit depth and superblock size, and the reconstructed plane; the original lies where org_select has it - the workgroup's LDS copy up to kLdsBlk (the
// SP_LDS instance, prediction in the wave's LDS sample buffers), a compact block in global memory above (SP_GLOBAL, prediction in the item's own BigWs `slot`).
template <typename PIX>
__global__ __launch_bounds__(kWgThreads, (sizeof(PIX) == 1 ? (int)kOcc : 2)) void k_kat_intra_search(const int* par, const int* slot, const PIX* plane, int fw, int fh, int bitdepth,
                                                                                                     const PIX* orgp, unsigned char* big, int* out) {
  __shared__ FrameJob<PIX> sJ;
  __shared__ WgShared sh;
  __shared__ SmallWs<PIX> sws;
  __shared__ TeamWs<PIX> s_view;
  const int lane = (int)threadIdx.x, it = (int)blockIdx.x;
  const Team t = mk_team(lane, 64, sh.tabs.izz);
  const int* q = par + kKatIntraPar * it;
  const int ypos = __builtin_amdgcn_readfirstlane(q[0]), xpos = __builtin_amdgcn_readfirstlane(q[1]), size = __builtin_amdgcn_readfirstlane(q[2]);
  const int sb = __builtin_amdgcn_readfirstlane(q[3]), nm = __builtin_amdgcn_readfirstlane(q[4]), off = __builtin_amdgcn_readfirstlane(q[5]);
  const PIX* go = orgp + off;
  const int lds_blk = size <= kLdsBlk;
  TeamWs<PIX> w = make_ws(&sws, &sh, (BigWs<PIX>*)big + __builtin_amdgcn_readfirstlane(slot[it]));
  ws_select(&w, size);
  if (lds_blk) {
    PIX* ob = (PIX*)sh.org_raw;
    for (int k = lane; k < size * size; k += 64) ob[k] = go[k];
    w.org_y = ob;
  } else {
    w.org_y = go;
  }
  w.org_sy = size;
  lds_st(&s_view, w);
  if (lane == 0) {
    sJ.cfg.width = fw; sJ.cfg.height = fh; sJ.cfg.bitdepth = bitdepth; sJ.cfg.sb_shift = sb == kMaxSb ? 0 : 1;
    sJ.rec.y = const_cast<PIX*>(plane); sJ.rec.sy = fw;   // read only
    sh.stack[0].size = size; sh.stack[0].ypos = ypos; sh.stack[0].xpos = xpos; sh.stack[0].bw = size; sh.stack[0].bh = size;
  }
  __syncthreads();
  WsP<PIX> ws = ldsc(&s_view);
  JobR<PIX> J = *ldsc(&sJ);
  int mode = -1;
  const unsigned sad = lds_blk ? intra_sad_search<PIX, SP_LDS>(t, J, ws, sh.stack[0], nm, &mode) : intra_sad_search<PIX, SP_GLOBAL>(t, J, ws, sh.stack[0], nm, &mode);
  if (lane == 0) { out[kKatIntraOut * it] = mode; out[kKatIntraOut * it + 1] = (int)sad; }
}
// build_org8 (tk_block_search.h) as search_bipred calls it.  outg: the SP_GLOBAL instance on the original plane with the item's skew and stride (lay[i]: its
// first sample in `orgp`), prediction and result compact blocks in global memory.  outl: blocks up to kLdsBlk also run the SP_LDS instance - original in the
// workgroup's LDS copy, prediction and result in the wave's LDS sample buffers (ws_select) - and the result is copied out; larger blocks leave outl as it was.
template <typename PIX>
__global__ __launch_bounds__(64) void k_kat_build_org8(const int* par, const int* lay, const PIX* orgp, const PIX* predp, int bitdepth, unsigned char* big, PIX* outg, PIX* outl) {
  __shared__ WgShared sh;
  __shared__ SmallWs<PIX> sws;
  const int lane = (int)threadIdx.x, it = (int)blockIdx.x;
  const Team t = mk_team(lane, 64, sh.tabs.izz);
  const int* q = par + kKatOrg8Par * it;
  const int size = __builtin_amdgcn_readfirstlane(q[0]), off = __builtin_amdgcn_readfirstlane(q[1]), sy = __builtin_amdgcn_readfirstlane(q[3]);
  const int n = size * size;
  const PIX* gy = orgp + lay[it];
  const PIX* gp = predp + off;
  build_org8<PIX, SP_GLOBAL>(t, outg + off, gy, sy, gp, size, bitdepth);
  if (size <= kLdsBlk) {
    TeamWs<PIX> w = make_ws(&sws, &sh, (BigWs<PIX>*)big);
    ws_select(&w, size);
    PIX* ob = (PIX*)sh.org_raw;
    for (int k = lane; k < n; k += 64) { ob[k] = gy[(k / size) * sy + k % size]; w.pred_y[k] = gp[k]; }
    __syncthreads();
    build_org8<PIX, SP_LDS>(t, w.org8, ob, size, w.pred_y, size, bitdepth);
    __syncthreads();
    for (int k = lane; k < n; k += 64) outl[off + k] = w.org8[k];
  }
}
}  // namespace tk

namespace {
template <typename PIX>
int kat_intra_search(int n, const int* par, const PIX* plane, int fw, int fh, const PIX* org, long long nsamp, int bitdepth, int* out) {
  if (n <= 0 || n > 4096 || !par || !plane || !org || !out || fw < 8 || fh < 8 || fw > 4096 || fh > 4096 || fw % 8 || fh % 8 || nsamp <= 0 || nsamp > (1ll << 30)) return 1;
  std::vector<int> slot(n, 0);
  int nbig = 0;
  for (int i = 0; i < n; i++) {
    if (int r = kat_intra_check(par + kKatIntraPar * i, fw, fh, nsamp)) return r;
    if (par[kKatIntraPar * i + 2] > kLdsBlk) slot[i] = nbig++;   // a prediction buffer in global memory of the item's own
  }
  if (!ensure_init_any()) return 3;
  DevBuf<int> d_par((size_t)kKatIntraPar * n, par), d_slot(n, slot.data()), d_o((size_t)kKatIntraOut * n);
  DevBuf<PIX> d_plane((size_t)fw * fh, plane), d_org((size_t)nsamp, org);
  DevBuf<unsigned char> d_big(sizeof(BigWs<PIX>) * (size_t)(nbig > 0 ? nbig : 1));
  hipLaunchKernelGGL(k_kat_intra_search<PIX>, dim3(n), dim3(64), 0, g_stream, d_par, d_slot, d_plane, fw, fh, bitdepth, d_org, d_big, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)kKatIntraOut * n * 4);
  return 0;
}
template <typename PIX>
int kat_build_org8(int n, const int* par, const PIX* org, const PIX* pred, long long nsamp, int bitdepth, PIX* outg, PIX* outl) {
  const int S = (int)sizeof(PIX);
  if (n <= 0 || !par || !org || !pred || !outg || !outl || nsamp <= 0 || nsamp > (1ll << 28)) return 1;
  for (int i = 0; i < n; i++)
    if (int r = kat_org8_check(par + kKatOrg8Par * i, nsamp, S)) return r;
  std::vector<PIX> planes;   // the originals as planes with the item's skew and stride, as kat_block_cost lays them out
  std::vector<int> lay(n);
  for (int i = 0; i < n; i++) {
    const int* q = par + kKatOrg8Par * i;
    const int size = q[0], sk = q[2] / S, st = q[3];
    const size_t base = (planes.size() * S + 15) / 16 * 16 / S;
    planes.resize(base + sk + (size_t)(size - 1) * st + size, (PIX)0);
    lay[i] = (int)(base + sk);
    for (int r = 0; r < size; r++) memcpy(&planes[base + sk + (size_t)r * st], org + q[1] + (size_t)r * size, (size_t)size * S);
  }
  if (planes.size() > (1u << 30)) return 2;
  if (!ensure_init_any()) return 3;
  DevBuf<int> d_par((size_t)kKatOrg8Par * n, par), d_lay(n, lay.data());
  DevBuf<PIX> d_org(planes.size(), planes.data()), d_pred((size_t)nsamp, pred), d_g((size_t)nsamp, outg), d_l((size_t)nsamp, outl);
  DevBuf<unsigned char> d_big(sizeof(BigWs<PIX>));   // make_ws points at it; blocks that run the LDS instance do not touch it
  hipLaunchKernelGGL(k_kat_build_org8<PIX>, dim3(n), dim3(64), 0, g_stream, d_par, d_lay, d_org, d_pred, bitdepth, d_big, d_g, d_l);
  HIPCHECK(hipGetLastError());
  backend::d2h(outg, d_g, (size_t)nsamp * S);
  backend::d2h(outl, d_l, (size_t)nsamp * S);
  return 0;
}
template <typename PIX>
int kat_block_cost(int n, const int* par, const double* lambda, const PIX* org, const PIX* rec, long long nsamp, int bitdepth, unsigned long long* out) {
  const int S = (int)sizeof(PIX);
  if (n <= 0 || !par || !lambda || !org || !rec || !out || nsamp <= 0 || nsamp > (1ll << 30)) return 1;
  for (int i = 0; i < n; i++)
    if (int r = kat_cost_check(par + kKatCostPar * i, lambda[i], nsamp, S)) return r;
  // the originals as planes with the item's skew and stride: every plane starts `skew` bytes after a 16-byte boundary
  std::vector<PIX> planes;
  std::vector<int> lay((size_t)3 * n);
  for (int i = 0; i < n; i++) {
    const int* q = par + kKatCostPar * i;
    const int size = q[0], bw = q[1], bh = q[2], skew = q[5], sy = q[6];
    const PIX* src = org + q[4];
    for (int pl = 0; pl < 3; pl++) {
      const int w = pl ? bw / 2 : bw, h = pl ? bh / 2 : bh, st = pl ? sy / 2 : sy, cst = pl ? size / 2 : size;
      const int sk = (pl ? skew / 2 : skew) / S;
      const PIX* s = src + (pl == 0 ? 0 : pl == 1 ? size * size : size * size * 5 / 4);
      const size_t base = (planes.size() * S + 15) / 16 * 16 / S;
      planes.resize(base + sk + (size_t)(h - 1) * st + w, (PIX)0);
      lay[3 * i + pl] = (int)(base + sk);
      for (int r = 0; r < h; r++) memcpy(&planes[base + sk + (size_t)r * st], s + (size_t)r * cst, (size_t)w * S);
    }
  }
  if (planes.size() > (1u << 30)) return 2;
  if (!ensure_init_any()) return 3;
  DevBuf<int> d_par((size_t)kKatCostPar * n, par), d_lay((size_t)3 * n, lay.data());
  DevBuf<double> d_lam(n, lambda);
  DevBuf<PIX> d_org(planes.size(), planes.data()), d_rec((size_t)nsamp, rec);
  DevBuf<unsigned char> d_big(sizeof(BigWs<PIX>));   // the per-wave global scratch make_ws points at; the cost does not touch it
  DevBuf<unsigned long long> d_o((size_t)kKatCostOut * n);
  hipLaunchKernelGGL(k_kat_block_cost<PIX>, dim3(n), dim3(64), 0, g_stream, d_par, d_lam, d_lay, d_org, d_rec, bitdepth, d_big, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)kKatCostOut * n * 8);
  return 0;
}
}  // namespace

extern "C" int thor_hip_kat_block_ctx(const thor_hip_cell* cells, long long ncells, int cell_stride, int n, const int* par, int* out) {
  static_assert(sizeof(thor_hip_cell) == sizeof(DbCell), "thor_hip_cell must mirror tk::DbCell");
  if (!cells || !par || !out || n <= 0 || ncells <= 0 || ncells > (1ll << 26) || cell_stride < 2 || cell_stride > 2048) return 1;
  for (int i = 0; i < n; i++) {
    if (par[kKatCtxPar * i + 3] != 4 * cell_stride) return 1;
    if (int r = kat_ctx_check(par + kKatCtxPar * i, ncells)) return r;
  }
  if (!ensure_init_any()) return 3;
  // one row and one column of zero cells in front of the grid: the indices bi - cs - 1 .. bi - 1 of blocks in the first row / column stay inside the buffer
  const size_t pad = (size_t)cell_stride + 1;
  DevBuf<DbCell> d_cells(pad + (size_t)ncells);
  backend::h2d(d_cells.get() + pad, cells, (size_t)ncells * sizeof(DbCell));
  DevBuf<int> d_par((size_t)kKatCtxPar * n, par), d_o((size_t)kKatCtxOut * n);
  hipLaunchKernelGGL(k_kat_block_ctx, dim3(n), dim3(64), 0, g_stream, d_cells.get() + pad, cell_stride, d_par, d_o);
  HIPCHECK(hipGetLastError());
  backend::d2h(out, d_o, (size_t)kKatCtxOut * n * 4);
  return 0;
}
extern "C" int thor_hip_kat_lds_block(void) { return kLdsBlk; }
extern "C" int thor_hip_kat_block_cost(int n, const int* par, const double* lambda, const void* org, const void* rec, long long nsamp, int bitdepth, unsigned long long* out) {
  KAT_BD(kat_block_cost<uint8_t>(n, par, lambda, (const uint8_t*)org, (const uint8_t*)rec, nsamp, 8, out),
         kat_block_cost<uint16_t>(n, par, lambda, (const uint16_t*)org, (const uint16_t*)rec, nsamp, bitdepth, out));
}
extern "C" int thor_hip_kat_intra_search(int n, const int* par, const void* plane, int width, int height, const void* org, long long nsamp, int bitdepth, int* out) {
  KAT_BD(kat_intra_search<uint8_t>(n, par, (const uint8_t*)plane, width, height, (const uint8_t*)org, nsamp, 8, out),
         kat_intra_search<uint16_t>(n, par, (const uint16_t*)plane, width, height, (const uint16_t*)org, nsamp, bitdepth, out));
}
extern "C" int thor_hip_kat_build_org8(int n, const int* par, const void* org, const void* pred, long long nsamp, int bitdepth, void* out_global, void* out_lds) {
  KAT_BD(kat_build_org8<uint8_t>(n, par, (const uint8_t*)org, (const uint8_t*)pred, nsamp, 8, (uint8_t*)out_global, (uint8_t*)out_lds),
         kat_build_org8<uint16_t>(n, par, (const uint16_t*)org, (const uint16_t*)pred, nsamp, bitdepth, (uint16_t*)out_global, (uint16_t*)out_lds));
}
