// kat_host_ctx.cpp - TEST INFRASTRUCTURE ONLY.  The host build of the block decision's neighbour context (thor_amd/csrc/tk_block_ctx.h: upright_avail,
// downleft_avail, get_mv_pred, get_mv_cands, find_contexts) and of its cost (tk_block_rd.h: ssd_part, ssd_total, rd_cost) behind two batch calls with the
// arguments of thor_hip_kat_block_ctx / thor_hip_kat_block_cost (include/thor_hip.h), so that tests/golden/kat11.npz (recorded from the reference,
// tests/golden/gen_kat11.py) pins them on the CPU (tests/test_kat_host.py) - the CPU twin of the device tests in tests/test_gpu_kat.py.
// Also intra_sad_search and build_org8 (tk_block_search.h) behind h_intra_search / h_build_org8, the twins of thor_hip_kat_intra_search / thor_hip_kat_build_org8.
// Plain build: 1-lane teams.  -DTHOR_HOSTSIM_LANES=64 -pthread: the cost with teams of `lanes` OS threads (team_sum / team_sum64 across lanes).
#include "../../thor_amd/csrc/tk_block.h"
#include "../../thor_amd/csrc/tk_tables.h"
#include "../../thor_amd/csrc/tk_kat_block.h"
#include <cstdlib>
#include <cstring>
#include <vector>
#ifdef THOR_HOSTSIM_LANES
#include <atomic>
#include <thread>
#endif
namespace tk {
Tables g_tab;
long long g_prune_stat[8];
#ifdef THOR_HOSTSIM_LANES
namespace hostlanes {   // every lane is an OS thread; one exchange primitive (publish a value, read everybody's), as in tests/hostsim/kat_host_bits.cpp
struct Shared { int n = 1; std::atomic<int> count{0}; std::atomic<int> sense{0}; unsigned long long slots[64]; };
static thread_local Shared* tl_sh = nullptr;
static thread_local int tl_rank = 0, tl_sense = 0;
int lanes() { return tl_sh ? tl_sh->n : 1; }
int rank() { return tl_rank; }
void barrier() {
  Shared* sh = tl_sh;
  if (!sh || sh->n == 1) return;
  const int my = tl_sense ^= 1;
  if (sh->count.fetch_add(1, std::memory_order_acq_rel) == sh->n - 1) { sh->count.store(0, std::memory_order_relaxed); sh->sense.store(my, std::memory_order_release); }
  else { int spins = 0; while (sh->sense.load(std::memory_order_acquire) != my) if (++spins > 200) { std::this_thread::yield(); spins = 0; } }
}
static thread_local unsigned long long tl_single[1];
const unsigned long long* exchange_begin(unsigned long long v) {
  Shared* sh = tl_sh;
  if (!sh || sh->n == 1) { tl_single[0] = v; return tl_single; }
  sh->slots[tl_rank] = v;
  barrier();
  return sh->slots;
}
void exchange_end() { barrier(); }
}  // namespace hostlanes
#endif
}  // namespace tk
using namespace tk;

// fn(rank): run by every lane of a team of `lanes`
template <class F> static int run_team(int lanes, F fn) {
#ifdef THOR_HOSTSIM_LANES
  if (lanes < 1 || lanes > 64) return 1;
  hostlanes::Shared sh;
  sh.n = lanes;
  std::vector<std::thread> th;
  for (int r = 0; r < lanes; r++)
    th.emplace_back([&, r]() {
      hostlanes::tl_sh = &sh; hostlanes::tl_rank = r; hostlanes::tl_sense = 0;
      fn(r);
    });
  for (auto& x : th) x.join();
#else
  if (lanes != 1) return 1;
  fn(0);
#endif
  return 0;
}

extern "C" int h_block_ctx(const DbCell* cells, long long ncells, int cell_stride, int n, const int* par, int* out) {
  if (!cells || !par || !out || n <= 0 || ncells <= 0 || cell_stride < 2) return 1;
  for (int i = 0; i < n; i++) {
    if (par[kKatCtxPar * i + 3] != 4 * cell_stride) return 1;
    if (int r = kat_ctx_check(par + kKatCtxPar * i, ncells)) return r;
  }
  const size_t pad = (size_t)cell_stride + 1;   // one row and one column of zero cells in front of the grid, as the device entry point has them
  std::vector<DbCell> g(pad + (size_t)ncells);
  memset(g.data(), 0, pad * sizeof(DbCell));
  memcpy(g.data() + pad, cells, (size_t)ncells * sizeof(DbCell));
  for (int i = 0; i < n; i++) kat_ctx_item(g.data() + pad, cell_stride, par + kKatCtxPar * i, out + kKatCtxOut * i);
  return 0;
}

template <typename PIX>
static int block_cost(int lanes, int n, const int* par, const double* lambda, const PIX* org, const PIX* rec, long long nsamp, int bitdepth, unsigned long long* out) {
  const int S = (int)sizeof(PIX);
  if (n <= 0 || !par || !lambda || !org || !rec || !out) return 1;
  for (int i = 0; i < n; i++)
    if (int r = kat_cost_check(par + kKatCostPar * i, lambda[i], nsamp, S)) return r;
  // the originals as planes with the item's skew and stride (every plane starts `skew` bytes after a 16-byte boundary), the reconstructions compact and aligned
  std::vector<size_t> lay((size_t)3 * n);
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    const int* q = par + kKatCostPar * i;
    for (int pl = 0; pl < 3; pl++) {
      const int w = pl ? q[1] / 2 : q[1], h = pl ? q[2] / 2 : q[2], st = pl ? q[6] / 2 : q[6], sk = (pl ? q[5] / 2 : q[5]) / S;
      const size_t base = (total * S + 15) / 16 * 16 / S;
      lay[3 * i + pl] = base + sk;
      total = base + sk + (size_t)(h - 1) * st + w;
    }
  }
  PIX* planes = (PIX*)aligned_alloc(64, (total * S + 63) / 64 * 64);
  PIX* recs = (PIX*)aligned_alloc(64, ((size_t)nsamp * S + 63) / 64 * 64);
  PIX* ldsb = (PIX*)aligned_alloc(64, (size_t)kLdsBlk * kLdsBlk * 3 * S);
  if (!planes || !recs || !ldsb) return 3;
  memset(planes, 0, total * S);
  memcpy(recs, rec, (size_t)nsamp * S);
  for (int i = 0; i < n; i++) {
    const int* q = par + kKatCostPar * i;
    const int size = q[0];
    for (int pl = 0; pl < 3; pl++) {
      const int w = pl ? q[1] / 2 : q[1], h = pl ? q[2] / 2 : q[2], st = pl ? q[6] / 2 : q[6], cst = pl ? size / 2 : size;
      const PIX* s = org + q[4] + (pl == 0 ? 0 : pl == 1 ? size * size : size * size * 5 / 4);
      for (int r = 0; r < h; r++) memcpy(planes + lay[3 * i + pl] + (size_t)r * st, s + (size_t)r * cst, (size_t)w * S);
    }
  }
  static FrameJob<PIX> J;
  J.cfg.bitdepth = bitdepth;
  const int rc = run_team(lanes, [&](int r) {
    const Team t = mk_team(r, lanes);
    for (int i = 0; i < n; i++) {
      const int* q = par + kKatCostPar * i;
      const int size = q[0], bw = q[1], bh = q[2], nbits = q[3], sy = q[6], nn = size * size, c = nn / 4;
      const PIX* gy = planes + lay[3 * i];
      const PIX* gu = planes + lay[3 * i + 1];
      const PIX* gv = planes + lay[3 * i + 2];
      PIX* ry = recs + q[4];
      const int lds_blk = size <= kLdsBlk;
      t.sync();
      if (lds_blk && r == 0) {   // the compact copy the engine keeps in LDS (org_select)
        for (int y = 0; y < bh; y++) memcpy(ldsb + y * size, gy + (size_t)y * sy, (size_t)bw * S);
        for (int y = 0; y < bh / 2; y++) {
          memcpy(ldsb + nn + y * (size / 2), gu + (size_t)y * (sy / 2), (size_t)(bw / 2) * S);
          memcpy(ldsb + nn + c + y * (size / 2), gv + (size_t)y * (sy / 2), (size_t)(bw / 2) * S);
        }
      }
      t.sync();
      TeamWs<PIX> w;
      memset(&w, 0, sizeof w);
      w.rec_y = ry; w.rec_u = ry + nn; w.rec_v = ry + nn + c;
      if (lds_blk) { w.org_y = ldsb; w.org_u = ldsb + nn; w.org_v = ldsb + nn + c; w.org_sy = size; w.org_sc = size / 2; }
      else { w.org_y = gy; w.org_u = gu; w.org_v = gv; w.org_sy = sy; w.org_sc = sy / 2; }
      Node nd;
      memset(&nd, 0, sizeof nd);
      nd.size = size; nd.bw = bw; nd.bh = bh;
      const unsigned long long ssd_g = ssd_total(t, ssd_part<SP_GLOBAL>(t, gy, sy, (const PIX*)ry, size, bw, bh));
      unsigned long long ssd_l = ~0ull, cost, cost_y;
      if (lds_blk) {
        ssd_l = ssd_total(t, ssd_part<SP_LDS>(t, w.org_y, size, (const PIX*)w.rec_y, size, bw, bh));
        cost = rd_cost<PIX, SP_LDS>(t, J, &w, nd, nbits, lambda[i]);
        cost_y = rd_cost<PIX, SP_LDS>(t, J, &w, nd, nbits, lambda[i], (long long)ssd_l);
      } else {
        cost = rd_cost<PIX, SP_GLOBAL>(t, J, &w, nd, nbits, lambda[i]);
        cost_y = rd_cost<PIX, SP_GLOBAL>(t, J, &w, nd, nbits, lambda[i], (long long)ssd_g);
      }
      if (r == 0) { unsigned long long* o = out + (size_t)kKatCostOut * i; o[0] = ssd_g; o[1] = ssd_l; o[2] = cost; o[3] = cost_y; }
    }
  });
  free(planes); free(recs); free(ldsb);
  return rc;
}
// intra_sad_search with the arguments of thor_hip_kat_intra_search; blocks up to kLdsBlk take the SP_LDS instance, as on the device
template <typename PIX>
static int intra_search(int lanes, int n, const int* par, const PIX* plane, int fw, int fh, const PIX* org, long long nsamp, int bitdepth, int* out) {
  if (n <= 0 || !par || !plane || !org || !out || fw < 8 || fh < 8 || fw % 8 || fh % 8) return 1;
  for (int i = 0; i < n; i++)
    if (int r = kat_intra_check(par + kKatIntraPar * i, fw, fh, nsamp)) return r;
  static FrameJob<PIX> J;
  static IntraEdge<PIX> edge;
  J.cfg.width = fw; J.cfg.height = fh; J.cfg.bitdepth = bitdepth;
  J.rec.y = const_cast<PIX*>(plane); J.rec.sy = fw;
  PIX* ob = (PIX*)aligned_alloc(64, (size_t)64 * 64 * sizeof(PIX));
  PIX* pb = (PIX*)aligned_alloc(64, (size_t)64 * 64 * sizeof(PIX));
  if (!ob || !pb) return 3;
  const int rc = run_team(lanes, [&](int r) {
    const Team t = mk_team(r, lanes);
    for (int i = 0; i < n; i++) {
      const int* q = par + kKatIntraPar * i;
      const int size = q[2];
      t.sync();
      if (r == 0) {
        J.cfg.sb_shift = q[3] == kMaxSb ? 0 : 1;
        memcpy(ob, org + q[5], (size_t)size * size * sizeof(PIX));
      }
      t.sync();
      TeamWs<PIX> w;
      memset(&w, 0, sizeof w);
      w.edgep = &edge; w.pred_y = pb; w.org_y = ob; w.org_sy = size;
      Node nd;
      memset(&nd, 0, sizeof nd);
      nd.ypos = q[0]; nd.xpos = q[1]; nd.size = size; nd.bw = size; nd.bh = size;
      int mode = -1;
      const unsigned sad = size <= kLdsBlk ? intra_sad_search<PIX, SP_LDS>(t, J, &w, nd, q[4], &mode) : intra_sad_search<PIX, SP_GLOBAL>(t, J, &w, nd, q[4], &mode);
      if (r == 0) { out[kKatIntraOut * i] = mode; out[kKatIntraOut * i + 1] = (int)sad; }
    }
  });
  free(ob); free(pb);
  return rc;
}
extern "C" int h_intra_search(int lanes, int n, const int* par, const void* plane, int fw, int fh, const void* org, long long nsamp, int bitdepth, int* out) {
  if (bitdepth == 8) return intra_search<uint8_t>(lanes, n, par, (const uint8_t*)plane, fw, fh, (const uint8_t*)org, nsamp, 8, out);
  if (bitdepth >= 9 && bitdepth <= 12) return intra_search<uint16_t>(lanes, n, par, (const uint16_t*)plane, fw, fh, (const uint16_t*)org, nsamp, bitdepth, out);
  return 1;
}
// build_org8 with the arguments of thor_hip_kat_build_org8: out_global from the original with the item's skew and stride, out_lds (blocks up to kLdsBlk) from an
// aligned compact copy
template <typename PIX>
static int org8(int lanes, int n, const int* par, const PIX* org, const PIX* pred, long long nsamp, int bitdepth, PIX* outg, PIX* outl) {
  const int S = (int)sizeof(PIX);
  if (n <= 0 || !par || !org || !pred || !outg || !outl) return 1;
  size_t most = 0;
  for (int i = 0; i < n; i++) {
    const int* q = par + kKatOrg8Par * i;
    if (int r = kat_org8_check(q, nsamp, S)) return r;
    const size_t need = q[2] / S + (size_t)(q[0] - 1) * q[3] + q[0];
    if (need > most) most = need;
  }
  PIX* pl = (PIX*)aligned_alloc(64, (most * S + 63) / 64 * 64);
  PIX* pools = (PIX*)aligned_alloc(64, ((size_t)nsamp * 3 * S + 63) / 64 * 64 + 192);   // prediction | result (global) | result (LDS), each 64-byte aligned
  PIX* ob = (PIX*)aligned_alloc(64, (size_t)kLdsBlk * kLdsBlk * S);
  if (!pl || !pools || !ob) return 3;
  const size_t pstep = ((size_t)nsamp * S + 63) / 64 * 64 / S;
  PIX *pp = pools, *pg = pools + pstep, *plds = pools + 2 * pstep;
  memcpy(pp, pred, (size_t)nsamp * S); memcpy(pg, outg, (size_t)nsamp * S); memcpy(plds, outl, (size_t)nsamp * S);
  const int rc = run_team(lanes, [&](int r) {
    const Team t = mk_team(r, lanes);
    for (int i = 0; i < n; i++) {
      const int* q = par + kKatOrg8Par * i;
      const int size = q[0], off = q[1], sk = q[2] / S, st = q[3];
      t.sync();
      if (r == 0) {
        for (int y = 0; y < size; y++) memcpy(pl + sk + (size_t)y * st, org + off + (size_t)y * size, (size_t)size * S);
        if (size <= kLdsBlk) memcpy(ob, org + off, (size_t)size * size * S);
      }
      t.sync();
      build_org8<PIX, SP_GLOBAL>(t, pg + off, pl + sk, st, pp + off, size, bitdepth);
      if (size <= kLdsBlk) build_org8<PIX, SP_LDS>(t, plds + off, ob, size, pp + off, size, bitdepth);
      t.sync();
    }
  });
  memcpy(outg, pg, (size_t)nsamp * S); memcpy(outl, plds, (size_t)nsamp * S);
  free(pl); free(pools); free(ob);
  return rc;
}
extern "C" int h_build_org8(int lanes, int n, const int* par, const void* org, const void* pred, long long nsamp, int bitdepth, void* outg, void* outl) {
  if (bitdepth == 8) return org8<uint8_t>(lanes, n, par, (const uint8_t*)org, (const uint8_t*)pred, nsamp, 8, (uint8_t*)outg, (uint8_t*)outl);
  if (bitdepth >= 9 && bitdepth <= 12) return org8<uint16_t>(lanes, n, par, (const uint16_t*)org, (const uint16_t*)pred, nsamp, bitdepth, (uint16_t*)outg, (uint16_t*)outl);
  return 1;
}
extern "C" int h_lds_block(void) { return kLdsBlk; }
extern "C" int h_block_cost(int lanes, int n, const int* par, const double* lambda, const void* org, const void* rec, long long nsamp, int bitdepth, unsigned long long* out) {
  if (bitdepth == 8) return block_cost<uint8_t>(lanes, n, par, lambda, (const uint8_t*)org, (const uint8_t*)rec, nsamp, 8, out);
  if (bitdepth >= 9 && bitdepth <= 12) return block_cost<uint16_t>(lanes, n, par, lambda, (const uint16_t*)org, (const uint16_t*)rec, nsamp, bitdepth, out);
  return 1;
}
