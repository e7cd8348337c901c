// kat_host_me.cpp - TEST INFRASTRUCTURE ONLY.  The host build of the device functions motion_estimate / motion_estimate_bi / me_stage_cb_window
// (thor_amd/csrc/tk_me.h) behind one batch call, so that tests/golden/kat8.npz (recorded from the reference's file-static motion_estimate /
// motion_estimate_bi, tests/golden/gen_kat8.py) pins them on the CPU (tests/test_kat_host.py) - the CPU twin of thor_hip_kat_motion_estimate / _bi
// (thor_amd/csrc/hip_kat.h, tests/test_gpu_kat.py).  Workspace as the product builds it (make_ws: the search window in the transform workspace + win_extra,
// the product's win_cap); the original block is the compact copy (stride = CB size) for CBs up to kLdsBlk and the frame plane above, as ws_select / org_select
// choose.  Plain build: 1-lane teams.  -DTHOR_HOSTSIM_LANES=64 -pthread: teams of `lanes` OS threads (the exchange of tests/hostsim/unit_me_lanes.cpp), which
// take the lane-per-candidate evaluators of tk_me_lanes.h.
#include "../../thor_amd/csrc/tk_block.h"
#include "../../thor_amd/csrc/tk_tables.h"
#include <cstring>
#ifdef THOR_HOSTSIM_LANES
#include <atomic>
#include <thread>
#include <vector>
#endif
namespace tk {
Tables g_tab;
long long g_prune_stat[8];
#ifdef THOR_HOSTSIM_LANES
namespace hostlanes {   // every lane is an OS thread; one exchange primitive (publish a value, read everybody's), as in tests/hostsim/unit_me_lanes.cpp
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

// par[17 * i ..]: cb_x, cb_y, cb, pu_dx, pu_dy, pw, ph, mvc.x, mvc.y, mvp.x, mvp.y, sign, enable_bipred, encoder_speed, ncand, cand_off, stage (layout of kat8.npz)
enum { NPAR = 17 };

template <typename PIX> struct HostWs {
  SmallWs<PIX> sws;
  WgShared sh;
  BigWs<PIX> big;
};

// items [0, n) by the lane `r` of a team of `lanes`; every lane runs the same sequence (the team's barriers pair up)
template <typename PIX>
static void run_items(int r, int lanes, HostWs<PIX>* H, int bi, int bitdepth, const PIX* cur, const PIX* ref0, const PIX* ref1, int stride, int fw, int fh, int n,
                      const int* par, const double* lam, const int16_t* cand, int* out, int16_t* list_out) {
  const Team t = mk_team(r, lanes);
  TeamWs<PIX> ws = make_ws(&H->sws, &H->sh, &H->big);
  MeWs* me = ws.mep;
  MeLists* lists = &H->sh.lists;
  PIX* orgc = (PIX*)H->sh.org_raw;
  for (int it = 0; it < n; it++) {
    const int* q = par + NPAR * it;
    const int cbx = q[0], cby = q[1], cb = q[2], pux = cbx + q[3], puy = cby + q[4];
    t.sync();
    if (r == 0) {
      memset(lists, 0, sizeof(*lists));
      const int nl = bi ? 6 : q[14];
      for (int c = 0; c < nl; c++) { lists->mvcand[0][c].x = cand[2 * (q[15] + c)]; lists->mvcand[0][c].y = cand[2 * (q[15] + c) + 1]; }
      lists->mvcand_num[0] = q[14];
      me->cwin_valid = 0;
    }
    const int lds_blk = cb <= kLdsBlk;
    if (lds_blk)
      for (int k = r; k < cb * cb; k += lanes) orgc[k] = cur[(size_t)(cby + k / cb) * stride + cbx + k % cb];
    t.sync();
    MeArgs a;
    a.cb_size = cb; a.ostride = lds_blk ? cb : stride; a.width = q[5]; a.height = q[6]; a.rstride = stride; a.sign = q[11]; a.fwidth = fw; a.fheight = fh;
    a.xpos = cbx; a.ypos = cby; a.pu_x = pux; a.pu_y = puy; a.enable_bipred = q[12]; a.bitdepth = bitdepth; a.speed = q[13]; a.lam = lam[it];
    const mv_t mvc = mk_mv(q[7], q[8]), mvp = mk_mv(q[9], q[10]);
    const PIX* org = lds_blk ? orgc + q[4] * cb + q[3] : cur + (size_t)puy * stride + pux;
    mv_t mv = mk_mv(0, 0);
    unsigned cost;
    if (bi) {
      const PIX* r0 = ref0 + (size_t)cby * stride + cbx;
      const PIX* r1 = ref1 + (size_t)cby * stride + cbx;
      cost = lds_blk ? motion_estimate_bi<PIX, SP_LDS>(t, me, org, r0, r1, a, mvc, mvp, 0, &mv) : motion_estimate_bi<PIX, SP_GLOBAL>(t, me, org, r0, r1, a, mvc, mvp, 0, &mv);
    } else {
      if (q[16]) me_stage_cb_window<PIX>(t, me, ref0 + (size_t)cby * stride + cbx, stride, cbx, cby, cb, mvc, a.sign, fw, fh, 0);
      const PIX* rp = ref0 + (size_t)puy * stride + pux;
      cost = lds_blk ? motion_estimate<PIX, SP_LDS>(t, me, org, rp, a, mvc, mvp, 0, &mv) : motion_estimate<PIX, SP_GLOBAL>(t, me, org, rp, a, mvc, mvp, 0, &mv);
    }
    t.sync();
    if (r == 0) {
      out[3 * it] = mv.x; out[3 * it + 1] = mv.y; out[3 * it + 2] = (int)cost;
      if (bi) for (int c = 0; c < 6; c++) { list_out[12 * it + 2 * c] = lists->mvcand[0][c].x; list_out[12 * it + 2 * c + 1] = lists->mvcand[0][c].y; }
    }
  }
}

template <typename PIX>
static int me_batch(int bi, int bitdepth, int lanes, const PIX* cur, const PIX* ref0, const PIX* ref1, int stride, int fw, int fh, int n, const int* par,
                    const double* lam, const int16_t* cand, int* out, int16_t* list_out) {
  static HostWs<PIX> H;
  static bool inited = false;
  if (!inited) { init_tables(&g_tab); inited = true; }
  xform_tables_fill(&H.sh.tabs, 0, 1);
#ifdef THOR_HOSTSIM_LANES
  if (lanes < 1 || lanes > 64) return 1;
  hostlanes::Shared sh;
  sh.n = lanes;
  std::vector<std::thread> th;
  for (int r = 0; r < lanes; r++)
    th.emplace_back([&, r]() {
      hostlanes::tl_sh = &sh; hostlanes::tl_rank = r; hostlanes::tl_sense = 0;
      run_items<PIX>(r, lanes, &H, bi, bitdepth, cur, ref0, ref1, stride, fw, fh, n, par, lam, cand, out, list_out);
    });
  for (auto& x : th) x.join();
#else
  if (lanes != 1) return 1;
  run_items<PIX>(0, 1, &H, bi, bitdepth, cur, ref0, ref1, stride, fw, fh, n, par, lam, cand, out, list_out);
#endif
  return 0;
}

// cur / ref0 / ref1: sample (0, 0) of three planes of `stride` samples per row with kPadY samples of replicate padding on every side (ref1: bi only).
// out[3 * i ..]: mv.x, mv.y, cost; list_out[12 * i ..] (bi): the six list entries (x, y) as the call leaves them.
extern "C" int h_me_batch(int bi, int bitdepth, int lanes, const void* cur, const void* ref0, const void* ref1, int stride, int fw, int fh, int n, const int* par,
                          const double* lam, const int16_t* cand, int* out, int16_t* list_out) {
  if (bitdepth == 8)
    return me_batch<uint8_t>(bi, 8, lanes, (const uint8_t*)cur, (const uint8_t*)ref0, (const uint8_t*)ref1, stride, fw, fh, n, par, lam, cand, out, list_out);
  return me_batch<uint16_t>(bi, bitdepth, lanes, (const uint16_t*)cur, (const uint16_t*)ref0, (const uint16_t*)ref1, stride, fw, fh, n, par, lam, cand, out, list_out);
}
