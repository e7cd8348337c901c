// kat_host_bits.cpp - TEST INFRASTRUCTURE ONLY.  The host build of the block syntax writer and its bit counter (thor_amd/csrc/tk_bits.h: bs_vlc / bs_mv /
// bs_coeff / bs_coeff_team / coeff_bits_team / bs_super_mode / bs_block_head_t / bs_block_t, counting and emitting) behind two batch calls, so that
// tests/golden/kat9.npz (recorded from the reference's put_vlc, write_mv, write_coeff, write_super_mode and write_block, tests/golden/gen_kat9.py) pins them on
// the CPU (tests/test_kat_host.py) - the CPU twin of thor_hip_kat_coeff_syntax / thor_hip_kat_block_syntax (thor_amd/csrc/hip_kat.h, tests/test_gpu_kat.py).
// Both run the items through thor_amd/csrc/tk_kat_bits.h.  Plain build: 1-lane teams.  -DTHOR_HOSTSIM_LANES=64 -pthread: teams of `lanes` OS threads (8, 16, 64:
// the widths of tests/test_reference_golden.py), which take coeff_bits_team's ballot automaton with W = lanes; bs_coeff_team's readlane form is device-only.
#include "../../thor_amd/csrc/tk_block.h"
#include "../../thor_amd/csrc/tk_tables.h"
#include "../../thor_amd/csrc/tk_kat_bits.h"
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
namespace hostlanes {   // every lane is an OS thread; one exchange primitive (publish a value, read everybody's), as in tests/hostsim/kat_host_me.cpp
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
  static bool inited = false;
  if (!inited) { init_tables(&g_tab); inited = true; }
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

// The arguments of thor_hip_kat_coeff_syntax (include/thor_hip.h) plus the team width.
extern "C" int h_coeff_syntax(int lanes, int n, const int* par, const int16_t* coef, int words, uint32_t* buf_single, uint32_t* buf_team, int* out) {
  for (int i = 0; i < n; i++) if (kat_coeff_check(par + kKatCoPar * i, words)) return 1;
  return run_team(lanes, [&](int r) {
    const Team t = mk_team(r, lanes);
    for (int i = 0; i < n; i++) {
      t.sync();
      kat_coeff_item(t, par + kKatCoPar * i, coef + (size_t)i * 256, coef + (size_t)i * 256, buf_single + (size_t)i * words, buf_team + (size_t)i * words, out + kKatCoOut * i);
    }
  });
}

// The arguments of thor_hip_kat_block_syntax plus the team width.
extern "C" int h_block_syntax(int lanes, int n, const int* par, const int16_t* pool, int npool, int words, uint32_t* buf_coop, uint32_t* buf_single, int* out) {
  std::vector<int16_t> coef((size_t)n * 3072);
  for (int i = 0; i < n; i++) if (kat_block_resolve(par + kKatBlPar * i, pool, npool, coef.data() + (size_t)i * 3072)) return 1;
  return run_team(lanes, [&](int r) {
    const Team t = mk_team(r, lanes);
    for (int i = 0; i < n; i++) {
      const int16_t* c = coef.data() + (size_t)i * 3072;
      const int* q = par + kKatBlPar * i;
      const int fits = !(q[0] == 0 && q[25] && q[9] >= 64);
      t.sync();
      kat_block_item(t, q, c, fits ? c + 1024 : nullptr, fits ? c + 2048 : nullptr, c, c + 1024, c + 2048, words * 32, buf_coop + (size_t)i * words, buf_single + (size_t)i * words,
                     out + kKatBlOut * i);
    }
  });
}
