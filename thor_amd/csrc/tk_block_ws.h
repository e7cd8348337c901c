// tk_block_ws.h - working set of the block decision: Node, WgShared, SmallWs / BigWs / TeamWs, ws_select, org_select, make_ws, profile slots.
#pragma once
#include "tk_common.h"
#include "tk_bits.h"
#include "tk_pred.h"
#include "tk_xform.h"
#include "tk_me.h"

namespace tk {
struct Node {
  int size, ypos, xpos, bw, bh;
  int stage, child;
  int md_done;          // top-down flow (encoder_speed > 0): mode decision already made, cost in cost_this
  unsigned cost_this;
  unsigned cost_small;
  int bitpos0;
  int encode_this_size, encode_rect;
  SynCtx syn;
  InterPred skip[2], merge[2];
  BlkParam best;
};
// Wave-uniform copy (scalar registers) of the geometry of a node that lives in LDS.
struct NodePos { int size, ypos, xpos, bw, bh; };
TK_DEV NodePos node_pos(const Node* n) {
  const auto l = ldsc(n);
  return {TKU(l->size), TKU(l->ypos), TKU(l->xpos), TKU(l->bw), TKU(l->bh)};
}

// Working set.  Per workgroup (= per superblock in flight): WgShared - constant tables, the per-SB candidate
// lists, the recursion stack of the master wave and the fork/join state of the parallel block decision.  Per
// wavefront: SmallWs (LDS: transform tiles, ME scratch, coefficient buffers, intra edges) and BigWs (sample blocks
// up to 128x128 in a global scratch arena that stays L1/L2 resident).
enum { kProfSlots = 32 };
enum { kMdMaxItems = 48 };
#ifndef TK_LDSBLK
#define TK_LDSBLK 16
#endif
enum { kLdsBlk = TK_LDSBLK };   // coding blocks up to this size keep their sample buffers in LDS (16 or 32)
enum { MD_SKIP = 0, MD_MERGE, MD_REF, MD_INTRA, MD_BIPRED, MD_TRIAL, MD_BIJOINT };
enum { WG_CMD_EXIT = 0, WG_CMD_MD = 1 };
struct MdItem { int8_t kind, a, b, pad; };
struct WgShared {
  XformTabs tabs;
  MeLists lists;
  Node stack[5];
  // ---- parallel block decision (mode_decision_par)
  int cmd;                       // what the parked waves do after the next workgroup barrier
  int next_item, n_items;        // work queue cursor (atomic) / length
  int refs_done, n_ref_items;    // reference searches finished (atomic) / expected; the last one triggers the bipred item
  int do_bipred;                 // 0 none, 1 one item (B frames), 2 lock-step phase after the queue (P frames)
  // A reference's MD_REF item searches its partitions one after the other and publishes each partition's vectors; the RDO
  // trials of (reference, partition) are queue items of their own (MD_TRIAL) that any wave takes once the vectors are there.
  int parts_done[kMaxRefs];      // partitions of reference r searched so far (atomic, released after ref_mv[r][part] is written)
  mv_t ref_mv[kMaxRefs][4][4];   // [reference][partition][quadrant]
  // bi-prediction search of P frames, run by all waves in lock step (bipred_par)
  const void* bp_org8;           // 2*org - pred of the current step (leader's buffer)
  unsigned bp_sad2[2][kMaxRefs];   // results of a lock-step search step, double-buffered (bipred_par)
  mv_t bp_mv2[2][kMaxRefs][4];
  // B frames: the telescope of the joint +mv / -mv search (motion_estimate_bi) runs as a queue item of its own (MD_BIJOINT) as soon as
  // the PART_NONE vector of its first reference is known; whoever gets there first - the item or the bi-prediction item that
  // needs its result - claims it (0 -> 1) and publishes the result (-> 2)
  int bj_state;
  unsigned bj_sad;
  mv_t bj_mv;
  int node;                      // index of the node being decided in `stack`
  mv_t mvp;
  mv_t mv_center[kMaxRefs];
  unsigned long long bestkey;    // min over finished trials of (cost << 32 | evaluation order), atomic
  unsigned long long wkey[kWaves];
  BlkParam wbest[kWaves];
  void* wsnap[kWaves];           // BigWs of wave w (its best-trial snapshot)
  MdItem items[kMdMaxItems];
  // original samples (Y, U, V; stride = block size) of the coding block being decided when it is at most kLdsBlk wide:
  // loaded once by the master, read by every trial of every wave instead of the frame in global memory
  alignas(16) unsigned char org_raw[kLdsBlk * kLdsBlk * 3];
};
// Bytes of per-wave LDS that extend the motion search's window beyond the transform workspace it borrows (tk_me_seg.h:MeWin).  The
// 8-bit kernel runs three workgroups per CU (53 KB of LDS each; two measured 12 % slower at full load, profiles/r04_call2_ab.md):
// 944 bytes more take 32x32 PUs with a reach of 16 samples.  The 16-bit kernel needs 224 VGPRs and runs two workgroups per CU
// anyway (80 KB each): 16-bit PUs up to 32x32 with a reach of 16.  -DTK_OCC=2 builds: 8-bit PUs up to 64x64.
template <typename PIX> struct WinExtra { enum { bytes = sizeof(PIX) == 1 ? (TK_OCC == 2 ? 7680 : 944) : 5376 }; };
template <typename PIX> struct SmallWs {
  XformWs xf;
  alignas(16) unsigned char win_extra[WinExtra<PIX>::bytes];   // must directly follow xf
  MeWs me;
  IntraEdge<PIX> edge;
  // quantised coefficients of the current trial; TU t of a tb-split block at offset t * qs^2 with
  // qs = min(TU size, 16).  Chroma needs more than 256 entries only for tb-split 64/128 blocks, which
  // use the BigWs buffers instead.
  int16_t coef_y[4 * 256], coef_u[256], coef_v[256];
  unsigned long long acc[12];
  // sample blocks (prediction, the two bi-prediction inputs, reconstruction, 2*org-pred) of coding blocks up to
  // kLdsBlk x kLdsBlk: the trials of the small blocks - the bulk of all trials - never round-trip through global memory
  alignas(16) PIX lbuf[7 * kLdsBlk * kLdsBlk];
#if defined(THOR_PROF)
  long long prof[kProfSlots];
#else
  long long prof[1];
#endif
};
// the row-segment loads of the motion search read the LDS sample blocks with 16-byte ds_read
static_assert(offsetof(SmallWs<uint8_t>, lbuf) % 16 == 0 && offsetof(SmallWs<uint16_t>, lbuf) % 16 == 0 && sizeof(SmallWs<uint8_t>) % 16 == 0 &&
              sizeof(SmallWs<uint16_t>) % 16 == 0 && offsetof(WgShared, org_raw) % 16 == 0, "LDS sample blocks must be 16-byte aligned");
template <typename PIX> struct BigWs {
  PIX pred_y[kMaxSb * kMaxSb], pred_u[kMaxSb * kMaxSb / 4], pred_v[kMaxSb * kMaxSb / 4];
  PIX p0_y[kMaxSb * kMaxSb], p0_u[kMaxSb * kMaxSb / 4], p0_v[kMaxSb * kMaxSb / 4];
  PIX p1_y[kMaxSb * kMaxSb], p1_u[kMaxSb * kMaxSb / 4], p1_v[kMaxSb * kMaxSb / 4];
  PIX rec_y[kMaxSb * kMaxSb], rec_u[kMaxSb * kMaxSb / 4], rec_v[kMaxSb * kMaxSb / 4];
  PIX org8[kMaxSb * kMaxSb];
  int16_t coef_u_big[4 * 256], coef_v_big[4 * 256];
  // snapshot of this wave's best trial of the current block decision (reconstruction + quantised coefficients): the final
  // encode of the winning trial copies it instead of predicting / transforming the block again (mode_decision_par)
  PIX best_y[kMaxSb * kMaxSb], best_u[kMaxSb * kMaxSb / 4], best_v[kMaxSb * kMaxSb / 4];
  int16_t best_cy[4 * 256], best_cu[4 * 256], best_cv[4 * 256];
};
template <typename PIX> struct TeamWs {  // view (lives in registers)
  XformWs* xfp;
  MeWs* mep;
  IntraEdge<PIX>* edgep;
  int16_t *coef_y, *coef_u, *coef_v;          // current (may point at the big chroma buffers)
  int16_t *coef_u_small, *coef_v_small, *coef_u_big, *coef_v_big;
  unsigned long long* acc;
  WgShared* sh;
  Node* stack;
  long long* prof;
  PIX *pred_y, *pred_u, *pred_v, *p0_y, *p0_u, *p0_v, *p1_y, *p1_u, *p1_v, *rec_y, *rec_u, *rec_v, *org8;  // current (ws_select)
  BigWs<PIX>* big;
  PIX* lbuf;
  const PIX *org_y, *org_u, *org_v;  // original samples of the current coding block (origin), strides org_sy / org_sc
  int org_sy, org_sc;
};
// On the device the per-wave view and the frame job live in LDS and are passed around as LDS-typed pointer / reference
// (ds_read of the members instead of generic loads); plain pointer / reference on the host.
#if TK_HOST
template <typename PIX> using WsP = TeamWs<PIX>*;
template <typename PIX> using JobR = const FrameJob<PIX>&;
#else
template <typename PIX> using WsP = TK_LDS TeamWs<PIX>*;
template <typename PIX> using JobR = const TK_LDS FrameJob<PIX>&;
#endif
// Point the sample-block views at the LDS buffers (coding blocks up to kLdsBlk) or at the global scratch slot.
template <class WP> TK_DEV void ws_select(WP w, int size) {  // WP: TeamWs<PIX>* in any address space
  if (size <= kLdsBlk) {
    auto b = w->lbuf;
    const int n = size * size, c = n >> 2;
    w->pred_y = b; w->pred_u = b + n; w->pred_v = b + n + c; b += n + 2 * c;
    w->p0_y = b; w->p0_u = b + n; w->p0_v = b + n + c; b += n + 2 * c;
    w->p1_y = b; w->p1_u = b + n; w->p1_v = b + n + c; b += n + 2 * c;
    w->rec_y = b; w->rec_u = b + n; w->rec_v = b + n + c; b += n + 2 * c;
    w->org8 = b;
  } else {
    auto g = w->big;
    w->pred_y = g->pred_y; w->pred_u = g->pred_u; w->pred_v = g->pred_v;
    w->p0_y = g->p0_y; w->p0_u = g->p0_u; w->p0_v = g->p0_v;
    w->p1_y = g->p1_y; w->p1_u = g->p1_u; w->p1_v = g->p1_v;
    w->rec_y = g->rec_y; w->rec_u = g->rec_u; w->rec_v = g->rec_v; w->org8 = g->org8;
  }
}
// Point ws->org_* at the original samples of coding block `nd`: the frame planes, or (blocks up to kLdsBlk) the
// workgroup's LDS copy, which the master fills with load = 1 before any wave uses it.
template <typename PIX>
TK_DEV void org_select(const Team t, JobR<PIX> J, WsP<PIX> w, int size, int ypos, int xpos, int bw, int bh, int load) {
  if (size <= kLdsBlk) {
    PIX* b = (PIX*)w->sh->org_raw;
    const int n = size * size, sc = size >> 1;
    if (load) {
      t.sync();
      const Div2 dw = mk_div(bw), dc = mk_div(bw >> 1);
      const TK_GLOBAL PIX* gy = gptr(J.orig.y + ypos * J.orig.sy + xpos);
      const TK_GLOBAL PIX* gu = gptr(J.orig.u + (ypos >> 1) * J.orig.sc + (xpos >> 1));
      const TK_GLOBAL PIX* gv = gptr(J.orig.v + (ypos >> 1) * J.orig.sc + (xpos >> 1));
      const auto bl = ldsc(b);
      for (int k = t.rank; k < bw * bh; k += t.size) { int i, j; split2(dw, k, i, j); bl[i * size + j] = gy[i * J.orig.sy + j]; }
      for (int k = t.rank; k < (bw >> 1) * (bh >> 1); k += t.size) {
        int i, j;
        split2(dc, k, i, j);
        bl[n + i * sc + j] = gu[i * J.orig.sc + j];
        bl[n + (n >> 2) + i * sc + j] = gv[i * J.orig.sc + j];
      }
      t.sync();
    }
    w->org_y = b; w->org_u = b + n; w->org_v = b + n + (n >> 2);
    w->org_sy = size; w->org_sc = sc;
  } else {
    w->org_y = J.orig.y + ypos * J.orig.sy + xpos;
    w->org_u = J.orig.u + (ypos >> 1) * J.orig.sc + (xpos >> 1);
    w->org_v = J.orig.v + (ypos >> 1) * J.orig.sc + (xpos >> 1);
    w->org_sy = J.orig.sy; w->org_sc = J.orig.sc;
  }
}

template <typename PIX> TK_DEV TeamWs<PIX> make_ws(SmallWs<PIX>* s, WgShared* sh, BigWs<PIX>* g) {
  TeamWs<PIX> w;
  w.xfp = &s->xf; w.mep = &s->me; w.edgep = &s->edge;
  w.sh = sh; s->xf.tabs = &sh->tabs; s->me.lists = &sh->lists;
  // the search window of a motion search lives in the transform workspace (in | tmp | coef: contiguous), idle during a search,
  // and continues into win_extra
  static_assert(offsetof(SmallWs<PIX>, win_extra) == offsetof(SmallWs<PIX>, xf) + sizeof(XformWs), "win_extra must directly follow the transform workspace");
  s->me.win = (uint32_t*)s->xf.in;
  s->me.win_cap = (int)(sizeof(XformWs) - offsetof(XformWs, in)) + (int)WinExtra<PIX>::bytes;
  s->me.cwin_valid = 0;
  w.coef_y = s->coef_y; w.coef_u = s->coef_u; w.coef_v = s->coef_v;
  w.coef_u_small = s->coef_u; w.coef_v_small = s->coef_v; w.coef_u_big = g->coef_u_big; w.coef_v_big = g->coef_v_big;
  w.acc = s->acc; w.stack = sh->stack; w.prof = s->prof;
  s->xf.prof = s->prof; s->me.prof = s->prof;
  w.big = g; w.lbuf = s->lbuf;
  w.org_y = w.org_u = w.org_v = nullptr; w.org_sy = w.org_sc = 0;
  ws_select(&w, kMaxSb);
  return w;
}

// -DTHOR_PROF -DTHOR_PROF_MD: slots 16..25 hold the time of the decision's work-queue items by kind (all waves) and of the phases
// the master runs alone, instead of the transform-unit sizes: 16 skip/merge items, 17 intra items, 18 search items (MD_REF),
// 19 trial items incl. their wait for the vectors, 20 wait of the trial items alone, 21 queue set-up (master), 22 block entry
// (contexts, candidates, original block), 23 early-skip path (check + trial + final encode), 24 final encode of decided blocks: bit emission
// (one lane), 25 final encode of decided blocks: reconstruction copy + cell state.
// -DTHOR_PROF_MD_PARTS=mask (default 7) keeps only some of them - 1: the items inside md_worker_sp's loop, 2: the trial items' wait, 4: the
// master's phases - and mask bit 8 makes the loop counters accumulate in registers and store once after the loop (bisection of the
// hang of the fully instrumented build, profiles/r04_call2_ab.md).
#if TK_PROF_MD
#ifndef THOR_PROF_MD_PARTS
#define THOR_PROF_MD_PARTS 7
#endif
#define TK_PROFMD_MARK(v) TK_PROF_MARK(v)
#define TK_PROFMD_ACC(ws, id, v) TK_PROF_ACC(ws, id, v)
#define TK_PROFMD_CNT(ws, id) TK_PROF_CNT(ws, id)
#define TK_PROFMD_ON(bit) ((THOR_PROF_MD_PARTS) & (bit))
#else
#define TK_PROFMD_ON(bit) 0
#define TK_PROFMD_MARK(v) do {} while (0)
#define TK_PROFMD_ACC(ws, id, v) do {} while (0)
#define TK_PROFMD_CNT(ws, id) do {} while (0)
#endif
enum { PF_SB = 0, PF_ESKIP, PF_ME_FULL, PF_ME_SUB, PF_PRED_INTER, PF_PRED_INTRA, PF_TU, PF_BITS, PF_COST, PF_FINAL,
       PF_CFL, PF_BIPRED_PREP, PF_QUANT };
}  // namespace tk
