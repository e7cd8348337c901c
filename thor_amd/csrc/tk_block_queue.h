// tk_block_queue.h - the block decision as an LDS work queue over the waves of the workgroup: par_trial .. mode_decision_par, wg_helper_loop.
#pragma once
#include "tk_block_md.h"

namespace tk {
// ---------------------------------------------------------------------------------
// mode_decision_rdo for the encoder_speed 0 operating points, spread over the wavefronts of the workgroup.
//
// The reference walks the trials of a block one after the other and keeps the first strictly smaller cost
// (encode_block.c:1885-2114).  Given the entry state most of them are independent:
//   * the uni-prediction search of each reference (its candidate list mvcand[r] is private to the reference) and the
//     12 RDO trials that follow it,
//   * the skip / merge candidates,
//   * the 10 intra modes x 2 transform splits,
// and only the bi-prediction search needs something from the others (the PART_NONE vector of every reference).
// Every such unit is a work item in a queue in LDS; the waves pop items until the queue is empty; the wave that
// finishes the LAST reference search runs the bi-prediction item.  Every trial has the index of its position in the
// reference's evaluation order, the winner is the trial with the smallest (cost << 32 | order) - the very trial the
// sequential strict-'<' scan would keep - and pruning compares lower-bound keys with the shared minimum (PruneCtx).
// With a single wave the queue is simply processed in the reference's order.
// Evaluation order indices: skip k: k | merge k, tb: 2+2k+tb | inter r, part, tb: 6+12r+3part+(tb+1) |
// bipred tb: 54+tb, joint (B frames): 56 | intra m, tb: 57+2m+tb.
// ---------------------------------------------------------------------------------
TK_DEV BlkParam blank_param() {
  BlkParam p;
  p.mode = M_SKIP; p.intra_mode = 0; p.skip_idx = 0; p.pb_part = P_NONE; p.ref0 = p.ref1 = 0; p.dir = 0;
  p.tb_param = 0; p.tb_split = 0; p.cbp_y = p.cbp_u = p.cbp_v = 0;
  for (int i = 0; i < 4; i++) { p.mv0[i] = mk_mv(0, 0); p.mv1[i] = mk_mv(0, 0); }
  return p;
}

// Keep the trial that is in ws->rec_* / ws->coef_* (reconstruction and quantised coefficients of a square block of `size`)
// in the wave's snapshot buffers.
template <typename PIX, int SP>
TK_DEV void snapshot_trial(const Team t, WsP<PIX> ws, int size, const BlkParam& p) {
  BigWs<PIX>* g = ws->big;
  const int sc = size >> 1;
  copy_block<SP_GLOBAL, SP>(t, g->best_y, size, ws->rec_y, size, size, size);
  copy_block<SP_GLOBAL, SP>(t, g->best_u, sc, ws->rec_u, sc, sc, sc);
  copy_block<SP_GLOBAL, SP>(t, g->best_v, sc, ws->rec_v, sc, sc, sc);
  if (TKU(p.cbp_y) | TKU(p.cbp_u) | TKU(p.cbp_v)) {
    const int tbs = TKU(p.tb_split);
    const int qy = tbs ? tmin(size >> 1, (int)kMaxQuant) : tmin(size, (int)kMaxQuant);
    const int ny = (tbs ? 4 : 1) * qy * qy;
    const int csplit = tbs && sc > 4;
    const int qc = csplit ? tmin(sc >> 1, (int)kMaxQuant) : tmin(sc, (int)kMaxQuant);
    const int nc = (csplit ? 4 : 1) * qc * qc;
    const int16_t *cy = ws->coef_y, *cu = ws->coef_u, *cv = ws->coef_v;
    TK_GLOBAL int16_t* dy = gptr(g->best_cy);
    TK_GLOBAL int16_t* du = gptr(g->best_cu);
    TK_GLOBAL int16_t* dv = gptr(g->best_cv);
    for (int k = t.rank; k < ny; k += t.size) dy[k] = cy[k];
    for (int k = t.rank; k < nc; k += t.size) { du[k] = cu[k]; dv[k] = cv[k]; }
  }
}

template <typename PIX> struct MdCtx {
  Wg wg;
  WgShared* sh;
  Node* nd;
  unsigned long long mykey;  // best key among this wave's trials
};

// Returns 0 when the trial was dropped before it touched the prediction buffers (rdo_trial: `untouched`), 1 otherwise.
template <typename PIX, int SP>
TK_DEV int par_trial(const Team t, JobR<PIX> J, WsP<PIX> ws, MdCtx<PIX>& M, BlkParam& p, unsigned order, int reuse_pred) {
  int untouched = 0;
  const unsigned cost = rdo_trial<PIX, SP>(t, J, ws, *M.nd, p, J.lambda, reuse_pred, 0xffffffffu, &M.sh->bestkey, order, nullptr, &untouched);
  if (cost == (unsigned)kCostInit) return !untouched;  // pruned: cannot have the smallest key
  const unsigned long long key = ((unsigned long long)cost << 32) | order;
  if (key < M.mykey) {
    M.mykey = key;
    if (t.rank == 0) {
      lds_st(&M.sh->wbest[M.wg.wave], normalize_best(*M.nd, p));
      *ldsc(&M.sh->wkey[M.wg.wave]) = key;
      wg_min64(&M.sh->bestkey, key);
    }
    snapshot_trial<PIX, SP>(t, ws, tk_uniform(ldsc(M.nd)->size), p);
    t.sync();
  }
  return 1;
}

// Wait (with the limit of every intra-workgroup wait) until *p, an LDS word another wave releases, reaches `at_least`.
TK_DEV void wg_wait_at_least(const Team t, int* p, int at_least) {
  const unsigned long long w0 = wg_clock();
  for (unsigned spins = 1;; spins++) {
    const int d = wg_load_acquire(p);   // every lane acquires (one broadcast LDS read)
    if (team_bcast0(t, d) >= at_least) break;
    if ((spins & 1023u) == 0 && tk_uniform64(wg_clock() - w0) > (unsigned long long)kWgWaitLimit) wg_wait_failed();
    wg_pause();
  }
}
// Telescope of the joint +mv / -mv search of a B frame (search_bipred_prediction_params me_mode 1, encode_block.c:1708-1737): claimed
// by the first wave that gets to it; result in sh->bj_sad / bj_mv, bj_state = 2.  Returns 0 when another wave has claimed it.
template <typename PIX, int SP>
TK_DEVNI int md_bijoint_telescope(const Team t, JobR<PIX> J, WsP<PIX> ws, MdCtx<PIX>& M) {
  const auto& c = J.cfg;
  WgShared* const sh_ = tk_uniform_ptr(M.sh);
  int mine = 0;
  if (t.rank == 0) mine = wg_cas(&sh_->bj_state, 0, 1);
  if (!team_bcast0(t, mine)) return 0;
  const NodePos nd = node_pos(M.nd);
  const int ri0 = J.interp_ref ? 1 : 0, ri1 = J.interp_ref ? 2 : 1;
  const Plane3<PIX> f0 = lds_ld(&J.ref[ri0]);
  const Plane3<PIX> f1 = lds_ld(&J.ref[ri1]);
  MeArgs a;
  a.cb_size = nd.size; a.ostride = ws->org_sy; a.width = nd.size; a.height = nd.size; a.rstride = f0.sy; a.sign = 0;
  a.fwidth = c.width; a.fheight = c.height; a.xpos = nd.xpos; a.ypos = nd.ypos; a.enable_bipred = 1;
  a.bitdepth = c.bitdepth; a.lam = J.sqrt_lambda; a.speed = c.encoder_speed; a.pu_x = nd.xpos; a.pu_y = nd.ypos;
  mv_t mvb = mk_mv(0, 0);
  const mv_t ctr = lds_ld(&sh_->ref_mv[ri0][0][0]);   // PART_NONE vector of the first reference = mv_center[ri0]
  const unsigned sad = motion_estimate_bi<PIX, SP>(t, ws->mep, ws->org_y, f0.y + nd.ypos * f0.sy + nd.xpos, f1.y + nd.ypos * f1.sy + nd.xpos, a, ctr,
                                                   lds_ld(&sh_->mvp), ri0, &mvb, 1);
  t.sync();
  if (t.rank == 0) {
    *ldsc(&sh_->bj_sad) = sad;
    lds_st(&sh_->bj_mv, mvb);
    wg_store_release(&sh_->bj_state, 2);
  }
  t.sync();
  return 1;
}

template <typename PIX, int SP>
TK_DEVNI void md_item_bipred(const Team t, JobR<PIX> J, WsP<PIX> ws, MdCtx<PIX>& M) {
  const auto& c = J.cfg;
  Node& nd_ = *M.nd;
  const NodePos nd = node_pos(&nd_);
  const int size = nd.size;
  const int max_tb = c.enable_tb_split == 1 ? 2 : 1;
  const mv_t mvp = lds_ld(&M.sh->mvp);
  mv_t mv_center[kMaxRefs];
  for (int r = 0; r < kMaxRefs; r++) mv_center[r] = lds_ld(&M.sh->mv_center[r]);
  int r0, r1;
  mv_t a0[4], a1[4];
  search_bipred<PIX, SP>(t, J, ws, nd_, 0, mv_center, mvp, &r0, &r1, a0, a1);
  BlkParam p = blank_param();
  p.mode = M_BIPRED; p.pb_part = P_NONE;
  p.ref0 = (int8_t)r0; p.ref1 = (int8_t)r1;
  for (int i = 0; i < 4; i++) { p.mv0[i] = a0[i]; p.mv1[i] = a1[i]; }
  for (int tb = 0, have_pred = 0; tb <= max_tb - 1; tb++) {
    p.tb_param = (int8_t)tb;
    have_pred |= par_trial<PIX, SP>(t, J, ws, M, p, 54u + (unsigned)tb, have_pred);
  }
  if (J.frame_type == F_B) {
    // joint +mv / -mv search (search_bipred_prediction_params me_mode 1, encode_block.c:1708-1737, 2052-2068)
    const int ri0 = J.interp_ref ? 1 : 0, ri1 = J.interp_ref ? 2 : 1;
    const Plane3<PIX> f0 = lds_ld(&J.ref[ri0]);
    const Plane3<PIX> f1 = lds_ld(&J.ref[ri1]);
    const PIX* oy = ws->org_y;
    MeArgs a;
    a.cb_size = size; a.ostride = ws->org_sy; a.width = size; a.height = size; a.rstride = f0.sy; a.sign = 0;
    a.fwidth = c.width; a.fheight = c.height; a.xpos = nd.xpos; a.ypos = nd.ypos; a.enable_bipred = 1;
    a.bitdepth = c.bitdepth; a.lam = J.sqrt_lambda; a.speed = c.encoder_speed; a.pu_x = nd.xpos; a.pu_y = nd.ypos;
    // the telescope of the joint search has run (or is running) on the wave that took the MD_BIJOINT item - or runs here if nobody
    // has claimed it yet; the extra candidates read the candidate list as the searches above left it
    WgShared* const sh_ = tk_uniform_ptr(M.sh);
    if (!md_bijoint_telescope<PIX, SP>(t, J, ws, M)) wg_wait_at_least(t, &sh_->bj_state, 2);
    mv_t mvb = lds_ld(&sh_->bj_mv);
    const unsigned sad0 = (unsigned)tk_uniform((int)*ldsc(&sh_->bj_sad));
    motion_estimate_bi<PIX, SP>(t, ws->mep, oy, f0.y + nd.ypos * f0.sy + nd.xpos, f1.y + nd.ypos * f1.sy + nd.xpos, a, mv_center[ri0], mvp, ri0, &mvb, 2, sad0);
    p.mode = M_BIPRED; p.pb_part = P_NONE;
    p.ref0 = (int8_t)ri0; p.ref1 = (int8_t)ri1;
    for (int i = 0; i < 4; i++) { p.mv0[i] = mvb; p.mv1[i] = mvb; }
    p.tb_param = 0;
    par_trial<PIX, SP>(t, J, ws, M, p, 56u, 0);
  }
}

// MD_REF: the motion searches of one reference (encode_block.c:1966-1984) - partition after partition, each one seeded by
// the candidates the earlier ones left in mvcand[r].  The vectors of a partition are published as soon as it is searched.
template <typename PIX, int SP>
TK_DEVNI void md_item_ref(const Team t, JobR<PIX> J, WsP<PIX> ws, MdCtx<PIX>& M, int r) {
  const auto& c = J.cfg;
  const NodePos nd = node_pos(M.nd);
  const int size = nd.size;
  const int max_pb = c.enable_pb_split ? 4 : 1;
  const mv_t mvp = lds_ld(&M.sh->mvp);
  const PIX* oy = ws->org_y;
  if (t.rank == 0) add_mvcand(ws->mep, r, mvp);
  t.sync();
  mv_t mv_center = mvp;
  if (t.rank == 0) ldsc(ws->mep)->cwin_valid = 0;
  t.sync();
  for (int part = 0; part < max_pb; part++) {
    mv_t mv_all[4];
    search_inter<PIX, SP>(t, J, ws, nd.ypos, nd.xpos, size, oy, ws->org_sy, r, mv_center, mvp, mv_all, part, J.sign[r]);
    add_cands4(t, ws, r, mv_all);
    if (part == 0) {
      mv_center = mv_all[0];
      // the eight searches of the HOR / VER / QUAD partitions all start from mv_center: one window for the block
      if (max_pb > 1) {
        const Plane3<PIX> rp = lds_ld(&J.ref[r]);
        me_stage_cb_window<PIX>(t, ws->mep, rp.y + nd.ypos * rp.sy + nd.xpos, rp.sy, nd.xpos, nd.ypos, size, mv_center, J.sign[r], c.width, c.height, r);
      }
    }
    if (t.rank == 0) {
      for (int i = 0; i < 4; i++) lds_st(&M.sh->ref_mv[r][part][i], mv_all[i]);
      if (part == max_pb - 1) lds_st(&M.sh->mv_center[r], mv_center);
      wg_fetch_add(&M.sh->parts_done[r], 1);   // release: the vectors above are visible to the wave that sees the count
    }
    t.sync();
  }
  if (t.rank == 0) ldsc(ws->mep)->cwin_valid = 0;   // the transform workspace the window lives in is about to be used again
  t.sync();
}

// MD_TRIAL: the RDO trials of one (reference, partition) (encode_block.c:1993-2012): tb_param -1 (no residual), 0 and 1 share one prediction.
template <typename PIX, int SP>
TK_DEVNI void md_item_trial(const Team t, JobR<PIX> J, WsP<PIX> ws, MdCtx<PIX>& M, int r, int part) {
  const auto& c = J.cfg;
  const int max_tb = c.enable_tb_split == 1 ? 2 : 1;
  r = tk_uniform(r); part = tk_uniform(part);
  WgShared* const sh_ = tk_uniform_ptr(M.sh);
  // the reference's search item was taken from the queue before this one: it is finished or running on another wave.  A wait of
  // kWgWaitLimit wall-clock ticks (a search item takes milliseconds) is a protocol error: wg_wait_failed() stops the kernel / the
  // simulation loudly instead of hanging the GPU (the host reports the aborted launch, hip_backend.h:run_superblocks).
  TK_PROFMD_MARK(pwt_);
  wg_wait_at_least(t, &sh_->parts_done[r], part + 1);
  if (TK_PROFMD_ON(2)) TK_PROFMD_ACC(ws, 20, pwt_);
  mv_t mv_all[4][4];
  for (int q = 0; q <= part; q++)
    for (int i = 0; i < 4; i++) mv_all[q][i] = lds_ld(&sh_->ref_mv[r][q][i]);
  // With enable_pb_split every inter trial predicts the four quadrants with mv0[0..3] whatever the partition, so a
  // partition whose quadrant vectors equal those of an EARLIER partition has the same prediction, residual, SSD and
  // coefficient bits as that one and strictly more header bits (longer partition code, more vector differences): its
  // cost is not smaller and its evaluation order is later - it can never be selected.  Skipped (exact).
  int dup = 0;
  for (int q = 0; q < part && c.enable_pb_split; q++) {
    int eq = 1;
    for (int i = 0; i < 4; i++) eq = eq && mv_all[q][i].x == mv_all[part][i].x && mv_all[q][i].y == mv_all[part][i].y;
    dup = dup || eq;
  }
  if (tk_uniform(dup)) return;
  BlkParam p = blank_param();
  p.mode = M_INTER;
  p.ref0 = p.ref1 = (int8_t)r;
  p.pb_part = (int8_t)part;
  for (int i = 0; i < 4; i++) { p.mv0[i] = mv_all[part][i]; p.mv1[i] = mv_all[part][i]; }
  for (int tb = -1, have_pred = 0; tb <= max_tb - 1; tb++) {
    p.tb_param = (int8_t)tb;
    have_pred |= par_trial<PIX, SP>(t, J, ws, M, p, 6u + 12u * (unsigned)r + 3u * (unsigned)part + (unsigned)(tb + 1), have_pred);
  }
}

// search_bipred_prediction_params (me_mode 0, PART_NONE) of a P frame with all waves in lock step.  The reference walks
// 2 iterations x {list 1, list 0}; inside one such step it searches EVERY reference against 2*org - pred of the other
// list and keeps the first strictly smaller SAD (encode_block.c:1770-1816).  The searches of one step are independent
// (each touches only its own candidate list), so wave w takes reference w; the leader (wave 0) builds 2*org - pred before
// and reduces in reference order after each step - the very scan of the reference.  Then the two trials (tb 0 / 1).
template <typename PIX, int SP>
TK_DEVNI void bipred_par(const Wg wg, const Team t, JobR<PIX> J, WsP<PIX> ws, MdCtx<PIX>& M) {
  const auto& c = J.cfg;
  WgShared* sh_ = M.sh;
  const auto sh = ldsc(sh_);
  const NodePos nd = node_pos(M.nd);
  const auto lists = ldsc(lds_ld(&ws->mep->lists));
  const int size = nd.size;
  const int num_iter = c.encoder_speed == 0 ? 2 : 1;
  const int max_tb = c.enable_tb_split == 1 ? 2 : 1;
  const mv_t mvp = lds_ld(&sh_->mvp);
  // Round 5: NO leader phase.  Every wave keeps the state of the search (the two lists' best vectors / references, the running minimum) in its
  // own registers - the reduction after a step reads the four waves' results and is the same deterministic scan in every wave - and every wave
  // builds ITS QUARTER of the rows of 2*org - pred straight into the shared buffer (the leader used to predict and subtract the whole block while
  // three waves waited: a third of a step).  Two workgroup barriers per step as before: after the build, after the searches.
  // A step whose inputs - reference and vector of the other list, hence 2*org - pred; and the candidate list of every
  // reference - equal those of the previous step of the same list finds the same SADs again, none of which is below
  // min_sad any more (the earlier step left min_sad <= all of them): it changes nothing and is skipped (about a third of
  // all steps on typical content).  Exact, not a heuristic.
  int prev_ref[2] = {-1, -1}, prev_cnt[2][kMaxRefs];
  mv_t prev_mv[2][4];
  mv_t min0[4], min1[4];
  for (int i = 0; i < 4; i++) { min0[i] = mvp; min1[i] = mvp; }
  int ref0 = 0, ref1 = 0;
  unsigned min_sad = 1u << 30;
  if (wg.wave == 0 && t.rank == 0) sh->bp_org8 = ws->org8;   // the shared 2*org - pred block: wave 0's buffer (visible after the fork barrier? no: published below)
  t.sync();
  wg.barrier();
  PIX* const org8 = (PIX*)sh->bp_org8;   // same address space as this wave's buffers (same block size)
  const int whole = nd.bw == size && nd.bh == size;
  for (int n = 0; n < num_iter; n++)
    for (int list = 1; list >= 0; list--) {
      const int buf = (2 * n + (1 - list)) & 1;   // result slots alternate: a fast wave's next step never overwrites what a slow one still reads
      const mv_t* mo = list ? min0 : min1;
      const int ref_o = list ? ref0 : ref1;
      int same = n > 0 && prev_ref[list] == ref_o;
      for (int i = 0; i < 4; i++) same = same && prev_mv[list][i].x == mo[i].x && prev_mv[list][i].y == mo[i].y;
      for (int r = 0; r < J.num_ref; r++) {
        const int cnt = lists->mvcand_num[r];
        same = same && prev_cnt[list][r] == cnt;
        prev_cnt[list][r] = cnt;
      }
      prev_ref[list] = ref_o;
      for (int i = 0; i < 4; i++) prev_mv[list][i] = mo[i];
      if (tk_uniform(same)) continue;   // the same decision in every wave: all of them read the same counts and hold the same state
      if (whole) {
        // this wave's rows of 2*org - pred (get_inter_prediction_luma of the other list's vector, inter_prediction.c:93-183; encode_block.c:1786-1791)
        const Plane3<PIX> rp = lds_ld(&J.ref[ref_o]);
        const int sgn = J.sign[ref_o];
        const mv_t mvc_ = clip_mv(mo[0], nd.ypos, nd.xpos, c.width, c.height, size, size, sgn);
        const SubPel sp = luma_setup(mvc_, sgn, size, size, c.width, c.height, nd.xpos, nd.ypos, c.enable_bipred);
        const PIX* ry = rp.y + nd.ypos * rp.sy + nd.xpos;
        const int rows = (size + wg.nwaves - 1) / wg.nwaves, r0 = tmin(size, wg.wave * rows), r1 = tmin(size, r0 + rows);   // every row has an owner for any wave count
        const auto o8 = spc<SP>(org8);
        const auto oys = spc<SP>(ws->org_y);
        const int osy = ws->org_sy;
        const Pow2 pw = mk_pow2(size);
        for (int k = r0 * size + t.rank; k < r1 * size; k += t.size) {
          int i, j;
          split2(pw, k, i, j);
          o8[k] = (PIX)sat_pix(2 * (int)oys[i * osy + j] - luma_sample(ry, rp.sy, i, j, sp, c.enable_bipred, c.bitdepth), c.bitdepth);
        }
      } else if (wg.wave == 0) {   // blocks cut by the frame edge: the whole-block path on one wave
        pred_inter_yuv<SP>(t, lds_ld(&J.ref[ref_o]), ws->pred_y, ws->pred_u, ws->pred_v, nd.ypos, nd.xpos, size, nd.bw, nd.bh, mo, J.sign[ref_o], c.width,
                           c.height, c.enable_bipred, 0, c.bitdepth, 1);
        t.sync();
        build_org8<PIX, SP>(t, org8, ws->org_y, ws->org_sy, ws->pred_y, size, c.bitdepth);
      }
      t.sync();
      wg.barrier();   // 2*org - pred is complete
      for (int r = wg.wave; r < J.num_ref; r += wg.nwaves) {
        mv_t mv_all[4];
        const unsigned sad = search_inter<PIX, SP>(t, J, ws, nd.ypos, nd.xpos, size, org8, size, r, lds_ld(&sh_->mv_center[r]), mvp, mv_all, 0, J.sign[r]);
        add_cands4(t, ws, r, mv_all);
        if (t.rank == 0) { sh->bp_sad2[buf][r] = sad; for (int i = 0; i < 4; i++) lds_st(&sh_->bp_mv2[buf][r][i], mv_all[i]); }
      }
      t.sync();
      wg.barrier();   // every reference's result is there
      for (int r = 0; r < J.num_ref; r++) {   // the reference's scan (encode_block.c:1770-1816), in every wave
        const unsigned sd = (unsigned)tk_uniform((int)sh->bp_sad2[buf][r]);
        if (sd < min_sad) {
          min_sad = sd;
          if (list) { ref1 = r; for (int i = 0; i < 4; i++) min1[i] = lds_ld(&sh_->bp_mv2[buf][r][i]); }
          else { ref0 = r; for (int i = 0; i < 4; i++) min0[i] = lds_ld(&sh_->bp_mv2[buf][r][i]); }
        }
      }
    }
  // trials: tb 0 on wave 0, tb 1 on the next wave (each builds its own prediction)
  for (int tb = 0; tb <= max_tb - 1; tb++)
    if (wg.wave == tb % wg.nwaves) {
      BlkParam p = blank_param();
      p.mode = M_BIPRED; p.pb_part = P_NONE;
      p.ref0 = (int8_t)ref0; p.ref1 = (int8_t)ref1;
      for (int i = 0; i < 4; i++) { p.mv0[i] = min0[i]; p.mv1[i] = min1[i]; }
      p.tb_param = (int8_t)tb;
      par_trial<PIX, SP>(t, J, ws, M, p, 54u + (unsigned)tb, 0);
    }
}

// Executed by every wave of the workgroup between the fork and the join barrier.
template <typename PIX, int SP>
TK_MDW void md_worker_sp(const Wg wg, const Team t, JobR<PIX> J, WsP<PIX> ws) {
  WgShared* sh_ = ws->sh;
  const auto sh = ldsc(sh_);
  MdCtx<PIX> M;
  M.wg = wg; M.sh = sh_; M.nd = &sh_->stack[sh->node]; M.mykey = ~0ull;
  if (t.rank == 0) sh->wsnap[wg.wave] = (void*)ws->big;
  const auto ndl = ldsc(M.nd);
  ws_select(ws, tk_uniform(ndl->size));
  org_select(t, J, ws, tk_uniform(ndl->size), ndl->ypos, ndl->xpos, ndl->bw, ndl->bh, 0);
  const auto& c = J.cfg;
  const int max_tb = c.enable_tb_split == 1 ? 2 : 1;
  const int n_items = sh->n_items;
#if TK_PROF_MD
  long long pmd_acc_[4] = {0, 0, 0, 0};
#endif
  for (;;) {
    int i = 0;
    if (t.rank == 0) i = wg_fetch_add(&sh_->next_item, 1);
    i = team_bcast0(t, i);
    if (i >= n_items) break;
    const int kind = team_bcast0(t, sh->items[i].kind), ia = team_bcast0(t, sh->items[i].a), ib = team_bcast0(t, sh->items[i].b);
    TK_PROFMD_MARK(pk_);
    if (kind == MD_SKIP) {
      BlkParam p = blank_param();
      set_cand(p, lds_ld(&M.nd->skip[ia]), ia, M_SKIP);
      par_trial<PIX, SP>(t, J, ws, M, p, (unsigned)ia, 0);
    } else if (kind == MD_MERGE) {
      BlkParam p = blank_param();
      set_cand(p, lds_ld(&M.nd->merge[ia]), ia, M_MERGE);
      for (int tb = 0, have_pred = 0; tb <= max_tb - 1; tb++) {
        p.tb_param = (int8_t)tb;
        have_pred |= par_trial<PIX, SP>(t, J, ws, M, p, 2u + 2u * (unsigned)ia + (unsigned)tb, have_pred);
      }
    } else if (kind == MD_INTRA) {
      BlkParam p = blank_param();
      p.mode = M_INTRA; p.intra_mode = (int8_t)ia; p.tb_param = (int8_t)ib;
      par_trial<PIX, SP>(t, J, ws, M, p, 57u + 2u * (unsigned)ia + (unsigned)ib, 0);
    } else if (kind == MD_REF) {
      md_item_ref<PIX, SP>(t, J, ws, M, ia);
      t.sync();
      int done = 0;
      if (t.rank == 0) done = wg_fetch_add(&sh_->refs_done, 1) + 1;
      done = team_bcast0(t, done);
      if (done == sh->n_ref_items && sh->do_bipred == 1) {
        md_item_bipred<PIX, SP>(t, J, ws, M);
      }
    } else if (kind == MD_TRIAL) {
      md_item_trial<PIX, SP>(t, J, ws, M, ia, ib);
    } else if (kind == MD_BIJOINT) {
      // its first reference's search item left the queue earlier: the PART_NONE vector is there or on its way
      wg_wait_at_least(t, &sh_->parts_done[J.interp_ref ? 1 : 0], 1);
      md_bijoint_telescope<PIX, SP>(t, J, ws, M);
    }
#if TK_PROF_MD
    if (TK_PROFMD_ON(1)) {
      const int slot_ = (kind == MD_SKIP || kind == MD_MERGE) ? 0 : kind == MD_INTRA ? 1 : (kind == MD_REF || kind == MD_BIJOINT) ? 2 : 3;
      if (TK_PROFMD_ON(8)) { const long long d_ = TK_CYC() - pk_; pmd_acc_[0] += slot_ == 0 ? d_ : 0; pmd_acc_[1] += slot_ == 1 ? d_ : 0; pmd_acc_[2] += slot_ == 2 ? d_ : 0; pmd_acc_[3] += slot_ == 3 ? d_ : 0; }
      else TK_PROF_ACC(ws, 16 + slot_, pk_);
    }
#endif
  }
#if TK_PROF_MD
  if (TK_PROFMD_ON(8) && t.rank == 0) for (int q_ = 0; q_ < 4; q_++) ws->prof[16 + q_] += pmd_acc_[q_];
#endif
  if (tk_uniform(sh->do_bipred) == 2) {  // uniform over the workgroup: every wave takes part (same number of barriers); a scalar branch - no
                                         // workgroup barrier behind an exec-masked one (scripts/check_barrier_hazard.py)
    t.sync();
    TK_PROF_MARK(pb_);
    wg.barrier();            // every reference search has finished: mv_center[] and the candidate lists are final
    bipred_par<PIX, SP>(wg, t, J, ws, M);
    TK_PROF_ACC(ws, 27, pb_);
  }
}
// The decision code exists twice: for coding blocks whose sample buffers live in LDS (up to kLdsBlk) and for the larger ones
// (global scratch); see tk_common.h SP_LDS / SP_GLOBAL.
template <typename PIX>
TK_DEV void md_worker(const Wg wg, const Team t, JobR<PIX> J, WsP<PIX> ws) {
  const auto sh = ldsc(ws->sh);
  const int size = tk_uniform(ldsc(&ws->sh->stack[sh->node])->size);
  if (size <= kLdsBlk) md_worker_sp<PIX, SP_LDS>(wg, t, J, ws);
  else md_worker_sp<PIX, SP_GLOBAL>(wg, t, J, ws);
}

// Parked waves: woken by the master at every fork until it posts WG_CMD_EXIT at the end of the superblock.
template <typename PIX>
TK_DEV void wg_helper_loop(const Wg wg, const Team t, JobR<PIX> J, WsP<PIX> ws) {
  for (;;) {
    TK_PROF_MARK(ph_);
    wg.barrier();
    TK_PROF_ACC(ws, 28, ph_);   // parked while the master works alone (quadtree walk, early skip, final encodes)
    const int cmd = team_bcast0(t, ws->sh->cmd);
    if (cmd == WG_CMD_EXIT) { wg.barrier(); break; }  // second barrier: every wave has read the command before the master reuses it
#ifdef THOR_PROF
    { TK_PROF_MARK(pw_); md_worker(wg, t, J, ws); TK_PROF_ACC(ws, 5, pw_); }
#else
    md_worker(wg, t, J, ws);
#endif
    t.sync();
    wg.barrier();
  }
}

// Master side.  Result in nd.best; returns min cost.
template <typename PIX>
TK_MDW unsigned mode_decision_par(const Wg wg, const Team t, JobR<PIX> J, WsP<PIX> ws, int node, int* win_wave) {
  const auto& c = J.cfg;
  WgShared* sh_ = ws->sh;
  const auto sh = ldsc(sh_);
  const auto nd = ldsc(&sh_->stack[node]);
  const int max_tb = c.enable_tb_split == 1 ? 2 : 1;
  const int inter = J.frame_type != F_I;
  TK_PROFMD_MARK(pqs_);
  mv_t mvp = mk_mv(0, 0);
  if (inter) mvp = get_mv_pred(J.cells, J.cell_stride, nd->ypos, nd->xpos, c.width, c.height, nd->size, sb_size_of(c));
  t.sync();
  if (t.rank == 0) {
    int n = 0;
    auto push = [&](int kind, int a, int b) { sh->items[n].kind = (int8_t)kind; sh->items[n].a = (int8_t)a; sh->items[n].b = (int8_t)b; sh->items[n].pad = 0; n++; };
    static_assert(2 + 2 + kMaxRefs + 1 + 2 * kNumIntraModes + 4 * kMaxRefs <= kMdMaxItems, "work queue too small");
    static_assert(6 + 12 * kMaxRefs <= 54, "evaluation-order layout: the reference trials must end before the bi-prediction trials");
    if (inter) {
      for (int k = 0; k < nd->syn.num_skip; k++) push(MD_SKIP, k, 0);
      for (int k = 0; k < nd->syn.num_merge; k++) push(MD_MERGE, k, 0);
      for (int r = 0; r < J.num_ref; r++) push(MD_REF, r, 0);
      if (J.num_ref > 1 && c.enable_bipred && J.frame_type == F_B) push(MD_BIJOINT, 0, 0);   // B frames: telescope of the joint search
      nd->syn.mvp.x = mvp.x; nd->syn.mvp.y = mvp.y;
    }
    for (int m = 0; m < J.num_intra_modes; m++)
      for (int tb = 0; tb <= max_tb - 1; tb++) push(MD_INTRA, m, tb);
    // the trials of the searched vectors come last: by the time the queue gets here most searches have published theirs
    if (inter)
      for (int part = 0; part < (c.enable_pb_split ? 4 : 1); part++)
        for (int r = 0; r < J.num_ref; r++) { push(MD_TRIAL, r, part); sh->parts_done[r] = 0; }
    sh->n_items = n; sh->next_item = 0;
    sh->refs_done = 0; sh->n_ref_items = inter ? J.num_ref : 0;
    sh->do_bipred = (inter && J.num_ref > 1 && c.enable_bipred) ? (J.frame_type == F_P ? 2 : 1) : 0;
    sh->bj_state = 0;
    sh->node = node; lds_st(&sh_->mvp, mvp);
    sh->bestkey = ~0ull;
    for (int w = 0; w < kWaves; w++) sh->wkey[w] = ~0ull;
    sh->cmd = WG_CMD_MD;
  }
  t.sync();
  if (TK_PROFMD_ON(4)) TK_PROFMD_ACC(ws, 21, pqs_);
  wg.barrier();   // fork
#ifdef THOR_PROF
  { TK_PROF_MARK(pw_); md_worker(wg, t, J, ws); TK_PROF_ACC(ws, 5, pw_); t.sync(); wg.barrier(); TK_PROF_ACC(ws, 29, pw_); }
#else
  md_worker(wg, t, J, ws);
  t.sync();
  wg.barrier();   // join
#endif
  unsigned long long best = ~0ull;
  int bw = 0;
  for (int w = 0; w < wg.nwaves; w++) {
    const unsigned long long k = sh->wkey[w];
    if (k < best) { best = k; bw = w; }
  }
  if (best == ~0ull) return kCostInit;
  if (t.rank == 0) lds_st(&sh_->stack[node].best, lds_ld(&sh_->wbest[bw]));
  t.sync();
  *win_wave = bw;
  return (unsigned)(best >> 32);
}
}  // namespace tk
