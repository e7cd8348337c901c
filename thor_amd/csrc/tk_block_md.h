// tk_block_md.h - mode_decision: the sequential block decision (one wave, the reference's trial order).
#pragma once
#include "tk_block_search.h"

namespace tk {
// ---------------------------------------------------------------------------------
// mode_decision_rdo (encode_block.c:1835-2121).  Result in nd.best; returns min cost.
// ---------------------------------------------------------------------------------
template <typename PIX, int SP>
TK_DEVNI unsigned mode_decision(const Team t, JobR<PIX> J, WsP<PIX> ws, Node& nd) {
  const auto& c = J.cfg;
  const int size = nd.size;
  const double lambda = J.lambda;
  const int rect = nd.bw != size || nd.bh != size;
  const int max_tb = c.enable_tb_split == 1 ? 2 : 1;
  const int max_pb = c.enable_pb_split ? 4 : 1;
  unsigned min_cost = kCostInit;
  int do_inter = 1, do_intra = 1;
  BlkParam p;
  // deterministic stand-in for the reference's uninitialised tmp_block_param
  p.mode = M_SKIP; p.intra_mode = 0; p.skip_idx = 0; p.pb_part = P_NONE; p.ref0 = p.ref1 = 0; p.dir = 0;
  p.tb_param = 0; p.tb_split = 0; p.cbp_y = p.cbp_u = p.cbp_v = 0;
  for (int i = 0; i < 4; i++) { p.mv0[i] = mk_mv(0, 0); p.mv1[i] = mk_mv(0, 0); }

  if (J.frame_type != F_I) {
    p.tb_param = 0;
    p.pb_part = P_NONE;
    for (int k = 0; k < nd.syn.num_skip; k++) {
      set_cand(p, nd.skip[k], k, M_SKIP);
      unsigned cost = rdo_trial<PIX, SP>(t, J, ws, nd, p, lambda);
      if (cost < min_cost) { min_cost = cost; if (t.rank == 0) keep_best(nd, p); }
    }
  }
  if ((size < 128 || c.encoder_speed == 0) && !rect) {
    if (J.frame_type != F_I) {
      for (int k = 0; k < nd.syn.num_merge; k++) {
        set_cand(p, nd.merge[k], k, M_MERGE);
        for (int tb = 0; tb <= max_tb - 1; tb++) {
          p.tb_param = (int8_t)tb;
          unsigned cost = rdo_trial<PIX, SP>(t, J, ws, nd, p, lambda, tb > 0, min_cost);
          if (cost < min_cost) { min_cost = cost; if (t.rank == 0) keep_best(nd, p); }
        }
      }
      // encoder_speed > 0: intra-vs-inter pre-decision by SAD (encode_block.c:1943-1947, 1990-1993)
      const int intra_inter_sad = c.encoder_speed > 0;
      unsigned sad_intra = 0xffffffffu;
      if (intra_inter_sad) {
        int im;
        sad_intra = intra_sad_search<PIX, SP>(t, J, ws, nd, J.num_intra_modes, &im);
        sad_intra += (unsigned)(int)mul_add_nofma(J.sqrt_lambda, 2.0, 0.5);
      }
      // uni-prediction per reference
      mv_t mv_center[kMaxRefs];
      mv_t mv_all[4][4];
      mv_t mvp = mk_mv(0, 0);
      const PIX* oy = ws->org_y;
      int min_idx = 0, max_idx = J.num_ref - 1;
      {
        const int br = ws->mep->lists->best_ref;
        if (!(br < 0 || c.encoder_speed < 2 || c.enable_bipred)) min_idx = max_idx = br;
      }
      if (J.frame_type == F_B && J.interp_ref > 2) min_idx = 1;
      unsigned worst_cost = 0, best_cost = 0xffffffffu;
      for (int r = min_idx; r <= max_idx; r++) {
        mvp = get_mv_pred(J.cells, J.cell_stride, nd.ypos, nd.xpos, c.width, c.height, size, sb_size_of(c));
        if (t.rank == 0) add_mvcand(ws->mep, r, mvp);
        t.sync();
        nd.syn.mvp = mvp;
        mv_center[r] = mvp;
        unsigned sad_inter = 0xffffffffu;
        for (int part = 0; part < max_pb; part++) {
          unsigned sad = search_inter<PIX, SP>(t, J, ws, nd.ypos, nd.xpos, size, oy, ws->org_sy, r, mv_center[r], mvp, mv_all[part], part, J.sign[r]);
          add_cands4(t, ws, r, mv_all[part]);
          mv_center[r] = mv_all[0][0];
          sad_inter = sad < sad_inter ? sad : sad_inter;
        }
        if (intra_inter_sad) {
          do_inter = sad_inter < sad_intra;
          if (sad_inter < sad_intra) do_intra = 0;
        }
        if (!do_inter) continue;
        p.mode = M_INTER;
        p.ref0 = p.ref1 = (int8_t)r;
        for (int part = 0; part < max_pb; part++) {
          p.pb_part = (int8_t)part;
          for (int i = 0; i < 4; i++) { p.mv0[i] = mv_all[part][i]; p.mv1[i] = mv_all[part][i]; }
          const int min_tb = c.encoder_speed < 1 ? -1 : 0;
          for (int tb = min_tb; tb <= max_tb - 1; tb++) {
            p.tb_param = (int8_t)tb;
            // worst/best cost feed only the encoder_speed 2 reference shortcut; where that is inactive the
            // exact costs of losing trials are never used and the trial may be pruned
            unsigned cost = rdo_trial<PIX, SP>(t, J, ws, nd, p, lambda, tb > min_tb, (c.encoder_speed < 2 || c.enable_bipred) ? min_cost : 0xffffffffu);
            worst_cost = cost > worst_cost ? cost : worst_cost;
            best_cost = cost < best_cost ? cost : best_cost;
            if (cost < min_cost) { min_cost = cost; if (t.rank == 0) keep_best(nd, p); }
          }
        }
      }
      // "one reference convincingly better": remember reference 0 for the rest of the SB (sic: best_ref_idx
      // is never updated in the reference, encode_block.c:1868/2018-2019); uint32 wrap-around as in C.
      if (worst_cost && worst_cost * 3u > best_cost * 4u) {
        t.sync();
        if (t.rank == 0) ws->mep->lists->best_ref = 0;
        t.sync();
      }
      // bi-prediction
      if (J.num_ref > 1 && c.enable_bipred && do_inter) {
        int r0, r1;
        mv_t a0[4], a1[4];
        search_bipred<PIX, SP>(t, J, ws, nd, 0, mv_center, mvp, &r0, &r1, a0, a1);
        p.mode = M_BIPRED;
        p.pb_part = P_NONE;
        p.ref0 = (int8_t)r0; p.ref1 = (int8_t)r1;
        for (int i = 0; i < 4; i++) { p.mv0[i] = a0[i]; p.mv1[i] = a1[i]; }
        for (int tb = 0; tb <= max_tb - 1; tb++) {
          p.tb_param = (int8_t)tb;
          unsigned cost = rdo_trial<PIX, SP>(t, J, ws, nd, p, lambda, tb > 0, min_cost);
          if (cost < min_cost) { min_cost = cost; if (t.rank == 0) keep_best(nd, p); }
        }
        if (J.frame_type == F_B && c.encoder_speed == 0) {
          // joint +mv / -mv search (search_bipred_prediction_params me_mode 1, encode_block.c:1708-1737, 2052-2068)
          const int ri0 = J.interp_ref ? 1 : 0, ri1 = J.interp_ref ? 2 : 1;
          const Plane3<PIX> f0 = lds_ld(&J.ref[ri0]);
          const Plane3<PIX> f1 = lds_ld(&J.ref[ri1]);
          MeArgs a;
          a.cb_size = size; a.ostride = ws->org_sy; a.width = size; a.height = size; a.rstride = f0.sy; a.sign = 0;
          a.fwidth = c.width; a.fheight = c.height; a.xpos = nd.xpos; a.ypos = nd.ypos; a.enable_bipred = 1;
          a.bitdepth = c.bitdepth; a.lam = J.sqrt_lambda; a.speed = c.encoder_speed; a.pu_x = nd.xpos; a.pu_y = nd.ypos;
          mv_t mvb;
          motion_estimate_bi<PIX, SP>(t, ws->mep, oy, f0.y + nd.ypos * f0.sy + nd.xpos, f1.y + nd.ypos * f1.sy + nd.xpos, a, mv_center[ri0],
                             mvp, ri0, &mvb);
          p.mode = M_BIPRED;
          p.pb_part = P_NONE;
          p.ref0 = (int8_t)ri0; p.ref1 = (int8_t)ri1;
          for (int i = 0; i < 4; i++) { p.mv0[i] = mvb; p.mv1[i] = mvb; }
          p.tb_param = 0;
          unsigned cost = rdo_trial<PIX, SP>(t, J, ws, nd, p, lambda);
          if (cost < min_cost) { min_cost = cost; if (t.rank == 0) keep_best(nd, p); }
        }
      }
    }
    // intra (encode_block.c:2070-2114).  The reference re-encodes the winning mode for both
    // tb_param values after the search; those trials are repeats of trials already made (same inputs,
    // deterministic), so their costs are taken from the search instead of being recomputed.
    p.mode = M_INTRA;
    int intra_mode = 0;
    unsigned best_tb_cost[2] = {kCostInit, kCostInit};
    if (!do_intra) {
    } else if (c.intra_rdo) {
      unsigned min_intra = kCostInit;
      for (int m = 0; m < J.num_intra_modes; m++) {
        p.intra_mode = (int8_t)m;
        unsigned tbc[2] = {kCostInit, kCostInit};
        int improved = 0;
        for (int tb = 0; tb <= max_tb - 1; tb++) {
          p.tb_param = (int8_t)tb;
          // only a cost below both the best intra cost and the best overall cost can change the outcome
          unsigned cost = rdo_trial<PIX, SP>(t, J, ws, nd, p, lambda, 0, min_intra < min_cost ? min_intra : min_cost);
          tbc[tb] = cost;
          if (cost < min_intra) { min_intra = cost; intra_mode = m; improved = 1; }
        }
        if (improved) { best_tb_cost[0] = tbc[0]; best_tb_cost[1] = tbc[1]; }
      }
      p.intra_mode = (int8_t)intra_mode;
      for (int tb = 0; tb <= max_tb - 1; tb++) {
        p.tb_param = (int8_t)tb;
        unsigned cost = best_tb_cost[tb];
        if (cost < min_cost) { min_cost = cost; p.cbp_y = p.cbp_u = p.cbp_v = 0; if (t.rank == 0) keep_best(nd, p); }
      }
    } else {
      intra_sad_search<PIX, SP>(t, J, ws, nd, J.num_intra_modes, &intra_mode);
      p.intra_mode = (int8_t)intra_mode;
      for (int tb = 0; tb <= max_tb - 1; tb++) {
        p.tb_param = (int8_t)tb;
        unsigned cost = rdo_trial<PIX, SP>(t, J, ws, nd, p, lambda);
        if (cost < min_cost) { min_cost = cost; if (t.rank == 0) keep_best(nd, p); }
      }
    }
  }
  return min_cost;
}
}  // namespace tk
