// tk_block_search.h - the decision's searches: search_inter, add_cands4, build_org8, search_bipred, intra_sad_search.
#pragma once
#include "tk_block_rd.h"

namespace tk {
// search_inter_prediction_params (encode_block.c:1033-1098)
// SP: address space of `org`
template <typename PIX, int SP>
TK_DEV unsigned search_inter(const Team t, JobR<PIX> J, WsP<PIX> ws, int ypos, int xpos, int size,
                             const PIX* org, int ostride, int ref_idx, mv_t mvc, mv_t mvp, mv_t* mv_arr, int part,
                             int sign) {
  const Plane3<PIX> ref = lds_ld(&J.ref[ref_idx]);
  const PIX* ref_y = ref.y + ypos * ref.sy + xpos;
  MeArgs a;
  a.cb_size = size; a.rstride = ref.sy; a.sign = sign; a.fwidth = J.cfg.width; a.fheight = J.cfg.height;
  a.xpos = xpos; a.ypos = ypos; a.enable_bipred = J.cfg.enable_bipred; a.bitdepth = J.cfg.bitdepth;
  a.lam = J.sqrt_lambda; a.ostride = ostride; a.speed = J.cfg.encoder_speed;
  unsigned sad = 0;
  mv_t mv, mvp2 = mvp;
  if (part == P_NONE) {
    a.width = size; a.height = size; a.pu_x = xpos; a.pu_y = ypos;
    sad += motion_estimate<PIX, SP>(t, ws->mep, org, ref_y, a, mvc, mvp2, ref_idx, &mv);
    mv_arr[0] = mv_arr[1] = mv_arr[2] = mv_arr[3] = mv;
  } else if (part == P_HOR) {
    a.width = size; a.height = size / 2;
    for (int index = 0; index < 4; index += 2) {
      int py = index >> 1;
      a.pu_x = xpos; a.pu_y = ypos + py * (size / 2);
      sad += motion_estimate<PIX, SP>(t, ws->mep, org + py * (size / 2) * ostride, ref_y + py * (size / 2) * ref.sy, a, mvc, mvp2, ref_idx, &mv);
      mv_arr[index] = mv; mv_arr[index + 1] = mv;
      mvp2 = mv_arr[0];
    }
  } else if (part == P_VER) {
    a.width = size / 2; a.height = size;
    for (int index = 0; index < 2; index++) {
      a.pu_x = xpos + index * (size / 2); a.pu_y = ypos;
      sad += motion_estimate<PIX, SP>(t, ws->mep, org + index * (size / 2), ref_y + index * (size / 2), a, mvc, mvp2, ref_idx, &mv);
      mv_arr[index] = mv; mv_arr[index + 2] = mv;
      mvp2 = mv_arr[0];
    }
  } else {
    a.width = size / 2; a.height = size / 2;
    for (int index = 0; index < 4; index++) {
      int px = index & 1, py = index >> 1;
      a.pu_x = xpos + px * (size / 2); a.pu_y = ypos + py * (size / 2);
      sad += motion_estimate<PIX, SP>(t, ws->mep, org + py * (size / 2) * ostride + px * (size / 2),
                             ref_y + py * (size / 2) * ref.sy + px * (size / 2), a, mvc, mvp2, ref_idx, &mv);
      mv_arr[index] = mv;
      mvp2 = mv_arr[0];
    }
  }
  return sad;
}

template <typename PIX> TK_DEV void add_cands4(const Team t, WsP<PIX> ws, int ref_idx, const mv_t* mv4) {
  if (t.rank == 0)
    for (int i = 0; i < 4; i++) add_mvcand(ws->mep, ref_idx, mv4[i]);
  t.sync();
}

// 2 * org - pred, saturated (the "original" of a bi-prediction search step, encode_block.c:1786-1791), for a size x size block:
// four samples per lane and step (sample blocks and original rows are aligned to four samples), sample by sample otherwise.
template <typename PIX, int SP>
TK_DEV void build_org8(const Team t, PIX* o8_, const PIX* oy_, int osy, const PIX* py_, int size, int bitdepth) {
#ifndef TK_NOVEC
  const int S = (int)sizeof(PIX);
  const unsigned al = (unsigned)(uintptr_t)o8_ | (unsigned)(uintptr_t)oy_ | (unsigned)(uintptr_t)py_ | (unsigned)(osy * S);
  if (tk_uniform(!(al & (unsigned)(4 * S - 1)))) {
    const int ppr = size >> 2, lg = ilog2((unsigned)ppr);
    for (int k = t.rank; k < ppr * size; k += t.size) {
      const int i = k >> lg, j = (k & (ppr - 1)) << 2;
      int o[4], p[4];
      load_samples<SP, PIX, 4>(oy_ + i * osy + j, o);
      load_samples<SP, PIX, 4>(py_ + i * size + j, p);
      for (int q = 0; q < 4; q++) o[q] = sat_pix(2 * o[q] - p[q], bitdepth);
      store_samples<SP, PIX, 4>(o8_ + i * size + j, o);
    }
    return;
  }
#endif
  const auto o8 = spc<SP>(o8_);
  const auto oys = spc<SP>(oy_);
  const auto pys = spc<SP>(py_);
  for (int k = t.rank; k < size * size; k += t.size) {
    int i, j;
    split2(mk_pow2(size), k, i, j);
    o8[k] = (PIX)sat_pix(2 * (int)oys[i * osy + j] - (int)pys[k], bitdepth);
  }
}

// search_bipred_prediction_params, me_mode 0 (encode_block.c:1739-1832) - P and B frames.
template <typename PIX, int SP>
TK_DEVNI void search_bipred(const Team t, JobR<PIX> J, WsP<PIX> ws, const Node& nd_, int part,
                          const mv_t* mv_center, mv_t mvp, int* ref_idx0, int* ref_idx1, mv_t* mv_arr0, mv_t* mv_arr1) {
  const auto& c = J.cfg;
  const NodePos nd = node_pos(&nd_);
  const auto lists = ldsc(lds_ld(&ws->mep->lists));
  const int size = nd.size;
  const int num_iter = c.encoder_speed == 0 ? 2 : 1;
  int min_ref0 = (J.frame_type == F_B && J.interp_ref > 0) ? 1 : 0, min_ref1 = 0;
  mv_t min0[4], min1[4];
  for (int i = 0; i < 4; i++) { min0[i] = mvp; min1[i] = mvp; }
  unsigned min_sad = 1u << 30;
  const PIX* oy = ws->org_y;
  const int osy = ws->org_sy;
  // a step whose inputs equal those of the previous step of the same list changes nothing (see bipred_par): skipped
  int prev_ref[2] = {-1, -1}, prev_cnt[2][kMaxRefs];
  mv_t prev_mv[2][4];
  for (int n = 0; n < num_iter; n++) {
    const int stop = part == 0 ? 0 : 1;
    for (int list = 1; list >= stop; list--) {
      mv_t mvo = list ? min0[0] : min1[0];
      int ref_o = list ? min_ref0 : min_ref1;
      {
        const mv_t* mo = list ? min0 : min1;
        int same = n > 0 && prev_ref[list] == ref_o;
        for (int i = 0; i < 4; i++) same = same && prev_mv[list][i].x == mo[i].x && prev_mv[list][i].y == mo[i].y;
        for (int r = 0; r < J.num_ref; r++) {
          const int cnt = lists->mvcand_num[r];
          same = same && prev_cnt[list][r] == cnt;
          prev_cnt[list][r] = cnt;
        }
        prev_ref[list] = ref_o;
        for (int i = 0; i < 4; i++) prev_mv[list][i] = mo[i];
        if (tk_uniform(same)) continue;
      }
      pred_inter_yuv<SP>(t, lds_ld(&J.ref[ref_o]), ws->pred_y, ws->pred_u, ws->pred_v, nd.ypos, nd.xpos, size, nd.bw, nd.bh,
                     list ? min0 : min1, J.sign[ref_o], c.width, c.height, c.enable_bipred, part > 0, c.bitdepth, 1);
      t.sync();
      build_org8<PIX, SP>(t, ws->org8, oy, osy, ws->pred_y, size, c.bitdepth);
      t.sync();
      int ref_start, ref_end;
      if (J.frame_type == F_P) { ref_start = 0; ref_end = J.num_ref - 1; }
      else {
        ref_start = ref_end = list ? 1 : 0;
        if (J.interp_ref) { ref_start++; ref_end++; }
      }
      for (int r = ref_start; r <= ref_end; r++) {
        mv_t mvp2 = (J.frame_type == F_B && list == 1) ? mvo : mvp;
        mv_t mv_all[4];
        unsigned sad = search_inter<PIX, SP>(t, J, ws, nd.ypos, nd.xpos, size, ws->org8, size, r, mv_center[r], mvp2, mv_all, part, J.sign[r]);
        add_cands4(t, ws, r, mv_all);
        if (sad < min_sad) {
          min_sad = sad;
          if (list) { min_ref1 = r; for (int i = 0; i < 4; i++) min1[i] = mv_all[i]; }
          else { min_ref0 = r; for (int i = 0; i < 4; i++) min0[i] = mv_all[i]; }
        }
      }
    }
  }
  *ref_idx0 = min_ref0;
  *ref_idx1 = min_ref1;
  for (int i = 0; i < 4; i++) { mv_arr0[i] = min0[i]; mv_arr1[i] = min1[i]; }
}

// search_intra_prediction_params (encode_block.c:928-1031): intra mode by luma SAD against the frame-edge
// prediction; evaluation order DC, HOR, VER, PLANAR (stop here when num_intra_modes == 4), then the six
// angular modes; first minimum wins.  DC is always built from (left, top) here (sic: `xposY >= 0` :953).
template <typename PIX, int SP>
TK_DEVNI unsigned intra_sad_search(const Team t, JobR<PIX> J, WsP<PIX> ws, const Node& nd, int num_modes, int* mode_out) {
  const auto& c = J.cfg;
  const int size = nd.size, bd = c.bitdepth;
  const int ur = upright_avail(nd.ypos, nd.xpos, size, size, c.width, sb_size_of(c));
  const int dl = downleft_avail(nd.ypos, nd.xpos, size, size, c.height, sb_size_of(c));
  const PIX* fy = J.rec.y + nd.ypos * J.rec.sy + nd.xpos;
  const PIX* oy = ws->org_y;
  const int osy = ws->org_sy;
  make_edges<SP>(t, ws->edgep, fy, J.rec.sy, (const PIX*)nullptr, 0, 0, 0, nd.ypos, nd.xpos, size, ur, dl, 0, bd);
  t.sync();
  unsigned min_sad = 1u << 30;
  int best = 0;
  const int n = num_modes == 4 ? 4 : 10;
  for (int e = 0; e < n; e++) {
    const int m = e == 0 ? 0 : e == 1 ? 2 : e == 2 ? 3 : e == 3 ? 1 : e;  // evaluation order -> intra_mode_t
    pred_intra<SP>(t, ws->edgep, 1, 1, size, ws->pred_y, size, m, bd);
    t.sync();
    int local = 0;
    for (int k = t.rank; k < size * size; k += t.size) {
      int i, j;
      split2(mk_pow2(size), k, i, j);
      local += iabs((int)spc<SP>(oy)[i * osy + j] - (int)spc<SP>(ws->pred_y)[k]);
    }
    const unsigned sad = (unsigned)team_sum(t, local) >> (bd - 8);
    t.sync();
    if (sad < min_sad) { min_sad = sad; best = m; }
  }
  *mode_out = best;
  return min_sad;
}
}  // namespace tk
