// tk_block_rd.h - rate-distortion core: ssd_*, rd_cost, improve_uv, predict_inter, PruneCtx, code_inter_plane, encode_block, rdo_trial, keep_best.
#pragma once
#include "tk_block_ctx.h"

namespace tk {
// ---------------------------------------------------------------------------------
// SSD / cost
// ---------------------------------------------------------------------------------
// Sum of squared differences of two sample blocks, kept in registers: ssd_part() is this lane's share (8-bit samples: at most
// 256 samples x 255^2 per lane and 1.6e9 for the three planes of a 128x128 block - 32-bit arithmetic; 64-bit for 16-bit
// samples), ssd_total() the wave-wide sum - one DPP reduction per cost instead of an LDS accumulator round trip per plane.
// SP: address space of both sample blocks.
template <typename PIX> struct SsdT { typedef unsigned long long type; };
template <> struct SsdT<uint8_t> { typedef unsigned type; };
// 8-bit samples, four at a time: sum (a-b)^2 = sum a^2 + sum b^2 - 2 sum ab as three packed dot products (v_dot4_u32_u8) on the
// dwords as loaded; the partial sums wrap modulo 2^32 and the difference is exact (the true value fits, see above).
TK_DEV unsigned udot4_u8(unsigned a, unsigned b, unsigned c) {
#if TK_HOST
  for (int k = 0; k < 4; k++) c += ((a >> (8 * k)) & 0xffu) * ((b >> (8 * k)) & 0xffu);
  return c;
#else
  return __builtin_amdgcn_udot4(a, b, c, false);
#endif
}
TK_DEV unsigned udot2_u16(unsigned a, unsigned b, unsigned c) {
#if TK_HOST
  return c + (a & 0xffffu) * (b & 0xffffu) + (a >> 16) * (b >> 16);
#else
  typedef unsigned short __attribute__((ext_vector_type(2))) u16x2;
  u16x2 x, y;
  __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &b, 4);
  return __builtin_amdgcn_udot2(x, y, c, false);
#endif
}
// NW dwords per lane and step (4 * NW 8-bit or 2 * NW 16-bit samples); rows and pointers aligned to 4 * NW bytes.  16-bit samples (up
// to 12 bits): a lane's share is at most 256 samples x 4095^2 < 2^32, so the same modular arithmetic is exact.
template <int SP, typename PIX, int NW> TK_DEV unsigned ssd_rows(const Team t, const PIX* a_, int as, const PIX* b_, int bs, int w, int h) {
  const int spp = 4 * NW / (int)sizeof(PIX);   // samples per piece
  const int ppr = w / spp;
  const int lg = (ppr & (ppr - 1)) ? -1 : ilog2((unsigned)ppr);
  unsigned sq = 0, ab = 0;
  for (int k = t.rank; k < ppr * h; k += t.size) {
    int i, j;
    if (lg >= 0) { i = k >> lg; j = k & (ppr - 1); } else { i = k / ppr; j = k - i * ppr; }
    uint32_t x[NW], y[NW];
#if TK_HOST
    __builtin_memcpy(x, a_ + i * as + j * spp, 4 * NW);
    __builtin_memcpy(y, b_ + i * bs + j * spp, 4 * NW);
#else
    typedef uint32_t __attribute__((ext_vector_type(NW))) vec_t;
    const vec_t xv = *(typename SpT<SP, const vec_t>::ptr)(spc<SP>(a_) + i * as + j * spp);
    const vec_t yv = *(typename SpT<SP, const vec_t>::ptr)(spc<SP>(b_) + i * bs + j * spp);
    __builtin_memcpy(x, &xv, 4 * NW);
    __builtin_memcpy(y, &yv, 4 * NW);
#endif
    TK_UNROLL
    for (int q = 0; q < NW; q++) {
      if constexpr (sizeof(PIX) == 1) { sq = udot4_u8(x[q], x[q], udot4_u8(y[q], y[q], sq)); ab = udot4_u8(x[q], y[q], ab); }
      else { sq = udot2_u16(x[q], x[q], udot2_u16(y[q], y[q], sq)); ab = udot2_u16(x[q], y[q], ab); }
    }
  }
  return sq - 2u * ab;
}
template <int SP, typename PIX>
TK_DEV typename SsdT<PIX>::type ssd_part(const Team t, const PIX* a_, int as, const PIX* b_, int bs, int w, int h) {
  a_ = tk_uniform_ptr(a_); b_ = tk_uniform_ptr(b_); as = tk_uniform(as); bs = tk_uniform(bs); w = tk_uniform(w); h = tk_uniform(h);
#ifndef TK_NOVEC
  // (host simulation with teams smaller than a wavefront: a lane's share of a large block of 16-bit samples can exceed the 256 samples for
  // which the modular 32-bit sums of ssd_rows are exact - such blocks take the 64-bit sample loop below)
  if (!(TK_HOST && sizeof(PIX) == 2 && (w * h) / t.size > 256)) {
    const int S = (int)sizeof(PIX);
    const unsigned al = (unsigned)(uintptr_t)a_ | (unsigned)(uintptr_t)b_ | (unsigned)(as * S) | (unsigned)(bs * S) | (unsigned)(w * S);
    if (!(al & 15u)) return ssd_rows<SP, PIX, 4>(t, a_, as, b_, bs, w, h);
    if (!(al & 7u)) return ssd_rows<SP, PIX, 2>(t, a_, as, b_, bs, w, h);
    if (!(al & 3u)) return ssd_rows<SP, PIX, 1>(t, a_, as, b_, bs, w, h);
  }
#endif
  const auto a = spc<SP>(a_);
  const auto b = spc<SP>(b_);
  typename SsdT<PIX>::type local = 0;
  if ((w & (w - 1)) == 0) {  // every width except the frame-edge rectangles
    const Pow2 pw = mk_pow2(w);
    for (int k = t.rank; k < w * h; k += t.size) {
      int i, j;
      split2(pw, k, i, j);
      int d = (int)a[i * as + j] - (int)b[i * bs + j];
      local += (typename SsdT<PIX>::type)(d * d);
    }
  } else {
    for (int k = t.rank; k < w * h; k += t.size) {
      int i = k / w, j = k - i * w;
      int d = (int)a[i * as + j] - (int)b[i * bs + j];
      local += (typename SsdT<PIX>::type)(d * d);
    }
  }
  return local;
}
TK_DEV unsigned long long ssd_total(const Team t, unsigned v) { return (unsigned long long)(unsigned)team_sum(t, (int)v); }
TK_DEV unsigned long long ssd_total(const Team t, unsigned long long v) { return team_sum64(t, v); }

// cost_calc (encode_block.c:916-926) on the trial recon in ws->rec_* vs. the original frame.
template <typename PIX, int SP>
TK_DEVNI unsigned rd_cost(const Team t, JobR<PIX> J, WsP<PIX> ws, const Node& nd_, int nbits, double lambda,
                         long long ssd_y = -1) {
  TK_PROF_T0();
  const auto nd = ldsc(&nd_);
  const int size = TKU(nd->size), bw = TKU(nd->bw), bh = TKU(nd->bh);
  const int sc = size >> 1;
  typename SsdT<PIX>::type part = 0;
  if (ssd_y < 0) part += ssd_part<SP>(t, ws->org_y, ws->org_sy, ws->rec_y, size, bw, bh);
  part += ssd_part<SP>(t, ws->org_u, ws->org_sc, ws->rec_u, sc, bw >> 1, bh >> 1);
  part += ssd_part<SP>(t, ws->org_v, ws->org_sc, ws->rec_v, sc, bw >> 1, bh >> 1);
  const unsigned long long ssd = ssd_total(t, part) + (ssd_y >= 0 ? (unsigned long long)ssd_y : 0ull);
  unsigned long long cost = (ssd >> (J.cfg.bitdepth * 2 - 16)) + (unsigned long long)(long long)mul_add_nofma(lambda, (double)nbits, 0.5);
  if (cost > (1ull << 30)) cost = 1ull << 30;
  TK_PROF_ADD(ws, PF_COST);
  return (unsigned)cost;
}

// ---------------------------------------------------------------------------------
// Chroma-from-luma (common_block.c:347-428).  y: luma prediction (stride n), u/v: chroma
// prediction (stride cstride>>1), ry: reconstructed luma (stride `stride`), n = luma size.
// ---------------------------------------------------------------------------------
template <typename PIX, int SP>
TK_DEVNI void improve_uv(const Team t, WsP<PIX> ws, const PIX* y_, PIX* u_, PIX* v_, const PIX* ry_, int n, int cstride,
                       int stride, int bitdepth) {
  const auto y = spc<SP>(y_); const auto u = spc<SP>(u_); const auto v = spc<SP>(v_); const auto ry = spc<SP>(ry_);
  (void)ws;
  const int nc = n >> 1, lognc = ilog2(nc), cs = cstride >> 1;
  long long tot8[8];
  typedef typename SsdT<PIX>::type sum_t;   // 32-bit sums for 8-bit samples (at most 4096 x 255^2 per sum), 64-bit otherwise
  long long sq;
  {
    sum_t local = 0;
    for (int k = t.rank; k < n * n; k += t.size) {
      int i, j;
      split2(mk_pow2(n), k, i, j);
      int d = (int)ry[i * stride + j] - (int)y[i * n + j];
      local += (sum_t)(d * d);
    }
    sq = (long long)ssd_total(t, local);
  }
  if ((sq >> (2 * ilog2(n))) <= (64ll << (2 * (bitdepth - 8)))) { t.sync(); return; }
  {
    sum_t ls[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = t.rank; k < nc * nc; k += t.size) {
      int i, j;
      split2(mk_pow2(nc), k, i, j);
      int us = u[i * cs + j], vs = v[i * cs + j];
      int ys = (y[(i * 2) * n + j * 2] + y[(i * 2) * n + j * 2 + 1] + y[(i * 2 + 1) * n + j * 2] + y[(i * 2 + 1) * n + j * 2 + 1] + 2) >> 2;
      ls[0] += ys; ls[1] += us; ls[2] += vs;
      ls[3] += (unsigned)(ys * ys); ls[4] += (unsigned)(ys * us); ls[5] += (unsigned)(ys * vs);
      ls[6] += (unsigned)(us * us); ls[7] += (unsigned)(vs * vs);
    }
    for (int q = 0; q < 8; q++) ls[q] = (sum_t)ssd_total(t, ls[q]);
    tot8[0] = (long long)ls[0]; tot8[1] = (long long)ls[1]; tot8[2] = (long long)ls[2]; tot8[3] = (long long)ls[3];
    tot8[4] = (long long)ls[4]; tot8[5] = (long long)ls[5]; tot8[6] = (long long)ls[6]; tot8[7] = (long long)ls[7];
  }
  const long long ysum = tot8[0], usum = tot8[1], vsum = tot8[2], yysum = tot8[3], yusum = tot8[4],
                  yvsum = tot8[5], uusum = tot8[6], vvsum = tot8[7];
  const long long ssyy = yysum - ((ysum * ysum) >> (lognc * 2));
  const long long ssuu = uusum - ((usum * usum) >> (lognc * 2));
  const long long ssvv = vvsum - ((vsum * vsum) >> (lognc * 2));
  const long long ssyu = yusum - ((ysum * usum) >> (lognc * 2));
  const long long ssyv = yvsum - ((ysum * vsum) >> (lognc * 2));
  if (!ssyy) return;
  for (int pl = 0; pl < 2; pl++) {
    const long long ssyc = pl ? ssyv : ssyu, sscc = pl ? ssvv : ssuu, csum = pl ? vsum : usum;
    const auto c = pl ? v : u;
    if (ssyc * ssyc * 2 > ssyy * sscc) {
      long long a64 = (ssyc << 16) / ssyy;
      long long b64 = ((csum << 16) - a64 * ysum) >> (lognc * 2);
      const long long alim = 1ll << (31 - bitdepth);
      int a = (int)(a64 < -alim ? -alim : (a64 > alim ? alim : a64));
      long long bb = b64 + (1 << 15);
      int b = (int)(bb < -(1ll << 31) ? -(1ll << 31) : (bb > ((1ll << 31) - 1) ? ((1ll << 31) - 1) : bb));
      for (int k = t.rank; k < nc * nc; k += t.size) {
        int i, j;
        split2(mk_pow2(nc), k, i, j);
        int s = 2;
        for (int q = 0; q < 4; q++) {
          int r = ry[(i * 2 + (q >> 1)) * stride + j * 2 + (q & 1)];
          int m = (int)((unsigned)a * (unsigned)r + (unsigned)b);  // wraps like the reference's int arithmetic
          s += sat_pix(m >> 16, bitdepth);
        }
        c[i * cs + j] = (PIX)(s >> 2);
      }
    }
  }
  t.sync();
}

// ---------------------------------------------------------------------------------
// encode_block (encode_block.c:1340-1514): prediction + residual coding of one CB into the trial
// buffers ws->rec_* / ws->coef_*; returns the number of bits of write_block.  `bs` counts or emits.
// ---------------------------------------------------------------------------------
template <typename PIX, int SP>
TK_DEV void predict_inter(const Team t, JobR<PIX> J, WsP<PIX> ws, const Node& nd_, const BlkParam& p,
                          int split) {
  const auto ndl = ldsc(&nd_);
  struct { int ypos, xpos, size, bw, bh; } nd = {TKU(ndl->ypos), TKU(ndl->xpos), TKU(ndl->size), TKU(ndl->bw), TKU(ndl->bh)};
  TK_PROF_T0();
  const auto& c = J.cfg;
  const int bi = (p.mode == M_BIPRED) || ((p.mode == M_SKIP || p.mode == M_MERGE) && p.dir == 2);
  if (bi) {
    pred_inter_yuv<SP>(t, lds_ld(&J.ref[p.ref0]), ws->p0_y, ws->p0_u, ws->p0_v, nd.ypos, nd.xpos, nd.size, nd.bw, nd.bh, p.mv0,
                   J.sign[p.ref0], c.width, c.height, c.enable_bipred, split, c.bitdepth);
    pred_inter_yuv<SP>(t, lds_ld(&J.ref[p.ref1]), ws->p1_y, ws->p1_u, ws->p1_v, nd.ypos, nd.xpos, nd.size, nd.bw, nd.bh, p.mv1,
                   J.sign[p.ref1], c.width, c.height, c.enable_bipred, split, c.bitdepth);
    t.sync();
    average_yuv<SP>(t, ws->pred_y, ws->pred_u, ws->pred_v, ws->p0_y, ws->p0_u, ws->p0_v, ws->p1_y, ws->p1_u, ws->p1_v,
                nd.size, nd.bw, nd.bh);
  } else {
    pred_inter_yuv<SP>(t, lds_ld(&J.ref[p.ref0]), ws->pred_y, ws->pred_u, ws->pred_v, nd.ypos, nd.xpos, nd.size, nd.bw, nd.bh,
                   p.mv0, J.sign[p.ref0], c.width, c.height, c.enable_bipred, split, c.bitdepth);
  }
  t.sync();
  TK_PROF_ADD(ws, PF_PRED_INTER);
}

// Exact partial-cost pruning of RDO trials.  A trial only matters if its cost is below a threshold the caller
// knows (the best cost so far; for the intra search also the best intra cost so far - strict '<' everywhere in
// mode_decision_rdo).  cost = SSD_Y + SSD_U + SSD_V + (unsigned)(lambda * bits + 0.5) is monotone in every
// term, so once the luma planes are coded, SSD_Y + (unsigned)(lambda * luma coefficient bits + 0.5) is a lower
// bound of the final cost: if it already reaches the threshold the chroma transform units, CfL, the bit count
// and the cost evaluation are skipped and the trial is reported as "not better" - results are unchanged.
// Parallel decision (mode_decision_par): the trials of one block run on several wavefronts in no particular order,
// so the threshold is the shared minimum over all FINISHED trials of the key (cost << 32 | evaluation order) - the
// winner is the trial with the smallest key, which is exactly the reference's "first strictly smaller cost in
// evaluation order".  A trial whose lower-bound key (lb << 32 | its order) already exceeds that minimum cannot have
// the smallest key, whatever the timing: pruning stays exact and only the amount of skipped work varies.
struct PruneCtx {
  unsigned thr;       // prune when the lower bound is >= thr (0xffffffff: never)
  const unsigned long long* bestkey;  // parallel decision: shared minimum key (nullptr: use thr)
  unsigned order;                     // evaluation order of this trial
  double lambda;
  long long ssd_y;    // out: luma SSD of the trial (reused by rd_cost), -1 if not computed
  int ybits[4];       // out: luma coefficient bits per TU
  int have_ybits;
  int pruned;         // out
  long long ssd_part; // tb-split luma: SSD / bits of the quadrants coded so far
  int bits_part;
  int head_bits;      // bits of the trial that do not depend on its residual (tk_bits.h:bs_block_head_t): part of every bound
};

// tb-split luma: call after quadrant `tu` (0..3, size s2 at (i,j) of the block) has been coded.  The first three
// quadrants give an early lower bound; after the fourth the accumulated values are the block's luma SSD / bits.
TK_DEV int prune_active(const PruneCtx* pc) { return pc && (pc->bestkey || pc->thr != 0xffffffffu); }
TK_DEV int prune_hit(const PruneCtx* pc, unsigned long long lb) {
  if (pc->bestkey) return ((lb << 32) | (unsigned long long)pc->order) > wg_load64(pc->bestkey);
  return lb >= (unsigned long long)pc->thr;
}

template <typename PIX, int SP>
TK_DEV int prune_after_quadrant(const Team t, JobR<PIX> J, WsP<PIX> ws, int nd_size, int intra, int tu, int i, int j,
                                int s2, int bit, const int16_t* coef, PruneCtx* pc) {
  if (!prune_active(pc)) return 0;
  t.sync();
  pc->ssd_part += (long long)ssd_total(t, ssd_part<SP>(t, ws->org_y + i * ws->org_sy + j, ws->org_sy, ws->rec_y + i * nd_size + j, nd_size, s2, s2));
  pc->ybits[tu] = bit ? coeff_bits_team<SP_LDS>(t, coef, s2, intra << 1) : 0;  // luma coefficients: always SmallWs (LDS)
  pc->bits_part += pc->ybits[tu];
  if (tu == 3) { pc->ssd_y = pc->ssd_part; pc->have_ybits = 1; }
  unsigned long long lb = ((unsigned long long)pc->ssd_part >> (J.cfg.bitdepth * 2 - 16)) + (unsigned long long)(long long)mul_add_nofma(pc->lambda, (double)(pc->bits_part + pc->head_bits), 0.5);
  if (lb > (1ull << 30)) lb = 1ull << 30;
#if TK_HOST
  { extern long long g_prune_stat[8]; g_prune_stat[4] += 1; if (prune_hit(pc, lb)) g_prune_stat[5 + (tu == 3)] += 1; }
#endif
  if (team_bcast0(t, prune_hit(pc, lb))) { pc->pruned = 1; return 1; }  // one lane's reading decides for the wave
  return 0;
}

template <typename PIX, int SP>
TK_DEV int prune_after_luma(const Team t, JobR<PIX> J, WsP<PIX> ws, int size, int bw, int bh, const BlkParam& p, int cbp_y,
                            int tb_split, PruneCtx* pc) {
  if (!prune_active(pc)) return 0;
  if (pc->pruned) return 1;
  if (pc->have_ybits) return 0;  // tb-split luma: bound already evaluated quadrant by quadrant
  t.sync();
  const unsigned long long ssd = ssd_total(t, ssd_part<SP>(t, ws->org_y, ws->org_sy, ws->rec_y, size, bw, bh));
  pc->ssd_y = (long long)ssd;
  const int coeff_type = (p.mode == M_INTRA) << 1;
  int bits = 0;
  if (!tb_split) {
    pc->ybits[0] = cbp_y ? coeff_bits_team<SP_LDS>(t, ws->coef_y, size, coeff_type) : 0;
    bits = pc->ybits[0];
  } else {
    const int qy = size / 2 < kMaxQuant ? size / 2 : kMaxQuant;
    for (int tu = 0; tu < 4; tu++) {
      pc->ybits[tu] = ((cbp_y >> (3 - tu)) & 1) ? coeff_bits_team<SP_LDS>(t, ws->coef_y + tu * qy * qy, size / 2, coeff_type) : 0;
      bits += pc->ybits[tu];
    }
  }
  pc->have_ybits = 1;
  unsigned long long lb = (ssd >> (J.cfg.bitdepth * 2 - 16)) + (unsigned long long)(long long)mul_add_nofma(pc->lambda, (double)(bits + pc->head_bits), 0.5);
  if (lb > (1ull << 30)) lb = 1ull << 30;
#if TK_HOST
  { extern long long g_prune_stat[8]; g_prune_stat[p.mode == M_INTRA ? 0 : 2] += 1; if (prune_hit(pc, lb)) g_prune_stat[p.mode == M_INTRA ? 1 : 3] += 1; }
#endif
  if (team_bcast0(t, prune_hit(pc, lb))) { pc->pruned = 1; return 1; }  // one lane's reading decides for the wave
  return 0;
}

// residual coding of one plane of an inter block (encode_and_reconstruct_block_inter :1275-1338)
// SP: address space of org / pred / rec, SC: of coef.  nd_size > 0: luma plane of a block of that size with pruning context pc.
template <typename PIX, int SP, int SC>
TK_DEV int code_inter_plane(const Team t, JobR<PIX> J, WsP<PIX> ws, const PIX* org, int ostride,
                            const PIX* pred, PIX* rec, int size, int qp, int coeff_type, int tb_split, int16_t* coef,
                            int nd_size = 0, PruneCtx* pc = nullptr) {
  const int bd = J.cfg.bitdepth;
  if (!tb_split) {
    int fast = (size == 64 && J.cfg.encoder_speed > 0) || J.cfg.encoder_speed > 1;
    return code_tu_sp<PIX, SP, SC>(t, ws->xfp, org, ostride, pred, size, rec, size, size, qp, coeff_type, fast, coef, bd);
  }
  const int s2 = size / 2;
  int cbp = 0, index = 0;
  for (int i = 0; i < size; i += s2)
    for (int j = 0; j < size; j += s2) {
      int fast = size == 64 || J.cfg.encoder_speed > 1;
      int bit = code_tu_sp<PIX, SP, SC>(t, ws->xfp, org + i * ostride + j, ostride, pred + i * size + j, size, rec + i * size + j, size,
                        s2, qp, coeff_type, fast, coef + index, bd);
      cbp = (cbp << 1) + bit;
      if (nd_size && prune_after_quadrant<PIX, SP>(t, J, ws, nd_size, 0, (i ? 2 : 0) + (j ? 1 : 0), i, j, s2, bit, coef + index, pc)) return cbp;
      index += tmin(s2, 16) * tmin(s2, 16);
    }
  return cbp;
}

// reuse_pred: the inter prediction of this (mode, refs, MVs) is already in ws->pred_* (previous trial
// of the same candidate with another tb_param) - exact, the prediction does not depend on tb_param.
// reuse_pred == 2: the caller vouches that ws->pred_* holds the prediction untouched (no CfL pass has refined its chroma).
// SP: address space of the coding block's sample buffers and original samples (SP_LDS for blocks up to kLdsBlk).
template <typename PIX, int SP>
TK_DEVNI int encode_block(const Team t, JobR<PIX> J, WsP<PIX> ws, Node& nd_, BlkParam& p, BitSink& bs,
                          int reuse_pred = 0, PruneCtx* pc = nullptr) {
  const auto& c = J.cfg;
  const NodePos nd = node_pos(&nd_);
  const int size = nd.size, sizeC = size >> 1;
  const int yc = nd.ypos >> 1, xc = nd.xpos >> 1;
  const int qpY = TKU(J.qp), qpC = TK_TAB.chroma_qp[qpY];
  const int tb_split = TKU(p.tb_param) > 0 ? TKU(p.tb_param) : 0;
  const int zero_block = TKU(p.tb_param) == -1;
  const int ftI = (TKU(J.frame_type) == F_I) << 1;
  const int bd = TKU(c.bitdepth);
  p.tb_split = (int8_t)tb_split;
  // chroma coefficients: SmallWs (LDS) except the 4 x 16x16 units of tb-split 64 / 128 blocks (global scratch)
  const int bigc = SP == SP_GLOBAL && tb_split && sizeC >= 32;
  ws->coef_u = bigc ? ws->coef_u_big : ws->coef_u_small;
  ws->coef_v = bigc ? ws->coef_v_big : ws->coef_v_small;
  const PIX* oy = ws->org_y;
  const PIX* ou = ws->org_u;
  const PIX* ov = ws->org_v;
  const int osy = TKU(ws->org_sy), osc = TKU(ws->org_sc);
  int cbp_y = 0, cbp_u = 0, cbp_v = 0;

  if (TKU(p.mode) == M_INTRA) {
    const int ur = upright_avail(nd.ypos, nd.xpos, size, size, c.width, sb_size_of(c));
    const int dl = downleft_avail(nd.ypos, nd.xpos, size, size, c.height, sb_size_of(c));
    const PIX* fy = J.rec.y + nd.ypos * J.rec.sy + nd.xpos;
    const PIX* fu = J.rec.u + yc * J.rec.sc + xc;
    const PIX* fv = J.rec.v + yc * J.rec.sc + xc;
    // luma (encode_and_reconstruct_block_intra :1100-1168)
    if (tb_split) {
      const int s2 = size / 2;
      int index = 0;
      for (int i = 0; i < size; i += s2)
        for (int j = 0; j < size; j += s2) {
          make_edges<SP>(t, ws->edgep, fy, J.rec.sy, ws->rec_y + i * size + j, size, i, j, nd.ypos, nd.xpos, s2, ur, dl, 1, bd);
          pred_intra<SP>(t, ws->edgep, nd.ypos + i, nd.xpos + j, s2, ws->pred_y + i * size + j, size, p.intra_mode, bd);
          t.sync();
          int bit = code_tu_sp<PIX, SP, SP_LDS>(t, ws->xfp, oy + i * osy + j, osy, ws->pred_y + i * size + j, size,
                            ws->rec_y + i * size + j, size, s2, qpY, ftI | 0, c.encoder_speed > 1, ws->coef_y + index, bd);
          cbp_y = (cbp_y << 1) + bit;
          if (prune_after_quadrant<PIX, SP>(t, J, ws, size, 1, (i ? 2 : 0) + (j ? 1 : 0), i, j, s2, bit, ws->coef_y + index, pc)) return 0;
          index += tmin(s2, 16) * tmin(s2, 16);
        }
    } else {
      make_edges<SP>(t, ws->edgep, fy, J.rec.sy, (const PIX*)nullptr, 0, 0, 0, nd.ypos, nd.xpos, size, ur, dl, 0, bd);
      pred_intra<SP>(t, ws->edgep, nd.ypos, nd.xpos, size, ws->pred_y, size, p.intra_mode, bd);
      t.sync();
      cbp_y = code_tu_sp<PIX, SP, SP_LDS>(t, ws->xfp, oy, osy, ws->pred_y, size, ws->rec_y, size, size, qpY, ftI | 0,
                      c.encoder_speed > 1, ws->coef_y, bd);
    }
    if (prune_after_luma<PIX, SP>(t, J, ws, size, nd.bw, nd.bh, p, cbp_y, tb_split, pc)) return 0;
    // chroma (encode_and_reconstruct_block_intra_uv :1170-1273)
    const int csplit = tb_split && sizeC > 4;
    if (csplit) {
      const int s2 = sizeC / 2;
      int index = 0;
      for (int i = 0; i < sizeC; i += s2)
        for (int j = 0; j < sizeC; j += s2) {
          make_edges<SP>(t, ws->edgep, fu, J.rec.sc, ws->rec_u + i * sizeC + j, sizeC, i, j, yc, xc, s2, ur, dl, 1, bd);
          pred_intra<SP>(t, ws->edgep, yc + i, xc + j, s2, ws->pred_u + i * sizeC + j, sizeC, p.intra_mode, bd);
          t.sync();
          make_edges<SP>(t, ws->edgep, fv, J.rec.sc, ws->rec_v + i * sizeC + j, sizeC, i, j, yc, xc, s2, ur, dl, 1, bd);
          pred_intra<SP>(t, ws->edgep, yc + i, xc + j, s2, ws->pred_v + i * sizeC + j, sizeC, p.intra_mode, bd);
          t.sync();
          if (c.cfl_intra)  // sic: luma pointers offset in CHROMA units (encode_block.c:1199)
            improve_uv<PIX, SP>(t, ws, ws->pred_y + i * sizeC + j, ws->pred_u + i * sizeC + j, ws->pred_v + i * sizeC + j,
                       ws->rec_y + (i << 1) * size + (j << 1), s2 << 1, sizeC << 1, size, bd);
          int bu, bv;
          if (bigc) {
            bu = code_tu_sp<PIX, SP, SP_GLOBAL>(t, ws->xfp, ou + i * osc + j, osc, ws->pred_u + i * sizeC + j, sizeC,
                             ws->rec_u + i * sizeC + j, sizeC, s2, qpC, ftI | 1, c.encoder_speed > 1, ws->coef_u + index, bd);
            bv = code_tu_sp<PIX, SP, SP_GLOBAL>(t, ws->xfp, ov + i * osc + j, osc, ws->pred_v + i * sizeC + j, sizeC,
                             ws->rec_v + i * sizeC + j, sizeC, s2, qpC, ftI | 1, c.encoder_speed > 1, ws->coef_v + index, bd);
          } else {
            bu = code_tu_sp<PIX, SP, SP_LDS>(t, ws->xfp, ou + i * osc + j, osc, ws->pred_u + i * sizeC + j, sizeC,
                             ws->rec_u + i * sizeC + j, sizeC, s2, qpC, ftI | 1, c.encoder_speed > 1, ws->coef_u + index, bd);
            bv = code_tu_sp<PIX, SP, SP_LDS>(t, ws->xfp, ov + i * osc + j, osc, ws->pred_v + i * sizeC + j, sizeC,
                             ws->rec_v + i * sizeC + j, sizeC, s2, qpC, ftI | 1, c.encoder_speed > 1, ws->coef_v + index, bd);
          }
          cbp_u = (cbp_u << 1) + bu;
          cbp_v = (cbp_v << 1) + bv;
          index += tmin(s2, 16) * tmin(s2, 16);
        }
    } else {
      make_edges<SP>(t, ws->edgep, fu, J.rec.sc, (const PIX*)nullptr, 0, 0, 0, yc, xc, sizeC, ur, dl, 0, bd);
      pred_intra<SP>(t, ws->edgep, yc, xc, sizeC, ws->pred_u, sizeC, p.intra_mode, bd);
      t.sync();
      make_edges<SP>(t, ws->edgep, fv, J.rec.sc, (const PIX*)nullptr, 0, 0, 0, yc, xc, sizeC, ur, dl, 0, bd);
      pred_intra<SP>(t, ws->edgep, yc, xc, sizeC, ws->pred_v, sizeC, p.intra_mode, bd);
      t.sync();
      if (c.cfl_intra) improve_uv<PIX, SP>(t, ws, ws->pred_y, ws->pred_u, ws->pred_v, ws->rec_y, size, size, size, bd);
      cbp_u = code_tu_sp<PIX, SP, SP_LDS>(t, ws->xfp, ou, osc, ws->pred_u, sizeC, ws->rec_u, sizeC, sizeC, qpC, ftI | 1,
                      c.encoder_speed > 1, ws->coef_u, bd);
      cbp_v = code_tu_sp<PIX, SP, SP_LDS>(t, ws->xfp, ov, osc, ws->pred_v, sizeC, ws->rec_v, sizeC, sizeC, qpC, ftI | 1,
                      c.encoder_speed > 1, ws->coef_v, bd);
    }
  } else {
    const int split = (TKU(p.mode) == M_INTER || TKU(p.mode) == M_BIPRED) ? c.enable_pb_split : 0;
    if (!(reuse_pred == 2 || (reuse_pred && !c.cfl_inter))) predict_inter<PIX, SP>(t, J, ws, nd_, p, split);
    if (TKU(p.mode) == M_SKIP || zero_block) {
      copy_block<SP, SP>(t, ws->rec_y, size, ws->pred_y, size, nd.bw, nd.bh);
      copy_block<SP, SP>(t, ws->rec_u, sizeC, ws->pred_u, sizeC, nd.bw >> 1, nd.bh >> 1);
      copy_block<SP, SP>(t, ws->rec_v, sizeC, ws->pred_v, sizeC, nd.bw >> 1, nd.bh >> 1);
      t.sync();
    } else {
      cbp_y = code_inter_plane<PIX, SP, SP_LDS>(t, J, ws, oy, osy, ws->pred_y, ws->rec_y, size, qpY, ftI | 0, tb_split, ws->coef_y, size, pc);
      if (prune_after_luma<PIX, SP>(t, J, ws, size, nd.bw, nd.bh, p, cbp_y, tb_split, pc)) return 0;
      if (c.cfl_inter) improve_uv<PIX, SP>(t, ws, ws->pred_y, ws->pred_u, ws->pred_v, ws->rec_y, size, size, size, bd);
      const int csplit = tb_split && sizeC > 4;
      if (bigc) {
        cbp_u = code_inter_plane<PIX, SP, SP_GLOBAL>(t, J, ws, ou, osc, ws->pred_u, ws->rec_u, sizeC, qpC, ftI | 1, csplit, ws->coef_u);
        cbp_v = code_inter_plane<PIX, SP, SP_GLOBAL>(t, J, ws, ov, osc, ws->pred_v, ws->rec_v, sizeC, qpC, ftI | 1, csplit, ws->coef_v);
      } else {
        cbp_u = code_inter_plane<PIX, SP, SP_LDS>(t, J, ws, ou, osc, ws->pred_u, ws->rec_u, sizeC, qpC, ftI | 1, csplit, ws->coef_u);
        cbp_v = code_inter_plane<PIX, SP, SP_LDS>(t, J, ws, ov, osc, ws->pred_v, ws->rec_v, sizeC, qpC, ftI | 1, csplit, ws->coef_v);
      }
    }
  }
  p.cbp_y = (uint8_t)cbp_y;
  p.cbp_u = (uint8_t)cbp_u;
  p.cbp_v = (uint8_t)cbp_v;
  TK_PROF_T0();
  const SynCtx syn = lds_ld(&nd_.syn);
  const int* yb = (pc && pc->have_ybits) ? pc->ybits : nullptr;
  int nb_ = bigc ? bs_block_t<false, SP_GLOBAL>(bs, syn, p, ws->coef_y, ws->coef_u, ws->coef_v, &t, yb)   // bs.emit == 0 always here
                 : bs_block_t<false, SP_LDS>(bs, syn, p, ws->coef_y, ws->coef_u, ws->coef_v, &t, yb);
  TK_PROF_ADD(ws, PF_BITS);
  return nb_;
}

// One RDO trial: count bits, evaluate cost, keep `best` (copy_best_parameters, :1615-1677).
template <typename PIX, int SP>
TK_DEV unsigned rdo_trial(const Team t, JobR<PIX> J, WsP<PIX> ws, Node& nd, BlkParam& p, double lambda,
                          int reuse_pred = 0, unsigned prune_thr = 0xffffffffu, const unsigned long long* bestkey = nullptr,
                          unsigned order = 0, int* nbits_out = nullptr, int* untouched = nullptr) {
  BitSink cnt;
  cnt.buf = nullptr; cnt.pos = 0; cnt.cap = 0; cnt.emit = 0; cnt.ovf = 0;
  PruneCtx pc;
  pc.thr = prune_thr; pc.bestkey = bestkey; pc.order = order; pc.lambda = lambda; pc.ssd_y = -1; pc.have_ybits = 0; pc.pruned = 0; pc.ssd_part = 0; pc.bits_part = 0;
  pc.head_bits = 0;
  if (bestkey || prune_thr != 0xffffffffu) {
    // The bits that do not depend on the residual (super-mode, partition, vector differences, intra mode, candidate index) are
    // known before anything is predicted or transformed, and the cost is monotone in every term: a trial whose bound with
    // SSD = 0 and no other bits already reaches the threshold / exceeds the shared minimum is dropped before it starts
    // (`untouched`: the prediction buffers still hold what they held), and the later bounds (luma coded) start from these
    // bits.  (A later trial of the same candidate has the same header bits against a threshold that has not grown: it is
    // dropped the same way and never asks for the prediction an earlier one did not build.)
    BitSink hb = cnt;
    bs_block_head_t<false>(hb, uniform_syn(lds_ld(&nd.syn)), uniform_blk(p));
    pc.head_bits = hb.pos;
    unsigned long long lb0 = (unsigned long long)(long long)mul_add_nofma(lambda, (double)hb.pos, 0.5);
    if (lb0 > (1ull << 30)) lb0 = 1ull << 30;
#if TK_HOST
    { extern long long g_prune_stat[8]; g_prune_stat[7] += prune_hit(&pc, lb0); }
#endif
    if (team_bcast0(t, prune_hit(&pc, lb0))) {
      if (untouched) *untouched = 1;
      return kCostInit;
    }
  }
  int nbits = encode_block<PIX, SP>(t, J, ws, nd, p, cnt, reuse_pred, &pc);
  if (nbits_out) *nbits_out = nbits;
  if (pc.pruned) return kCostInit;  // lower bound >= threshold: cannot be selected
  return rd_cost<PIX, SP>(t, J, ws, nd, nbits, lambda, pc.ssd_y);
}

TK_DEV BlkParam normalize_best(const Node& nd, const BlkParam& p) {
  BlkParam b = p;
  if (p.mode == M_SKIP || p.mode == M_MERGE) {
    const InterPred c = lds_ld((p.mode == M_SKIP) ? &nd.skip[p.skip_idx] : &nd.merge[p.skip_idx]);
    b.ref0 = c.ref0; b.ref1 = c.ref1; b.dir = c.dir;
    for (int i = 0; i < 4; i++) { b.mv0[i] = c.mv0; b.mv1[i] = c.mv1; }
  } else if (p.mode == M_INTRA) {
    b.ref0 = b.ref1 = 0; b.dir = -1;
    for (int i = 0; i < 4; i++) { b.mv0[i] = mk_mv(0, 0); b.mv1[i] = mk_mv(0, 0); }
  } else if (p.mode == M_INTER) b.dir = 0;
  else b.dir = 2;
  return b;
}
TK_DEV void keep_best(Node& nd, const BlkParam& p) { lds_st(&nd.best, normalize_best(nd, p)); }

TK_DEV void set_cand(BlkParam& p, const InterPred& c, int idx, int mode) {
  p.mode = (int8_t)mode;
  p.skip_idx = (int8_t)idx;
  p.ref0 = c.ref0; p.ref1 = c.ref1; p.dir = c.dir;
  for (int i = 0; i < 4; i++) { p.mv0[i] = c.mv0; p.mv1[i] = c.mv1; }
}
}  // namespace tk
