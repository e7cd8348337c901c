/* refshim.c - TEST INFRASTRUCTURE.  Compiled only by oracle/Makefile (target reflib) when the
 * reference tree is present.  It #includes the reference's enc/encode_block.c BY PATH (nothing is
 * copied into this repository) to reach its file-static kernels, and exports thin wrappers so that
 * tests/golden/gen_kat*.py can record known-answer vectors from the real reference code.
 * -DREFSHIM_HBD: the 16-bit build of the same file (enc/encode_block_hbd.c by path) with the two motion-search
 * wrappers only, suffixed _hbd; linked into a shared object of its own (libthorref_hbd.so). */
#define STR2(x) #x
#define STR(x) STR2(x)
#ifdef REFSHIM_HBD
#include STR(REFDIR/enc/encode_block_hbd.c)
#define SHIM(name) name##_hbd
#else
#include STR(REFDIR/enc/encode_block.c)
#define SHIM(name) name
#endif
#include "simd.h"

/* motion_estimate (enc/encode_block.c:517, file-static) as search_inter_prediction_params calls it (:1033-1095): orig = the PU's first sample inside the
 * coding block's compact original block (stride = size = CB size), ref = the PU's co-located sample in the padded reference plane, xpos / ypos = the CB's
 * position.  mvcand: *mvcand_num full-pel entries.  use_simd = 1 is what the encoder executes.  mv_io: in mvc.x, mvc.y, mvp.x, mvp.y; out mv.x, mv.y. */
int SHIM(ref_motion_estimate)(SAMPLE* orig, SAMPLE* ref, int size, int stride_r, int width, int height, int16_t* mv_io, double lambda, int encoder_speed,
                              int bitdepth, int sign, int fwidth, int fheight, int xpos, int ypos, const int16_t* cand, int ncand, int enable_bipred) {
  static enc_params p;
  static mv_t list[64];
  mv_t mv, mvc, mvp;
  int n = ncand;
  memset(&p, 0, sizeof p);
  p.encoder_speed = encoder_speed; p.bitdepth = bitdepth; p.sync = 0;
  use_simd = 1;
  memset(list, 0, sizeof list);
  for (int i = 0; i < ncand; i++) { list[i].x = cand[2 * i]; list[i].y = cand[2 * i + 1]; }
  mvc.x = mv_io[0]; mvc.y = mv_io[1]; mvp.x = mv_io[2]; mvp.y = mv_io[3];
  mv.x = mv.y = 0;
  int r = motion_estimate(orig, ref, size, stride_r, width, height, &mv, &mvc, &mvp, lambda, &p, sign, fwidth, fheight, xpos, ypos, list, &n, enable_bipred);
  mv_io[4] = mv.x; mv_io[5] = mv.y;
  return r;
}
/* motion_estimate_bi (:798): one vector used as +mv on ref0 and -mv on ref1.  cand_io: six entries (x, y); the first ncand are the list on entry, all six are
 * returned as the call leaves them (slots ncand..3 zero-filled, slots 4 and 5 overwritten with mvp and (0,0)). */
int SHIM(ref_motion_estimate_bi)(SAMPLE* orig, SAMPLE* ref0, SAMPLE* ref1, int size, int stride_r, int16_t* mv_io, double lambda, int encoder_speed,
                                 int bitdepth, int sign, int fwidth, int fheight, int xpos, int ypos, int16_t* cand_io, int ncand, int enable_bipred) {
  static enc_params p;
  static mv_t list[64];
  mv_t mv, mvc, mvp;
  int n = ncand;
  memset(&p, 0, sizeof p);
  p.encoder_speed = encoder_speed; p.bitdepth = bitdepth; p.sync = 0;
  use_simd = 1;
  for (int i = 0; i < 6; i++) { list[i].x = cand_io[2 * i]; list[i].y = cand_io[2 * i + 1]; }
  mvc.x = mv_io[0]; mvc.y = mv_io[1]; mvp.x = mv_io[2]; mvp.y = mv_io[3];
  mv.x = mv.y = 0;
  int r = motion_estimate_bi(orig, ref0, ref1, size, stride_r, size, size, &mv, &mvc, &mvp, lambda, &p, sign, fwidth, fheight, xpos, ypos, list, &n, enable_bipred);
  for (int i = 0; i < 6; i++) { cand_io[2 * i] = list[i].x; cand_io[2 * i + 1] = list[i].y; }
  mv_io[4] = mv.x; mv_io[5] = mv.y;
  return r;
}

#ifndef REFSHIM_HBD
void ref_init(int simd) { use_simd = simd; }
unsigned ref_sad_calc(uint8_t* a, uint8_t* b, int astride, int bstride, int w, int h) { return sad_calc(a, b, astride, bstride, w, h); }
int ref_quantize(int16_t* coeff, int16_t* coeffq, int qp, int size, int coeff_block_type) {
  return quantize(coeff, coeffq, qp, size, coeff_block_type, NULL);
}
int ref_quote_mv_bits(int dy, int dx) { return quote_mv_bits(dy, dx); }
/* widesad_calc (enc/encode_block.c:430-453, file-static): SAD at the five horizontal offsets -3 -1 0 1 3, the best one and its offset; 16x16 with use_simd
 * takes widesad_calc_simd (enc/enc_kernels.c:84-113), which needs `a` 16-byte aligned */
unsigned ref_widesad_calc(uint8_t* a, uint8_t* b, int astride, int bstride, int w, int h, int* x) { return widesad_calc(a, b, astride, bstride, w, h, x); }
/* bit length of write_coeff (enc/write_bits.c:145) for one coefficient block */
int ref_coeff_bits(int16_t* coeff, int size, int type) {
  static uint8_t buf[1 << 16];
  stream_t s;
  s.bytesize = sizeof buf; s.bytepos = 0; s.bitstream = buf; s.bitbuf = 0; s.bitrest = 32;
  write_coeff(&s, coeff, size, type);
  return get_bit_pos(&s);
}

/* The two sub-block tests of the early-skip check (enc/encode_block.c:2146-2229, file-static): luma = 2x2 average + (N/2)-point transform against half the
 * threshold, chroma = calc_cbp on the residual's column sums - with use_simd (what the encoder runs) calc_cbp_simd (enc/enc_kernels.c:828-907).  They read
 * params->bitdepth only.  pblock is a compact size x size block. */
int ref_early_skip_sub(int chroma, uint8_t* orig, int ostride, int size, int qp, uint8_t* pblock, float thr, int bitdepth, int simd) {
  static enc_params p;
  static encoder_info_t ei;
  memset(&p, 0, sizeof p);
  memset(&ei, 0, sizeof ei);
  p.bitdepth = bitdepth;
  ei.params = &p;
  use_simd = simd;
  return chroma ? check_early_skip_sub_blockC(&ei, orig, ostride, size, qp, pblock, thr) : check_early_skip_sub_block(&ei, orig, ostride, size, qp, pblock, thr);
}

/* encoder_speed > 0 sub-pel approximations (file-static in encode_block.c) and their SIMD twins */
unsigned ref_fasthalf(uint8_t* a, uint8_t* b, int as, int bs, int w, int h, int* x, int* y, int simd) {
  if (simd) return sad_calc_fasthalf_simd_lbd(a, b, as, bs, w, h, x, y);
  return sad_calc_fasthalf(a, b, as, bs, w, h, x, y);
}
unsigned ref_fastquarter(uint8_t* o, uint8_t* r, int os, int rs, int w, int h, int* x, int* y, int simd) {
  if (simd) return sad_calc_fastquarter_simd_lbd(o, r, os, rs, w, h, x, y);
  return sad_calc_fastquarter(o, r, os, rs, w, h, x, y);
}
int ref_clpf_sample(int X, int A, int B, int C, int D, int E, int F, int G, int H, int s, unsigned dmp) { return clpf_sample(X, A, B, C, D, E, F, G, H, s, dmp); }
void ref_detect_multi_clpf(const uint8_t* rec, const uint8_t* org, int x0, int y0, int width, int height, int ostride, int rstride, int* sum,
                           unsigned shift, unsigned size, unsigned dmp, int simd) {
  if (simd) detect_multi_clpf_simd_lbd(rec, org, x0, y0, width, height, ostride, rstride, sum, shift, size, dmp);
  else detect_multi_clpf_lbd(rec, org, x0, y0, width, height, ostride, rstride, sum, shift, size, dmp);
}
#endif
