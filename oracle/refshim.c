/* refshim.c - TEST INFRASTRUCTURE.  Compiled only by oracle/Makefile (target reflib) when the
 * reference tree is present.  It #includes the reference's enc/encode_block.c BY PATH (nothing is
 * copied into this repository) to reach its file-static kernels, and exports thin wrappers so that
 * tests/golden/gen_kat*.py can record known-answer vectors from the real reference code.
 * -DREFSHIM_HBD: the 16-bit build of the same file (enc/encode_block_hbd.c by path) with the two motion-search
 * wrappers and the two CDEF entries only, suffixed _hbd; linked into a shared object of its own (libthorref_hbd.so).
 * enc/encode_frame.c (encode_frame_hbd.c) is included the same way, for its file-static dist_8x8: the two shared objects take the functions of that file from
 * this translation unit instead of encode_frame.o / encode_frame_hbd.o. */
#define STR2(x) #x
#define STR(x) STR2(x)
#ifdef REFSHIM_HBD
#include STR(REFDIR/enc/encode_block_hbd.c)
#include STR(REFDIR/enc/encode_frame_hbd.c)
#define SHIM(name) name##_hbd
#else
#include STR(REFDIR/enc/encode_block.c)
#include STR(REFDIR/enc/encode_frame.c)
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

/* ---- CDEF at frame level (tests/golden/gen_kat10.py -> kat10.npz).  Frames are packed planar 4:2:0 (Y, U, V, stride = width); mode: one byte per 4x4 cell,
 * (height / 4) rows of (width / 4), the block_mode_t of deblock_data_t.  The frames are rebuilt with create_yuv_frame (pad 0, as mainenc.c:176-178 makes
 * orig and rec), so rows have the alignment the reference's SIMD loads expect. */
typedef struct {
  enc_params params;
  encoder_info_t ei;
  yuv_frame_t rec, org;
  stream_t stream;
  uint8_t* sbuf;
  int nfb;
} cdef_shim_t;
static void cdef_shim_planes(yuv_frame_t* f, SAMPLE* yuv, int to_frame) {
  const int w = f->width, h = f->height;
  SAMPLE* pl[3] = {f->y, f->u, f->v};
  SAMPLE* p = yuv;
  for (int k = 0; k < 3; k++) {
    const int pw = k ? w / 2 : w, ph = k ? h / 2 : h, st = k ? f->stride_c : f->stride_y;
    for (int i = 0; i < ph; i++, p += pw) {
      if (to_frame) memcpy(pl[k] + i * st, p, pw * sizeof(SAMPLE));
      else memcpy(p, pl[k] + i * st, pw * sizeof(SAMPLE));
    }
  }
}
static void cdef_shim_open(cdef_shim_t* c, SAMPLE* rec_yuv, SAMPLE* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, int qp, int cdef_bits, int speed) {
  memset(c, 0, sizeof *c);
  c->params.bitdepth = c->params.input_bitdepth = bitdepth; c->params.subsample = 420; c->params.cdef = speed + 1;
  c->params.width = width; c->params.height = height;
  c->ei.params = &c->params; c->ei.width = width; c->ei.height = height;
  c->ei.frame_info.qp = qp; c->ei.frame_info.lambda = 1.0;
  c->ei.cdef_damping = 5; c->ei.cdef_bits = cdef_bits;                                   /* encode_frame.c:685-686 */
  TEMPLATE(create_yuv_frame)(&c->rec, width, height, 420, 0, 0, bitdepth, bitdepth);
  TEMPLATE(create_yuv_frame)(&c->org, width, height, 420, 0, 0, bitdepth, bitdepth);
  cdef_shim_planes(&c->rec, rec_yuv, 1); cdef_shim_planes(&c->org, org_yuv, 1);
  c->ei.rec = &c->rec; c->ei.orig = &c->org;
  const int ncell = (width / MIN_PB_SIZE) * (height / MIN_PB_SIZE);
  c->ei.deblock_data = (deblock_data_t*)calloc(ncell, sizeof(deblock_data_t));
  for (int i = 0; i < ncell; i++) c->ei.deblock_data[i].mode = (block_mode_t)mode[i];
  c->nfb = ((width + 63) >> 6) * ((height + 63) >> 6);
  c->ei.cdef = (cdef_strengths*)calloc(c->nfb, sizeof(cdef_strengths));
  c->sbuf = (uint8_t*)calloc(1, 1 << 16);
  c->stream.bytesize = 1 << 16; c->stream.bytepos = 0; c->stream.bitstream = c->sbuf; c->stream.bitbuf = 0; c->stream.bitrest = 32;
  c->ei.stream = &c->stream;
  use_simd = 1;
}
static void cdef_shim_close(cdef_shim_t* c) {
  TEMPLATE(close_yuv_frame)(&c->rec); TEMPLATE(close_yuv_frame)(&c->org);
  free(c->ei.deblock_data); free(c->ei.cdef); free(c->sbuf);
}
/* cdef_search + cdef_frame for planes 0, 1, 2 as encode_frame.c:768-774 runs them.  rec_yuv: the deblocked frame on entry, the filtered frame on return.
 * Returns cdef_search's bits.  strengths / uv_strengths: 8 entries each (127 where the search wrote none, :688-689).  fb_sel[4 * fb ..]: level and
 * sec_strength of plane[0], then of plane[1], of encoder_info->cdef[fb].  dir / var: per 8x8 luma block in frame raster order (width / 8 per row), -1 / 0 in
 * all-skip filter blocks; what cdef_frame(plane 0) left, which the chroma planes then read.  bit_pos: length of the per-filter-block preset string. */
int SHIM(ref_cdef_frame)(SAMPLE* rec_yuv, SAMPLE* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, int qp, int cdef_bits, int speed,
                         int* strengths, int* uv_strengths, int* fb_sel, int* dir, int* var, int* bit_pos) {
  cdef_shim_t c;
  cdef_shim_open(&c, rec_yuv, org_yuv, mode, width, height, bitdepth, qp, cdef_bits, speed);
  encoder_info_t* ei = &c.ei;
  for (int i = 0; i < 8; i++) ei->cdef_strengths[i] = ei->cdef_uv_strengths[i] = 127;
  for (int fb = 0; fb < c.nfb; fb++)
    for (int k = 0; k < 64; k++) ei->cdef[fb].dir[k] = -1;
  int bits = TEMPLATE(cdef_search)(ei->rec, ei->orig, ei->deblock_data, &ei->frame_info, ei, ei->cdef_strengths, ei->cdef_uv_strengths, ei->params->cdef - 1);
  TEMPLATE(cdef_frame)(ei->cdef, ei->rec, ei->orig, ei->deblock_data, &c.stream, 0, ei->params->bitdepth, 0);
  TEMPLATE(cdef_frame)(ei->cdef, ei->rec, ei->orig, ei->deblock_data, &c.stream, 0, ei->params->bitdepth, 1);
  TEMPLATE(cdef_frame)(ei->cdef, ei->rec, ei->orig, ei->deblock_data, &c.stream, 0, ei->params->bitdepth, 2);
  cdef_shim_planes(&c.rec, rec_yuv, 0);
  for (int i = 0; i < 8; i++) { strengths[i] = ei->cdef_strengths[i]; uv_strengths[i] = ei->cdef_uv_strengths[i]; }
  const int nfb_h = (width + 63) >> 6, bw = width / 8, bh = height / 8;
  for (int fb = 0; fb < c.nfb; fb++)
    for (int pl = 0; pl < 2; pl++) { fb_sel[4 * fb + 2 * pl] = ei->cdef[fb].plane[pl].level; fb_sel[4 * fb + 2 * pl + 1] = ei->cdef[fb].plane[pl].sec_strength; }
  for (int by = 0; by < bh; by++)
    for (int bx = 0; bx < bw; bx++) {
      const cdef_strengths* s = &ei->cdef[(by >> 3) * nfb_h + (bx >> 3)];
      dir[by * bw + bx] = s->dir[(by & 7) * 8 + (bx & 7)]; var[by * bw + bx] = s->dir[(by & 7) * 8 + (bx & 7)] < 0 ? 0 : s->var[(by & 7) * 8 + (bx & 7)];
    }
  *bit_pos = get_bit_pos(&c.stream);
  cdef_shim_close(&c);
  return bits;
}
/* The per-strength distortions cdef_search keeps in locals: its own loop (encode_frame.c:287-388) with its own functions - cdef_allskip, cdef_prepare_input,
 * cdef_find_dir[_simd], adjust_strength, cdef_filter_block[_simd], dist_8x8 - and nothing else.  mse[(g * nfb + fb) * 64 + gi], g = 0 luma / 1 chroma, fb in
 * frame raster order (zero for all-skip filter blocks and for gi >= the speed's number of strengths).  The generator checks the arrays against what
 * cdef_search itself chose. */
void SHIM(ref_cdef_mse)(SAMPLE* rec_yuv, SAMPLE* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, int speed, uint64_t* mse) {
  cdef_shim_t c;
  cdef_shim_open(&c, rec_yuv, org_yuv, mode, width, height, bitdepth, 32, 3, speed);
  yuv_frame_t *rec = &c.rec, *org = &c.org;
  deblock_data_t* deblock_data = c.ei.deblock_data;
  const int num_fb_hor = (width + 63) >> 6, num_fb_ver = (height + 63) >> 6, nfb = c.nfb;
  const int pri_damping = c.ei.cdef_damping, sec_damping = pri_damping, total_strengths = pristrengths[speed], bs = 8, bslog = 3, coeff_shift = bitdepth - 8;
  const int padding = 2 + CDEF_FULL, hpadding = 16 - padding, stride16 = (64 + 2 * padding + 15) & ~15, offset16 = padding * stride16 + padding + hpadding;
  uint16_t* src16 = thor_alloc((64 + 2 * padding) * stride16 * sizeof(uint16_t) + hpadding, 32);
  SAMPLE* dst = thor_alloc(bs * bs * sizeof(SAMPLE), 32);
  int cdef_directions_copy[8][2 + CDEF_FULL];
  cdef_init(stride16, cdef_directions_copy);
  memset(mse, 0, sizeof(uint64_t) * 2 * nfb * 64);
  for (int k = 0; k < num_fb_ver; k++)
    for (int l = 0; l < num_fb_hor; l++) {
      const int xoff = l << 6, yoff = k << 6, ci = k * num_fb_hor + l;
      if (cdef_allskip(xoff, yoff, width, height, deblock_data, 6)) continue;
      int h = min(height, (k + 1) << 6) & 63, w = min(width, (l + 1) << 6) & 63;
      h += !h << 6; w += !w << 6;
      for (int plane = 0; plane < 3; plane++) {
        const int sub = plane != 0 && rec->sub;
        const int sstride = plane != 0 ? rec->stride_c : rec->stride_y;
        SAMPLE* src_buffer = plane != 0 ? (plane == 1 ? rec->u : rec->v) : rec->y;
        int sizex = min(width - xoff, 64) >> sub, sizey = min(height - yoff, 64) >> sub, xpos = xoff >> sub, ypos = yoff >> sub;
        boundary_type bt = (TILE_LEFT_BOUNDARY & -!xpos) | (TILE_ABOVE_BOUNDARY & -!ypos) | (TILE_RIGHT_BOUNDARY & -(xpos == (width >> sub) - sizex)) |
                           (TILE_BOTTOM_BOUNDARY & -(ypos == (height >> sub) - sizey));
        TEMPLATE(cdef_prepare_input)(sizex, sizey, xpos, ypos, bt, padding, src16 + offset16, stride16, src_buffer, sstride);
        for (int gi = 0; gi < total_strengths; gi++) {
          const int pri_strength = priconv[speed][gi / CDEF_SEC_STRENGTHS], sec_strength = gi % CDEF_SEC_STRENGTHS;
          uint64_t* acc = &mse[((size_t)(!!plane) * nfb + ci) * 64 + gi];
          for (int m = 0; m < ((h + bs - 1) >> (bslog + sub)); m++)
            for (int n = 0; n < ((w + bs - 1) >> (bslog + sub)); n++) {
              xpos = (xoff >> sub) + n * bs; ypos = (yoff >> sub) + m * bs;
              sizex = min((width >> sub) - xpos, bs); sizey = min((height >> sub) - ypos, bs);
              const int index = ((yoff + m * 8) / MIN_PB_SIZE) * (width / MIN_PB_SIZE) + ((xoff + n * 8) / MIN_PB_SIZE);
              if (plane == 0 && gi == 0)
                c.ei.cdef[ci].dir[m * bs + n] = (use_simd ? TEMPLATE(cdef_find_dir_simd) : TEMPLATE(cdef_find_dir))(src_buffer + ypos * sstride + xpos, sstride, &c.ei.cdef[ci].var[m * bs + n], coeff_shift);
              if (deblock_data[index].mode == MODE_SKIP) continue;
              const int adj_str = plane ? pri_strength : adjust_strength(pri_strength, c.ei.cdef[ci].var[m * bs + n]);
              const int adj_pri_damping = adj_str ? max(log2i(adj_str), pri_damping - !!plane) : pri_damping - !!plane;
              const int adj_sec_damping = sec_damping - !!plane;
#ifdef HBD
              (use_simd ? cdef_filter_block_simd : cdef_filter_block)(NULL, dst, sizex, src16 + offset16 + n * bs + m * bs * stride16, stride16,
#else
              (use_simd ? cdef_filter_block_simd : cdef_filter_block)(dst, NULL, sizex, src16 + offset16 + n * bs + m * bs * stride16, stride16,
#endif
                  adj_str << coeff_shift, sec_strength << coeff_shift, pri_strength ? c.ei.cdef[ci].dir[m * bs + n] : 0, adj_pri_damping + coeff_shift,
                  adj_sec_damping + coeff_shift, sizex, cdef_directions_copy, coeff_shift);
              SAMPLE* org_buffer = (plane != 0 ? (plane == 1 ? org->u : org->v) : org->y) + ypos * sstride + xpos;
              if (plane || sizex != 8 || sizey != 8) {
                for (int i = 0; i < sizey; i++)
                  for (int j = 0; j < sizex; j++)
                    *acc += (dst[i * sizex + j] - org_buffer[i * sstride + j]) * (dst[i * sizex + j] - org_buffer[i * sstride + j]);
              } else *acc += dist_8x8(dst, sizex, org_buffer, sstride, coeff_shift);
            }
        }
      }
    }
  thor_free(src16); thor_free(dst);
  cdef_shim_close(&c);
}

/* cost_calc (enc/encode_block.c:916, file-static) as mode_decision_rdo calls it (tests/golden/gen_kat11.py -> kat11.npz): org / rec are compact blocks - Y size x size,
 * then U and V (size / 2)^2 each, stride = size - copied into two yuv_block_t, whose planes are arrays of MAX_SB_SIZE^2 samples; sub = 1 (4:2:0); use_simd = 1
 * is what the encoder executes (ssd_calc takes ssd_calc_simd for square blocks wider than 4). */
uint32_t SHIM(ref_cost_calc)(const SAMPLE* org, const SAMPLE* rec, int size, int width, int height, int nbits, double lambda, int bitdepth) {
  static yuv_block_t o __attribute__((aligned(32))), r __attribute__((aligned(32)));
  const int n = size * size, c = n / 4;
  memcpy(o.y, org, n * sizeof(SAMPLE)); memcpy(o.u, org + n, c * sizeof(SAMPLE)); memcpy(o.v, org + n + c, c * sizeof(SAMPLE));
  memcpy(r.y, rec, n * sizeof(SAMPLE)); memcpy(r.u, rec + n, c * sizeof(SAMPLE)); memcpy(r.v, rec + n + c, c * sizeof(SAMPLE));
  use_simd = 1;
  return cost_calc(&o, &r, size, width, height, 1, nbits, lambda, bitdepth);
}

/* search_intra_prediction_params (enc/encode_block.c:928, file-static) as mode_decision_rdo calls it: org_y a compact size x size block, plane the reconstructed
 * luma plane of fwidth x fheight samples with stride fwidth.  It reads rec->y, rec->stride_y and block_pos only.  Returns the SAD, *mode the intra_mode_t. */
int SHIM(ref_search_intra)(const SAMPLE* org_y, SAMPLE* plane, int fwidth, int fheight, int ypos, int xpos, int size, int sb_size, int num_intra_modes, int bitdepth, int* mode) {
  static SAMPLE o[MAX_SB_SIZE * MAX_SB_SIZE] __attribute__((aligned(32)));
  yuv_frame_t rec;
  block_pos_t bp;
  intra_mode_t m = MODE_DC;
  memset(&rec, 0, sizeof rec); memset(&bp, 0, sizeof bp);
  memcpy(o, org_y, size * size * sizeof(SAMPLE));
  rec.y = plane; rec.stride_y = fwidth; rec.width = fwidth; rec.height = fheight;
  bp.ypos = (uint16_t)ypos; bp.xpos = (uint16_t)xpos; bp.size = bp.bwidth = bp.bheight = (uint8_t)size; bp.sb_size = (uint8_t)sb_size;
  use_simd = 1;
  int sad = search_intra_prediction_params(o, &rec, &bp, fwidth, fheight, num_intra_modes, &m, bitdepth);
  *mode = (int)m;
  return sad;
}
/* The ten predictions that search weighs, by the functions it calls: out[mode * size * size ..], mode = intra_mode_t. */
void SHIM(ref_intra_preds)(SAMPLE* plane, int fwidth, int fheight, int ypos, int xpos, int size, int sb_size, int bitdepth, SAMPLE* out) {
  SAMPLE left_[2 * MAX_TR_SIZE + 2], top_[2 * MAX_TR_SIZE + 2], top_left;
  SAMPLE *left = left_ + 1, *top = top_ + 1;
  const int n = size * size;
  const int ur = get_upright_available(ypos, xpos, size, size, fwidth, fheight, sb_size), dl = get_downleft_available(ypos, xpos, size, size, fwidth, fheight, sb_size);
  TEMPLATE(make_top_and_left)(left, top, &top_left, &plane[ypos * fwidth + xpos], fwidth, NULL, 0, 0, 0, ypos, xpos, size, ur, dl, 0, bitdepth);
  TEMPLATE(get_dc_pred)(left, top, size, out + MODE_DC * n, size, bitdepth);
  TEMPLATE(get_hor_pred)(left, size, out + MODE_HOR * n, size);
  TEMPLATE(get_ver_pred)(top, size, out + MODE_VER * n, size);
  TEMPLATE(get_planar_pred)(left, top, top_left, size, out + MODE_PLANAR * n, size, bitdepth);
  TEMPLATE(get_upleft_pred)(left, top, top_left, size, out + MODE_UPLEFT * n, size);
  TEMPLATE(get_upright_pred)(top, size, out + MODE_UPRIGHT * n, size);
  TEMPLATE(get_upupright_pred)(top, size, out + MODE_UPUPRIGHT * n, size);
  TEMPLATE(get_upupleft_pred)(left, top, top_left, size, out + MODE_UPUPLEFT * n, size);
  TEMPLATE(get_upleftleft_pred)(left, top, top_left, size, out + MODE_UPLEFTLEFT * n, size);
  TEMPLATE(get_downleftleft_pred)(left, size, out + MODE_DOWNLEFTLEFT * n, size);
}

#ifndef REFSHIM_HBD
/* get_upright_available / get_downleft_available (common/common_block.h:60-95, static inline) as every caller uses them */
int ref_upright_available(int ypos, int xpos, int bwidth, int bheight, int fwidth, int fheight, int sb_size) { return get_upright_available(ypos, xpos, bwidth, bheight, fwidth, fheight, sb_size); }
int ref_downleft_available(int ypos, int xpos, int bwidth, int bheight, int fwidth, int fheight, int sb_size) { return get_downleft_available(ypos, xpos, bwidth, bheight, fwidth, fheight, sb_size); }
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
/* ---- the block syntax as bit STRINGS (tests/golden/gen_kat9.py): every wrapper writes into a fresh stream_t, returns the bit length and copies the string
 * - bitstream[0..bytepos) followed by the top 32 - bitrest bits of bitbuf - to out (at most out_bytes bytes). */
static uint8_t syn_buf[1 << 17];
static void syn_open(stream_t* s) {
  memset(syn_buf, 0, sizeof syn_buf);
  s->bytesize = sizeof syn_buf; s->bytepos = 0; s->bitstream = syn_buf; s->bitbuf = 0; s->bitrest = 32;
}
static int syn_close(stream_t* s, uint8_t* out, int out_bytes) {
  int nbits = get_bit_pos(s), n = 0;
  for (uint32_t i = 0; i < s->bytepos && n < out_bytes; i++) out[n++] = s->bitstream[i];
  for (int k = 0; k < (int)(32 - s->bitrest + 7) / 8 && n < out_bytes; k++) out[n++] = (uint8_t)(s->bitbuf >> (24 - 8 * k));
  return nbits;
}
/* put_vlc (enc/putvlc.c:73-160): one codeword of table n */
int ref_put_vlc(int n, unsigned cn, uint8_t* out, int out_bytes) {
  stream_t s;
  syn_open(&s);
  put_vlc(n, cn, &s);
  return syn_close(&s, out, out_bytes);
}
/* write_mv (enc/write_bits.c:123-143) */
int ref_write_mv(int mvx, int mvy, int mvpx, int mvpy, uint8_t* out, int out_bytes) {
  stream_t s;
  mv_t mv, mvp;
  mv.x = (int16_t)mvx; mv.y = (int16_t)mvy; mvp.x = (int16_t)mvpx; mvp.y = (int16_t)mvpy;
  syn_open(&s);
  write_mv(&s, &mv, &mvp);
  return syn_close(&s, out, out_bytes);
}
/* write_coeff (enc/write_bits.c:145-241) */
int ref_write_coeff(int16_t* coeff, int size, int type, uint8_t* out, int out_bytes) {
  stream_t s;
  syn_open(&s);
  write_coeff(&s, coeff, size, type);
  return syn_close(&s, out, out_bytes);
}
/* The flat parameter row of a kat9.npz block item (tests/golden/gen_kat9.py: BL_PAR): 0 kind, 1 split_flag, 2 frame_type, 3 num_ref, 4 enable_bipred,
 * 5 interp_ref, 6 max_pb_part, 7 max_tb_part, 8 num_intra_modes, 9 size, 10 encode_this_size, 11 context index, 12 context cbp, 13 num_skip, 14 num_merge,
 * 15 mvp.x, 16 mvp.y, 17 mode, 18 intra_mode, 19 skip_idx, 20 pb_part, 21 ref_idx0, 22 ref_idx1, 23 dir, 24 tb_param, 25 tb_split, 26..28 cbp y / u / v,
 * 29..36 mv_arr0 (x, y), 37..44 mv_arr1.  max_delta_qp = bitrate = 0, 4:2:0; the frame is as large as the block or empty, which makes
 * encode_this_size (enc/write_bits.c:386-388) come out as asked. */
static enc_params syn_params;
static encoder_info_t syn_ei;
static block_info_t syn_bi;
static block_context_t syn_ctx;
static block_param_t syn_bp;
static void syn_fill(const int* q) {
  memset(&syn_params, 0, sizeof syn_params); memset(&syn_ei, 0, sizeof syn_ei); memset(&syn_bi, 0, sizeof syn_bi);
  memset(&syn_ctx, 0, sizeof syn_ctx); memset(&syn_bp, 0, sizeof syn_bp);
  syn_params.enable_bipred = q[4]; syn_params.subsample = 420; syn_params.log2_sb_size = 7;
  syn_ei.params = &syn_params;
  syn_ei.frame_info.frame_type = (frame_type_t)q[2]; syn_ei.frame_info.num_ref = q[3]; syn_ei.frame_info.interp_ref = q[5];
  syn_ei.frame_info.num_intra_modes = q[8];
  syn_ei.width = syn_ei.height = q[10] ? q[9] : 0;
  syn_bi.block_pos.size = (uint8_t)q[9]; syn_bi.block_pos.bwidth = syn_bi.block_pos.bheight = (uint8_t)q[9]; syn_bi.block_pos.sb_size = 128;
  syn_bi.block_context = &syn_ctx; syn_bi.sub = 1;
  syn_ctx.index = (int8_t)q[11]; syn_ctx.cbp = (int8_t)q[12];
  syn_bi.max_num_pb_part = q[6]; syn_bi.max_num_tb_part = q[7]; syn_bi.num_skip_vec = q[13]; syn_bi.num_merge_vec = q[14];
  syn_bi.mvp.x = (int16_t)q[15]; syn_bi.mvp.y = (int16_t)q[16];
  syn_bp.mode = (block_mode_t)q[17]; syn_bp.intra_mode = (intra_mode_t)q[18]; syn_bp.skip_idx = q[19]; syn_bp.pb_part = q[20];
  syn_bp.ref_idx0 = q[21]; syn_bp.ref_idx1 = q[22]; syn_bp.dir = q[23]; syn_bp.tb_param = q[24]; syn_bp.tb_split = q[25];
  syn_bp.cbp.y = (uint8_t)q[26]; syn_bp.cbp.u = (uint8_t)q[27]; syn_bp.cbp.v = (uint8_t)q[28];
  for (int k = 0; k < 4; k++) {
    syn_bp.mv_arr0[k].x = (int16_t)q[29 + 2 * k]; syn_bp.mv_arr0[k].y = (int16_t)q[30 + 2 * k];
    syn_bp.mv_arr1[k].x = (int16_t)q[37 + 2 * k]; syn_bp.mv_arr1[k].y = (int16_t)q[38 + 2 * k];
  }
}
/* write_super_mode (enc/write_bits.c:257-358) with split_flag = par[1], encode_this_size = par[10] */
int ref_write_super_mode(const int* par, uint8_t* out, int out_bytes) {
  stream_t s;
  syn_fill(par);
  syn_open(&s);
  write_super_mode(&s, &syn_ei, &syn_bi, &syn_bp, par[1], par[10]);
  return syn_close(&s, out, out_bytes);
}
/* write_block (enc/write_bits.c:360-600); cy / cu / cv: 4 * MAX_QUANT_SIZE^2 coefficients each, laid out as block_param_t holds them */
int ref_write_block(const int* par, const int16_t* cy, const int16_t* cu, const int16_t* cv, uint8_t* out, int out_bytes) {
  stream_t s;
  syn_fill(par);
  memcpy(syn_bp.coeff_y, cy, sizeof syn_bp.coeff_y); memcpy(syn_bp.coeff_u, cu, sizeof syn_bp.coeff_u); memcpy(syn_bp.coeff_v, cv, sizeof syn_bp.coeff_v);
  syn_open(&s);
  int r = write_block(&s, &syn_ei, &syn_bi, &syn_bp);
  int n = syn_close(&s, out, out_bytes);
  return r == n ? n : -1;
}
/* zigzag16 / zigzag64 / zigzag256 (common/common_tables.c): position -> scan index of a qsize x qsize block */
void ref_zigzag(int qsize, int* out) {
  const int* z = qsize == 4 ? zigzag16 : qsize == 8 ? zigzag64 : zigzag256;
  for (int i = 0; i < qsize * qsize; i++) out[i] = z[i];
}
#endif
