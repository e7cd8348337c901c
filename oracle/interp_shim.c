/* interp_shim.c - TEST INFRASTRUCTURE.  Compiled only by oracle/Makefile (target interpshim) when the reference tree is present.  It #includes the
 * reference's common/temporal_interp.c BY PATH (nothing is copied into this repository) to reach its file-static stages - scale_frame_down2x2[_simd],
 * motion_estimate_bi, upscale_mv_data_2x2, interpolate_frame - and walks them in the order of interpolate_frames (:909-992), handing back what each stage
 * leaves behind, so that tests/golden/gen_kat12.py can record the stages and not only the final picture.  -DINTERP_SHIM_HBD: the 16-bit build
 * (what common/temporal_interp_hbd.c compiles), suffixed _hbd.  Both objects go into oracle/_ref/libinterpshim.so with the reference's common objects EXCEPT
 * temporal_interp.o / temporal_interp_hbd.o: this translation unit defines interpolate_frames_lbd / _hbd itself.
 *
 * The vector field before the merge pass: motion_estimate_bi allocates the merge pass's two output arrays with thor_alloc between its raster pass and its
 * merge pass (:832-833) and nowhere else.  For the included file thor_alloc is a macro that first copies mv_data->mv[1] of the call in flight (once per call) and then
 * allocates as before; the function itself stays unmodified. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#define STR2(x) #x
#define STR(x) STR2(x)
#ifdef INTERP_SHIM_HBD   /* the sample type of the 16-bit build, chosen before the first header as common/temporal_interp_hbd.c chooses it */
#define SAMPLE uint16_t
#define TEMPLATE(name) name##_hbd
#define HBD
#define SHIM(name) name##_hbd
#else
#define SHIM(name) name
#endif
#include "global.h"
#include "simd.h"

static const void* shim_src_mv1;   /* mv_data->mv[1] of the motion_estimate_bi call in flight */
static int16_t* shim_dst_mv1;      /* where its state before the merge pass goes; NULL once taken */
static size_t shim_mv_bytes;
static void shim_take_raster(void) {
  if (shim_dst_mv1) { memcpy(shim_dst_mv1, shim_src_mv1, shim_mv_bytes); shim_dst_mv1 = NULL; }
}
/* a macro, not a wrapper function: thor_alloc is alloca here (simd.h), its memory must belong to the caller's frame; the name inside is not expanded again */
#define thor_alloc(size, align) (shim_take_raster(), thor_alloc(size, align))
#include STR(REFDIR/common/temporal_interp.c)
#undef thor_alloc

static void shim_fill(yuv_frame_t* f, const SAMPLE* yuv) {
  const int w = f->width, h = f->height;
  for (int i = 0; i < h; i++) memcpy(f->y + i * f->stride_y, yuv + i * w, w * sizeof(SAMPLE));
  yuv += w * h;
  for (int i = 0; i < h / 2; i++) memcpy(f->u + i * f->stride_c, yuv + i * (w / 2), (w / 2) * sizeof(SAMPLE));
  yuv += (w / 2) * (h / 2);
  for (int i = 0; i < h / 2; i++) memcpy(f->v + i * f->stride_c, yuv + i * (w / 2), (w / 2) * sizeof(SAMPLE));
  TEMPLATE(pad_yuv_frame)(f);
}
/* the whole padded plane, rows of (w + 2 * pad) samples */
static SAMPLE* shim_take(SAMPLE* dst, const SAMPLE* p, int stride, int w, int h, int pad) {
  for (int i = -pad; i < h + pad; i++, dst += w + 2 * pad) memcpy(dst, p + i * stride - pad, (w + 2 * pad) * sizeof(SAMPLE));
  return dst;
}

/* interpolate_frames(new, ref0, ref1, ratio, pos) on two packed planar 4:2:0 frames (Y, U, V, stride = width), references padded by `pad` like the
 * encoder's.  Returns the number of pyramid levels.
 *   pyr       per reference r = 0, 1, per level l = 1 .. levels-1: the luma plane of in_down[l][r] with its padding of 32, (h>>l)+64 rows of (w>>l)+64
 *   mv_final  per level l = 0 .. levels-1: mv[0] then mv[1] of mv_data[l] after motion_estimate_bi, bw*bh (x, y) pairs each
 *   mv1_raster  per level: mv[1] as the raster pass left it (before the merge pass)
 *   out       new_frame after pad_yuv_frame (enc/mainenc.c:354): Y with `pad`, U and V with pad / 2, whole padded planes */
int SHIM(ref_interp_stages)(const SAMPLE* yuv0, const SAMPLE* yuv1, int widthin, int heightin, int bitdepth, int pad, int ratio, int pos, SAMPLE* pyr,
                            int16_t* mv_final, int16_t* mv1_raster, SAMPLE* out) {
  use_simd = 1;   /* what the encoder binary executes (init_use_simd) */
  yuv_frame_t ref[2], new_frame;
  for (int r = 0; r < 2; r++) {
    TEMPLATE(create_yuv_frame)(&ref[r], widthin, heightin, 420, pad, pad, bitdepth, bitdepth);
    shim_fill(&ref[r], r ? yuv1 : yuv0);
  }
  TEMPLATE(create_yuv_frame)(&new_frame, widthin, heightin, 420, pad, pad, bitdepth, bitdepth);

  /* from here: the statements of interpolate_frames in their order, with the copies in between */
  int max_levels = min(MAX_LEVELS, (int)(log10(min(widthin, heightin)) / log10(2.0) - 4.0));
  mv_data_t* mv_data[MAX_LEVELS];
  mv_data_t* spatial_mv_data[MAX_LEVELS];
  mv_data_t* guide_mv_data[NUM_GUIDES];
  yuv_frame_t in_down_store[MAX_LEVELS][2];
  yuv_frame_t* in_down[MAX_LEVELS][2];
  for (int j = 0; j < max_levels; j++) {
    mv_data[j] = alloc_mv_data(widthin >> j, heightin >> j, BLOCK_STEP / 2, BLOCK_STEP, ratio, pos, 1);
    mv_data[j]->ratio = ratio;
    spatial_mv_data[j] = alloc_mv_data(widthin >> j, heightin >> j, BLOCK_STEP / 2, BLOCK_STEP, ratio, pos, 1);
    spatial_mv_data[j]->ratio = ratio;
  }
  for (int i = 1; i < max_levels; ++i)
    for (int r = 0; r < 2; r++) {
      in_down[i][r] = &in_down_store[i][r];
      TEMPLATE(create_yuv_frame)(in_down[i][r], widthin >> i, heightin >> i, 420, 32, 32, bitdepth, bitdepth);
    }
  in_down[0][0] = &ref[0];
  in_down[0][1] = &ref[1];
  for (int l = 0; l < max_levels - 1; ++l)
    for (int r = 0; r < 2; r++) {
      TEMPLATE(scale_frame_down2x2_simd)(in_down[l][r], in_down[l + 1][r]);
      TEMPLATE(pad_yuv_frame)(in_down[l + 1][r]);
    }
  for (int r = 0; r < 2; r++)
    for (int l = 1; l < max_levels; l++) pyr = shim_take(pyr, in_down[l][r]->y, in_down[l][r]->stride_y, widthin >> l, heightin >> l, 32);

  size_t off[MAX_LEVELS + 1];   /* start of each level's fields, in vectors */
  off[0] = 0;
  for (int l = 0; l < max_levels; l++) off[l + 1] = off[l] + (size_t)mv_data[l]->bw * mv_data[l]->bh;
  for (int lvl = max_levels - 1; lvl >= 0; --lvl) {
    int num_guides = 0;
    if (lvl != max_levels - 1) guide_mv_data[num_guides++] = spatial_mv_data[lvl];
    const size_t n = (size_t)mv_data[lvl]->bw * mv_data[lvl]->bh;
    shim_src_mv1 = mv_data[lvl]->mv[1]; shim_dst_mv1 = mv1_raster + 2 * off[lvl]; shim_mv_bytes = n * sizeof(mv_t);
    motion_estimate_bi(mv_data[lvl], guide_mv_data, num_guides, in_down[lvl][0], in_down[lvl][1], pos);
    if (shim_dst_mv1) return -1;   /* the raster field was not taken: the reference changed */
    memcpy(mv_final + 2 * (2 * off[lvl]), mv_data[lvl]->mv[0], n * sizeof(mv_t));
    memcpy(mv_final + 2 * (2 * off[lvl] + n), mv_data[lvl]->mv[1], n * sizeof(mv_t));
    if (lvl == 0) interpolate_frame(mv_data[lvl], in_down[lvl][0], in_down[lvl][1], &new_frame, widthin, heightin, pos, ratio);
    if (lvl > 0) upscale_mv_data_2x2(mv_data[lvl], spatial_mv_data[lvl - 1]);
  }
  TEMPLATE(pad_yuv_frame)(&new_frame);
  out = shim_take(out, new_frame.y, new_frame.stride_y, widthin, heightin, pad);
  out = shim_take(out, new_frame.u, new_frame.stride_c, widthin / 2, heightin / 2, pad / 2);
  out = shim_take(out, new_frame.v, new_frame.stride_c, widthin / 2, heightin / 2, pad / 2);

  for (int j = 0; j < max_levels; j++) { free_mv_data(mv_data[j]); free_mv_data(spatial_mv_data[j]); }
  for (int i = 1; i < max_levels; ++i)
    for (int r = 0; r < 2; r++) TEMPLATE(close_yuv_frame)(in_down[i][r]);
  for (int r = 0; r < 2; r++) TEMPLATE(close_yuv_frame)(&ref[r]);
  TEMPLATE(close_yuv_frame)(&new_frame);
  return max_levels;
}
