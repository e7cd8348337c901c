/* thor_hip.h - C ABI of libthor_hip.so, the MI355X (gfx950) implementation of the Thor encoder's
 * per-block hot path.  Plain C: pointers and sizes only, no C++/torch types.
 *
 * Three groups of entry points:
 *
 *  (1) The drop-in seam.  encode_frame_lbd / encode_frame_hbd are the only symbols the reference
 *      front end (enc/mainenc.o) imports from the hot path (enc/encode_frame.h:32-33, called at
 *      enc/mainenc.c:548).  Linking the reference's mainenc/strings/putbits/putvlc/write_bits
 *      objects against this library instead of encode_frame.o/encode_block.o gives a Thorenc that
 *      runs the block path on the GPU.  They take the reference's own
 *      encoder_info_t (enc/mainenc.h:158-184); its layout is restated in thor_abi.h.
 *
 *  (2) The sequence API used by bench.py / the tests: N independent closed streams (what the
 *      reference produces with -skip c*F -n F) encoded in lock step on one GPU,
 *      with the low-delay GOP decisions of enc/mainenc.c:261-523 made on the host.
 *
 *  (3) Kernel-level batch entry points for known-answer tests against the scalar reference
 *      functions (sad_calc encode_block.c:417, get_inter_prediction_luma inter_prediction.c:117,
 *      transform/quantize/dequantize/inverse_transform, deblock_frame_y/uv common_frame.c:47/354).
 *
 * Error convention: like the reference's fatalerror() (common/global.h:38-44) unrecoverable
 * conditions (no GPU, HIP failure, bit-buffer overflow) print to stderr and abort(); the
 * sequence API additionally returns 0 on success / non-zero on bad arguments.
 */
#ifndef THOR_HIP_H
#define THOR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) drop-in seam ------------------------------------------------------------------- */
struct thor_encoder_info; /* == reference encoder_info_t, see thor_abi.h */
void encode_frame_lbd(struct thor_encoder_info* encoder_info); /* replaces enc/encode_frame.c:637 (SAMPLE=uint8_t)  */
void encode_frame_hbd(struct thor_encoder_info* encoder_info); /* replaces enc/encode_frame_hbd.c (SAMPLE=uint16_t) */

/* ---- (2) sequence API --------------------------------------------------------------------- */
typedef struct thor_hip_params { /* the enc_params fields this path honours (enc/mainenc.h:35-112) */
  int width, height, qp;
  int bitdepth, input_bitdepth;
  float frame_rate;
  float lambda_coeffI, lambda_coeffP;
  float early_skip_thr;
  int enable_tb_split, enable_pb_split, max_num_ref, HQperiod;
  int num_reorder_pics, interp_ref;
  int dqpP, dqpI;
  float mqpP;
  int intra_period, intra_rdo, encoder_speed;
  int deblocking, cdef, clpf, use_block_contexts, enable_bipred;
  int cfl_intra, cfl_inter;
  /* hierarchical-B coding (num_reorder_pics > 0; enc/mainenc.c:270-345) */
  int dyadic_coding;
  float lambda_coeffB, lambda_coeffB0, lambda_coeffB1, lambda_coeffB2, lambda_coeffB3;
  int dqpB, dqpB0, dqpB1, dqpB2, dqpB3;
  float mqpB, mqpB0, mqpB1, mqpB2, mqpB3;
  int max_clpf_strength; /* CLPF strength cap (enc/strings.c:351) */
  int log2_sb_size;      /* 7: 128x128 superblocks (the default), 6: 64x64; nothing else is accepted (enc/strings.c:299) */
} thor_hip_params;

typedef struct thor_hip_encoder thor_hip_encoder;

/* Fill *p with the reference defaults (enc/strings.c:287-356) and then apply a Thorenc config
 * file ("-name value" tokens, ';' comments).  cfg_path may be NULL. Returns 0 on success. */
int thor_hip_params_from_config(thor_hip_params* p, const char* cfg_path);

/* Apply one "-name value" option (same names as enc/strings.c:287-356) on top of *p.  Returns 0 when the option is
 * honoured; 1 = not an option of the reference's table; 2 = known, but the value is not implemented by this path
 * (quantisation matrices, delta-QP / rate control, sync, subsampling other than 4:2:0, SB size other than 128: they
 * change the bitstream, so they are rejected instead of ignored); 3 = front-end option (-if/-of/-rf/-n/-skip).
 * thor_hip_params_from_config applies the same rule to every token of the file (returns non-zero), except that a file
 * may say "-log2_sb_size 6". */
int thor_hip_params_set(thor_hip_params* p, const char* name, const char* value);

/* Choose the superblock size: log2_sb_size 7 (128x128) or 6 (64x64) is stored in *p and 0 returned; any other value
 * returns 2 and leaves *p alone.  thor_hip_params_set keeps answering 2 to "-log2_sb_size" with anything but 7, as it
 * did before 64x64 superblocks were implemented, so this is the call (or the struct field itself) to select them. */
int thor_hip_params_set_sb_size(thor_hip_params* p, int log2_sb_size);

int thor_hip_device_count(void);
/* One process drives ONE GPU from ONE thread (the reference's encode_frame is neither re-entrant nor threaded,
 * SURVEY.md 8b): the first thor_hip_open binds the process to `device`; NULL is returned - with a message on stderr -
 * for a device index the node does not have (a node without any device included), for a second device in the same
 * process, and for parameter sets this path cannot encode bit-exactly.  Multi-GPU = one process per GPU (bench.py under torch.distributed.run). */
thor_hip_encoder* thor_hip_open(const thor_hip_params* p, int num_streams, int device);
void thor_hip_close(thor_hip_encoder* e);

/* Coding-order schedule (the frame loop of enc/mainenc.c:246-625).  thor_hip_begin_sequence fixes the
 * chunk [skip, skip + num_frames) of an input holding file_frames frames for one stream; without it a
 * stream is an open-ended low-delay sequence starting at frame 0.  thor_hip_next_frame returns 1 and the
 * chunk-relative DISPLAY index of the next frame to code (B frames are coded out of display order), or 0
 * when the chunk is finished; the following encode call must be given exactly that frame.  Calling it is
 * optional for low-delay streams (coding order == display order). */
int thor_hip_begin_sequence(thor_hip_encoder* e, int stream, int skip, int num_frames, int file_frames);
int thor_hip_next_frame(thor_hip_encoder* e, int stream, int* display_index);

/* Frames cross this API at the INPUT bit depth: planar 4:2:0, input_bitdepth 8: bytes; 10 / 12: little-endian uint16 -
 * thor_hip_frame_bytes(e) bytes each.  bitdepth (the depth the encoder works at) may be higher: (10, 8), (12, 8) and (12, 10) are
 * accepted besides the three equal pairs.  The device then widens a staged frame (v << (bitdepth - input_bitdepth)) and rounds a
 * reconstruction back (saturate((v + half) >> shift)), as the reference reads its -if and writes its -rf file
 * (common/common_frame.c:484-650), and distortion is measured at the input depth (common/snr.c:39-61).  With equal depths nothing
 * is launched or copied beyond what equal depths always took.  input_bitdepth > bitdepth is refused by thor_hip_open. */
size_t thor_hip_frame_bytes(const thor_hip_encoder* e);
/* Copy one such frame of stream `stream` into HBM staging slot `slot` (slots are allocated on demand). */
int thor_hip_stage_frame(thor_hip_encoder* e, int stream, int slot, const void* yuv);
/* Same, for a frame that is already in HBM (`dev_yuv` is a device pointer to the same contiguous planar layout):
 * device-to-device copy on the library's stream, synchronous at return.  The caller must have finished writing the
 * source (e.g. torch.cuda.synchronize()).  Used by bench.py: rank 0 broadcasts the clip over RCCL and every rank cuts
 * its chunks' frames out of it without a host round trip.  With input_bitdepth < bitdepth the widening kernel reads dev_yuv
 * directly (no intermediate copy); dev_yuv must then be 16-byte aligned (returns 1 otherwise). */
int thor_hip_stage_frame_device(thor_hip_encoder* e, int stream, int slot, const void* dev_yuv);
/* Encode the next frame of every stream from staging slot slots[stream] (inputs already resident
 * in HBM).  Blocks until the bits of all streams are assembled on the host. */
int thor_hip_encode_staged(thor_hip_encoder* e, const int* slots);
/* Encode the next `nframes` frames of every stream, each from the staging slot with the frame's chunk-relative DISPLAY index (what
 * thor_hip_next_frame reports; low-delay streams: the coded index), with the streams in TWO GROUPS HALF A FRAME APART: a launch of the
 * persistent superblock kernel carries the second half of one group's frame (the narrowing end of its dependency wavefront over the
 * superblock grid) and the first half of the other group's, so the workgroup slots one group leaves idle are taken by the other - in lock
 * step (thor_hip_encode_staged frame by frame) every stream ramps up and down at the same time.  The run starts and ends on a frame
 * boundary of every stream; the bits and reconstructions are those of the frame-by-frame calls (the order in which superblocks are coded
 * never changes a result: every superblock starts after its dependencies, enc/encode_frame.c:697-835 raster order).
 * `done` (may be NULL) is called from the calling thread whenever the frames of streams [first_stream, first_stream + num_streams) are
 * complete: their bits are appended, thor_hip_get_recon returns that frame and thor_hip_last_display_index its display index until the
 * callback returns.  Returns 0; 2 when a stream has fewer than `nframes` frames left in its chunk, 3 when a frame of the run is not staged -
 * both are found by a dry run of every stream's schedule BEFORE the first launch: a refused run touches nothing and may be repeated. */
typedef void (*thor_hip_frames_done_fn)(void* user, int first_stream, int num_streams);
int thor_hip_encode_staged_run(thor_hip_encoder* e, int nframes, thor_hip_frames_done_fn done, void* user);
/* Chunk-relative display index of the frame stream `stream` coded last (-1: none yet). */
int thor_hip_last_display_index(const thor_hip_encoder* e, int stream);
/* Convenience: stage + encode one host frame per stream (PCIe inclusive). */
int thor_hip_encode_frame(thor_hip_encoder* e, const void* const* yuv_per_stream);

/* Finished bitstream of a stream so far (sequence header + framed frames, identical to the file
 * the reference writes with -of). The pointer stays valid until the next encode call. */
size_t thor_hip_stream_bytes(const thor_hip_encoder* e, int stream);
const uint8_t* thor_hip_stream_data(const thor_hip_encoder* e, int stream);
/* Reconstruction of the most recently CODED frame of a stream (the reference writes these with -rf in
 * display order), thor_hip_frame_bytes(e) bytes of input-depth samples. */
int thor_hip_get_recon(thor_hip_encoder* e, int stream, void* yuv_out);

/* Frames in the layouts decoders, capture cards and GPU pipelines hold: semi-planar chroma (NV12 / NV21 at 8 bits; P010 / P012 / P016
 * above), a row pitch wider than the picture, 16-bit samples in the high bits.  A layout is given per call, not in thor_hip_params.
 * All fields 0 apart from `size` is the packed planar frame of the calls above.  Samples are input_bitdepth wide: one byte for 8 bits,
 * two bytes (little-endian) otherwise.  One kernel converts between the layout and the encoder's planes, depth conversion included:
 *   staging:  x = msb_aligned ? s >> (16 - input_bitdepth) : s;  the staged sample is x << (bitdepth - input_bitdepth)
 *   fetching: r = the reconstruction rounded and saturated to input_bitdepth (thor_hip_get_recon's value);
 *             written is msb_aligned ? r << (16 - input_bitdepth) : r
 * Bytes of a row beyond the picture's width and bytes between the planes are never read on staging and never written on fetching.
 * Planes must not overlap (not checked). */
enum { THOR_HIP_CHROMA_PLANAR = 0, THOR_HIP_CHROMA_UV = 1, THOR_HIP_CHROMA_VU = 2 };
typedef struct thor_hip_frame_layout {
  int    size;         /* sizeof(thor_hip_frame_layout): lets the struct grow later */
  int    chroma;       /* planar U,V planes | one interleaved plane U0 V0 U1 V1.. | V0 U0.. */
  int    msb_aligned;  /* 0: value in the low bits.  1: value << (16 - input_bitdepth), the P010 / P012 / P016
                          convention; only legal with input_bitdepth > 8 */
  int    pitch_y;      /* bytes between luma rows; 0 = tight */
  int    pitch_c;      /* bytes between rows of each chroma plane (or of the interleaved plane); 0 = tight */
  size_t offset_u;     /* bytes from the base to the U plane (or the interleaved plane);
                          0 = directly after luma (pitch_y * height) */
  size_t offset_v;     /* planar only: bytes from the base to the V plane; 0 = directly after U (pitch_c * height / 2) */
} thor_hip_frame_layout;
/* Bytes a frame in `layout` spans from its base, whole pitch of the last row included (width * height * 3 / 2 samples when tight);
 * 0 if the layout is refused: `size` is wrong, `chroma` is unknown, a pitch is below the row's bytes, a pitch or an offset is no
 * multiple of the sample size, msb_aligned is set with 8-bit input.  thor_hip_layout_bytes_for needs no encoder (and no device). */
size_t thor_hip_layout_bytes(const thor_hip_encoder* e, const thor_hip_frame_layout* layout);
size_t thor_hip_layout_bytes_for(int width, int height, int input_bitdepth, const thor_hip_frame_layout* layout);
/* thor_hip_stage_frame / thor_hip_stage_frame_device (on_device != 0: `frame` is a device pointer) for a frame in `layout`.  A device
 * frame is read by the kernel that writes the slot: no intermediate copy, no alignment demanded beyond the sample size (16-byte aligned
 * base and pitches move in 16-byte vectors, anything else sample by sample).  A host frame's thor_hip_layout_bytes bytes are copied
 * once into a device buffer the encoder keeps and the same kernel runs.  Synchronous at return, on the library's stream, like
 * thor_hip_stage_frame_device.  Returns 0; 1 for a bad argument, a refused layout or a base pointer that is not sample-aligned -
 * found before the device is touched. */
int thor_hip_stage_frame_layout(thor_hip_encoder* e, int stream, int slot, const void* frame, const thor_hip_frame_layout* layout, int on_device);
/* thor_hip_get_recon into a frame in `layout`, in host memory or (on_device != 0) in device memory.  Same return values. */
int thor_hip_get_recon_layout(thor_hip_encoder* e, int stream, void* frame, const thor_hip_frame_layout* layout, int on_device);

/* RGB frames, as screen capture, renderers and tensor pipelines hold them.  The format is given per call.  Staging an RGB frame means exactly:
 * convert it to a planar 4:2:0 frame of input_bitdepth samples (below) and stage that frame (so every sample is then widened by
 * bitdepth - input_bitdepth like any staged frame); fetching means: take thor_hip_get_recon's frame (already rounded back to input_bitdepth) and
 * convert it to RGB (below).  One kernel each way (k_rgb_in, k_rgb_out); integers only.
 *
 * Samples: one byte for depth 8, a little-endian 16-bit word for depth 10 / 12 / 16.  A sample's value is s >> (16 - depth) when msb_aligned,
 * else s (not masked: a value above 2^depth - 1 only meets the clamps below).  Packed orders hold 4 or 3 samples per pixel in the order named; the
 * fourth channel (A) is ignored on input and written as 2^depth - 1 (shifted like the others when msb_aligned).  PLANAR_RGB is three planes R, G, B,
 * plane_stride bytes apart, each with `pitch`.
 *
 * Constants, with n = input_bitdepth, M = 2^depth - 1, and Kr / Kb over 10000: 2990 / 1140 (BT.601), 2126 / 722 (BT.709), 2627 / 593 (BT.2020,
 * non-constant luminance); Kg = 10000 - Kr - Kb (5870, 7152, 6780).
 *   limited range: SY = 219 << (n - 8), SC = 224 << (n - 8), OY = 16 << (n - 8);  full range: SY = SC = 2^n - 1, OY = 0;  OC = 1 << (n - 1)
 *   rdiv(a, b) = (2 * a + b) / (2 * b) in integers (a / b rounded to nearest, halves up; a, b positive; 64-bit)
 * RGB -> Y'CbCr, F = 24 fractional bits:
 *   yr = rdiv((Kr * SY) << F, 10000 * M)   yb = rdiv((Kb * SY) << F, 10000 * M)   yg = rdiv(SY << F, M) - yr - yb
 *   ub = rdiv(SC << F, 2 * M)   ur = -rdiv((Kr * SC) << F, 2 * (10000 - Kb) * M)   ug = -ub - ur
 *   vr = rdiv(SC << F, 2 * M)   vb = -rdiv((Kb * SC) << F, 2 * (10000 - Kr) * M)   vg = -vr - vb
 *   Y(x, y)  = clamp((yr * R + yg * G + yb * B + (OY << F) + (1 << (F - 1))) >> F, 0, 2^n - 1)            for every pixel
 *   chroma sample (i, j) sums taps of weight w, total 2^L, over the rows 2j and 2j + 1:
 *     chroma_site 0 (centre): columns 2i, 2i + 1, w = 1, L = 2
 *     chroma_site 1 (left):   columns 2i - 1, 2i, 2i + 1 with w = 1, 2, 1; column -1 is column 0; L = 3
 *     tR = sum of w * R over the taps, tG and tB likewise
 *   Cb(i, j) = clamp((ur * tR + ug * tG + ub * tB + (OC << (F + L)) + (1 << (F + L - 1))) >> (F + L), 0, 2^n - 1),  Cr with vr, vg, vb
 *   (>> is the arithmetic shift: floor).  ur + ug + ub = vr + vg + vb = 0, so R = G = B gives Cb = Cr = OC; black gives Y = OY and white OY + SY.
 *   The coefficients are at most 1.5 units of 2^-24 off, times M <= 65535: under 0.01 of a code value, so a result differs from the textbook
 *   formula in float64, rounded to nearest, only where that lies within 0.01 of a rounding step, and then by one.
 * Y'CbCr -> RGB, G = 20 fractional bits, chroma sample (i, j) used for the four pixels of its quad with either chroma_site:
 *   iy = rdiv(M << G, SY)   rv = rdiv((2 * (10000 - Kr) * M) << G, 10000 * SC)   bu = rdiv((2 * (10000 - Kb) * M) << G, 10000 * SC)
 *   gu = -rdiv((2 * Kb * (10000 - Kb) * M) << G, 10000 * Kg * SC)   gv = -rdiv((2 * Kr * (10000 - Kr) * M) << G, 10000 * Kg * SC)
 *   l = iy * (Y - OY) + (1 << (G - 1))
 *   R = clamp((l + rv * (Cr - OC)) >> G, 0, M)   G = clamp((l + gu * (Cb - OC) + gv * (Cr - OC)) >> G, 0, M)   B = clamp((l + bu * (Cb - OC)) >> G, 0, M)
 *   written as value << (16 - depth) when msb_aligned.
 * Bytes of a row beyond the picture's width and bytes between planes are never read on staging and never written on fetching. */
enum { THOR_HIP_RGB_RGBA = 0, THOR_HIP_RGB_BGRA = 1, THOR_HIP_RGB_ARGB = 2, THOR_HIP_RGB_ABGR = 3, THOR_HIP_RGB_RGB = 4, THOR_HIP_RGB_BGR = 5,
       THOR_HIP_RGB_PLANAR_RGB = 6 };
enum { THOR_HIP_MATRIX_BT601 = 0, THOR_HIP_MATRIX_BT709 = 1, THOR_HIP_MATRIX_BT2020 = 2 };
typedef struct thor_hip_rgb_format {
  int    size;         /* sizeof(thor_hip_rgb_format) */
  int    order;        /* THOR_HIP_RGB_* */
  int    depth;        /* bits per channel: 8 (one byte), 10, 12 or 16 (16-bit words) */
  int    msb_aligned;  /* depth 10 / 12 only: the value sits in the high bits of the word, as in P010 */
  int    matrix;       /* THOR_HIP_MATRIX_* */
  int    full_range;   /* 0: 16..235 / 16..240 scaled to input_bitdepth; 1: 0..2^input_bitdepth - 1 */
  int    chroma_site;  /* 0: centre of the 2x2 quad; 1: left (the MPEG-2 / H.264 default) */
  int    pitch;        /* bytes between rows; 0 = tight */
  size_t plane_stride; /* PLANAR_RGB only: bytes between planes; 0 = pitch * height */
} thor_hip_rgb_format;
/* Bytes a frame in `fmt` spans from its base; 0 if the format is refused: `size` is wrong; order, depth, matrix, full_range or chroma_site is
 * unknown; msb_aligned is set with depth 8 or 16; the pitch is negative, below the row's bytes or no multiple of the sample size; plane_stride
 * is set for a packed order, is below pitch * height or is no multiple of the sample size.  thor_hip_rgb_bytes_for needs no encoder and no device
 * (width and height: multiples of 8, at least 16). */
size_t thor_hip_rgb_bytes(const thor_hip_encoder* e, const thor_hip_rgb_format* fmt);
size_t thor_hip_rgb_bytes_for(int width, int height, const thor_hip_rgb_format* fmt);
/* thor_hip_stage_frame_layout / thor_hip_get_recon_layout for an RGB frame: same return values (0; 1 for a bad argument, a refused format or a base
 * pointer that is not sample-aligned - found before the device is touched), same ordering, synchronous at return on the library's stream.  A host
 * frame is copied once into the device buffer the encoder keeps for layouts; a device frame is read (written) in place.  Rows that are 16-byte
 * aligned (4-byte aligned for RGB / BGR) move in whole vectors, anything else sample by sample. */
int thor_hip_stage_frame_rgb(thor_hip_encoder* e, int stream, int slot, const void* frame, const thor_hip_rgb_format* fmt, int on_device);
int thor_hip_get_recon_rgb(thor_hip_encoder* e, int stream, void* frame, const thor_hip_rgb_format* fmt, int on_device);

/* Frames of another size: staging resamples them to the encoder's width x height on the device (k_scale_in), so that one decoder surface can feed
 * engines at several sizes and a source whose size is no multiple of 8 can be coded at the nearest legal size.  Staging a scaled frame means exactly:
 * (1) resample the source - a 4:2:0 frame of input_bitdepth samples, src_width x src_height, in `layout` at the SOURCE size - to a planar 4:2:0 frame
 * of input_bitdepth samples at width x height (below), and (2) stage that frame, so every sample is then widened by bitdepth - input_bitdepth like
 * any staged frame.  Integers only; nothing of it is floating point, on the host or on the device.
 *
 * Each plane is resampled separably, horizontally first, then vertically.  Luma: S -> T is src_width -> width and src_height -> height; chroma:
 * src_width / 2 -> width / 2 and src_height / 2 -> height / 2.
 * Taps.  For one axis with source length S, destination length T, D = 2 * max(S, T) and destination index i, the distance numerator of source
 * sample k is
 *   centre-aligned: n(k) = (2i + 1) * S - (2k + 1) * T          co-sited: n(k) = 2 * (i * S - k * T)
 * Co-sited is used only for the horizontal axis of chroma when chroma_site == 1 (left, the MPEG-2 / H.264 default, as in thor_hip_rgb_format);
 * everything else is centre-aligned.  The filter argument is n / D: the support stretches with the ratio when downscaling (which anti-aliases) and is
 * one source sample wide when upscaling.  The taps are all k with a = |n(k)| < A * D, a contiguous range.  Weights, in exact 64-bit integers:
 *   THOR_HIP_SCALE_BILINEAR (A = 1): W = D - a
 *   THOR_HIP_SCALE_BICUBIC (Catmull-Rom, A = 2): a < D: W = 3a^3 - 5a^2 D + 2D^3;  otherwise W = -a^3 + 5a^2 D - 8a D^2 + 4D^3
 * Coefficients: c(k) = floor((2 * W(k) * 16384 + sumW) / (2 * sumW)), sumW the sum over the taps (floor, not truncation: W can be negative); then
 * 16384 - sum c is added to the tap with the largest W, the lowest k among equals, so every tap set sums to 16384 exactly.  A tap outside
 * [0, S - 1] reads the edge sample.  S == T gives the single tap 16384 at k = i: a scaled call at the coded size is layout staging, exactly.
 * Passes, with g = 2 guard bits, n = input_bitdepth and x = s >> msb as in layout staging:
 *   horizontal: I = (sum c(k) * x(k) + (1 << (13 - g))) >> (14 - g)          (arithmetic shift; I is signed)
 *   vertical:   O = clamp((sum c(k) * I(k) + (1 << (13 + g))) >> (14 + g), 0, 2^n - 1)
 * Limits, refused before the device is touched: src_width and src_height even and within 16 .. 8192; on each axis S <= 8 * T and T <= 8 * S (at most
 * 33 taps); an unknown filter or site; a layout that is refused at the source size; and, when a table is built, a tap set with sum |c| > 26214
 * (with that bound I fits 16 bits and the vertical sum 32 bits at n = 12).  RGB sources are not scaled.  There is no scaled fetch: reconstruction and
 * PSNR are at the coded size, against the staged (scaled) original. */
enum { THOR_HIP_SCALE_BILINEAR = 0, THOR_HIP_SCALE_BICUBIC = 1 };
typedef struct thor_hip_scale {
  int size;         /* sizeof(thor_hip_scale) */
  int src_width;    /* of the frame handed over */
  int src_height;
  int filter;       /* THOR_HIP_SCALE_* */
  int chroma_site;  /* 0: centre, 1: left - the horizontal position of the chroma samples, in the source and in the result */
} thor_hip_scale;
/* Bytes the source frame spans from its base in `layout` (NULL = packed planar) at the source size; 0 = refused (see the limits above; a table is not
 * built).  thor_hip_scale_bytes_for needs no encoder and no device. */
size_t thor_hip_scale_bytes(const thor_hip_encoder* e, const thor_hip_scale* scale, const thor_hip_frame_layout* layout);
size_t thor_hip_scale_bytes_for(int width, int height, int input_bitdepth, const thor_hip_scale* scale, const thor_hip_frame_layout* layout);
/* thor_hip_stage_frame_layout for a frame of another size: same return values (0; 1 for a bad argument, a refused scale or layout or a base pointer
 * that is not sample-aligned - found before the device is touched, and the slot stays as it was), same ordering, synchronous at return.  The encoder
 * keeps the tap tables of the most recent (source size, filter, site) and rebuilds them only when those change. */
int thor_hip_stage_frame_scaled(thor_hip_encoder* e, int stream, int slot, const void* frame, const thor_hip_scale* scale,
                                const thor_hip_frame_layout* layout /* at the SOURCE size; NULL = packed planar */, int on_device);
/* No device: the taps of destination index i on one axis (S -> T).  *first = the first source index (negative at the left edge), coeff[0 .. count - 1]
 * the coefficients.  Returns the count; 0 = refused (S or T outside 1 .. 8192, ratio above 8, unknown filter, i outside [0, T), cap too small). */
int thor_hip_scale_taps(int S, int T, int filter, int cosited, int i, int* first, short* coeff, int cap);

/* Rate control: a target bitrate per stream.  This is the library's own rate control, not the reference's (-bitrate / -max_delta_qp change the QP after every
 * superblock in raster order and stay refused, thor_hip_params_set returns 2): it picks ONE base QP per frame, so every frame is exactly what the block path
 * produces at that QP, the stream is an ordinary Thor stream and the reference decoder reproduces the reconstruction.  Integers only, except the one line that
 * forms T; everything below is normative, and tests/rc_model.py restates it.
 *
 * Analysis (k_rc_cost, one launch per group of frames, before the frame's jobs are set up; nothing is launched for a stream without rate control).  The luma of
 * the staged original at the engine's depth is halved: h(x, y) = (Y(2x, 2y) + Y(2x + 1, 2y) + Y(2x, 2y + 1) + Y(2x + 1, 2y + 1) + 2) >> 2, a plane of width / 2 x
 * height / 2 samples kept per stream until the next frame's analysis (two planes alternate).  That plane is cut into 8x8 blocks from its top-left corner; width and height
 * are multiples of 8, so a block at the right / bottom edge may be 4 wide / high and is evaluated on the n samples inside the plane.  Per block:
 *   intra = sum |h - m|, m = (sum h + n / 2) / n                                    (integer division)
 *   inter = min over (dx, dy) in [-8, 8]^2 of sum |h(x, y) - h_prev(x + dx, y + dy)|, over the vectors whose displaced block lies wholly inside the previous
 *           plane (no padding; the zero vector always does).  h_prev: the plane of the frame analysed before this one for the stream, in CODING order.  The first
 *           frame of a stream, and the first after thor_hip_begin_sequence or thor_hip_set_rate_control, has none: inter = intra.
 * Per frame three exact 64-bit sums over the blocks: sum_intra = sum intra, sum_best = sum min(intra, inter), n_intra = the number of blocks with intra < inter.
 *
 * Controller, per stream.  T = (long long)((double)bitrate / (double)frame_rate), at least 1; B = bitrate * buffer_ms / 1000, at least 1.  State, all zero when
 * a sequence begins: fullness F, the overflow count, the frame count, and per frame class c (0: I, 1: P, 2..5: B of level 0, 1, 2, 3 and deeper) a count n[c], a
 * factor f[c] (Q16) and an average a[c] of the frame's bits.  step(q) = 2^((q - 4) / 6) in Q16, the 52 literal values of thor_amd/csrc/tk_rc.h.  A frame's cost
 * is sum_intra for an I frame and sum_best otherwise, clamped to 1 .. 2^36; with factors of at most 2^26 no product below reaches 2^63.  All divisions are integer divisions of non-negative values, except F / span, which rounds
 * towards zero.
 *   qp(b)      the QP of the frame at base QP b: the reference's per-frame formula (enc/mainenc.c:281-314: dqpI; mqpP / dqpP off the HQperiod grid; mqpB* / dqpB* by
 *              B level; clamped to 0..51) with b in the place of -qp.  Without rate control b is -qp itself: the same function serves both.
 *   decision   the stream's first frame: b = initial_qp (0: the parameter set's qp).  Otherwise with [lo, hi] = [min_qp, max_qp] ([min_qp_i, max_qp_i] for an I frame):
 *                budget = T * 4 for an I frame; T * a[c] / max(1, (sum over c' >= 1 of n[c'] * a[c']) / (sum of n[c'])) when n[c] > 0; else T
 *                budget = max(budget - F / max(1, B / (2 * T)), T / 8)               (the fullness is paid back over half the buffer)
 *                b = the lowest b in [lo, hi) with (n[c] > 0 ? f[c] : f0[c]) * cost / step(qp(b)) <= budget, else hi;   f0 = {296000, 217000, 216000, 188000, 174000, 174000}
 *   update     after the frame is coded at q = qp(b) with `bits` bits (thor_hip_frame_stats.num_bits: without the 4-byte framing and the sequence header):
 *                o = clamp(bits * step(q) / cost, 1, 2^26);   f[c] = n[c] > 0 ? (f[c] + o) / 2 : o;   a[c] = n[c] > 0 ? (3 * a[c] + bits) / 4 : bits;   n[c] += 1;
 *                when the n sum to 65536 each becomes (n + 1) / 2;   F = max(F + bits - T, -B);   a frame that ends with F > B counts as an overflow.
 * The chosen QP is the frame's QP everywhere: block decisions and lambda, deblocking, CDEF, CLPF, the frame header, thor_hip_frame_stats.qp and the report. */
typedef struct thor_hip_rate_control {
  int size;         /* sizeof(thor_hip_rate_control) */
  int bitrate;      /* bits per second; 0 = off */
  int buffer_ms;    /* the virtual buffer in milliseconds of the bitrate; 0 = 1000 */
  int min_qp;       /* base QP range of inter frames; min_qp == max_qp == 0 means 0..51 */
  int max_qp;
  int min_qp_i;     /* the same for I frames */
  int max_qp_i;
  int initial_qp;   /* base QP of the first frame of a sequence; 0 = the parameter set's qp */
} thor_hip_rate_control;
/* 0 when thor_hip_set_rate_control would accept *rc (NULL included: it means off); 1 otherwise: `size` is wrong, a value is negative, a minimum is above its
 * maximum, a QP is above 51.  Needs no encoder and no device. */
int thor_hip_rate_control_check(const thor_hip_rate_control* rc);
/* Turn rate control on for one stream (each stream has its own target; NULL or bitrate 0: off).  Legal before the stream's first frame and right after
 * thor_hip_begin_sequence, which keeps the target and restarts the controller.  Returns 0; 1 for a bad argument or a refused *rc, 2 when the stream is in the
 * middle of a sequence - nothing is touched then.  While it is off for every stream the encoder launches, copies, allocates and synchronises exactly as before. */
int thor_hip_set_rate_control(thor_hip_encoder* e, int stream, const thor_hip_rate_control* rc);
typedef struct thor_hip_frame_rc {
  int base_qp;                     /* the controller's choice; thor_hip_frame_stats.qp is qp(base_qp) */
  int frame_class;                 /* 0: I, 1: P, 2..5: B of level 0, 1, 2, 3 and deeper */
  unsigned long long sum_intra, sum_best, n_intra;
  long long fullness;              /* F after this frame */
  long long buffer_bits;           /* B */
  long long target_bits;           /* T */
  int overflows;                   /* frames so far that ended with F > B */
} thor_hip_frame_rc;
/* Record i (coding order, the index of thor_hip_get_frame_stats) of a rate-controlled stream.  Returns 0; 1 on a bad argument or a stream without rate control. */
int thor_hip_get_frame_rc(const thor_hip_encoder* e, int stream, int i, thor_hip_frame_rc* out);

/* Key frames: where a stream may be entered.  Low-delay parameter sets only (num_reorder_pics == 0): for a hierarchical-B set every entry point below returns 2
 * and touches nothing.  A promoted frame is exactly the I frame -intra_period would have made at its place (frame type I, the I rule of qp(b), no references,
 * lambda_coeffI, the I frame's number of intra modes) and later frames drop every reference older than it; nothing else of the schedule moves - the coded-frame
 * count, the HQperiod phase of later frames and the distance to the last P or I frame run on.  So -intra_period 0 with key frames asked for at 0, 4, 8 ... is
 * byte for byte the stream of -intra_period 4.
 *
 * thor_hip_force_key_frame: frame display_index of the stream's chunk (what thor_hip_next_frame reports; for low delay the coded index) becomes a key frame.  The
 * frame must not be coded yet - one that thor_hip_next_frame has already handed out still qualifies.  Up to 64 requests may be pending per stream; a frame asked
 * for twice counts once, a request leaves the set when its frame is scheduled, thor_hip_begin_sequence empties the set.  A request for a frame the schedule makes
 * an I frame anyway is accepted and changes nothing.  Returns 0; 1: bad argument, a frame outside the chunk or already coded, a full set; 2: not low delay. */
int thor_hip_force_key_frame(thor_hip_encoder* e, int stream, int display_index);
/* Scene cuts, per stream.  The analysis is the one of rate control above (k_rc_cost, the same two half-size planes per stream): a stream with scene cuts on is
 * analysed before each of its frames whether it is rate-controlled or not, I frames included, so that the next frame has its predecessor.  Normative, integers
 * only: a P frame of the stream is promoted if and only if
 *   its analysis had a previous plane (not the first frame after thor_hip_begin_sequence, thor_hip_set_rate_control or thor_hip_set_scene_cut),
 *   frame_num - last_intra >= max(1, min_interval)                      (last_intra: the frame number of the stream's last I frame of any origin), and
 *   sum_intra > 0 and sum_best * 100 >= (unsigned long long)percent * sum_intra.
 * The sums are below 2^36 (an 8192 x 8192 frame of 12-bit samples: 2^24 half-size samples of at most 2^12 each) and percent <= 100 < 2^7: both products stay
 * below 2^43.  Per stream the order is analysis, cut decision and promotion, and only then the rate controller's decision: a promoted frame is class 0 there
 * (cost sum_intra, budget 4 T, the I range of base QPs) and updates f[0], a[0], n[0].  tests/key_model.py restates the rule.
 * There is no default for percent: what separates a cut from motion depends on the content. */
typedef struct thor_hip_scene_cut {
  int size;           /* sizeof(thor_hip_scene_cut) */
  int percent;        /* 1 .. 100; 0 = off */
  int min_interval;   /* >= 0: frames since the last I frame before a cut may be declared (0 acts as 1) */
} thor_hip_scene_cut;
/* 0 when thor_hip_set_scene_cut would accept *sc (NULL included: off); 1 otherwise: `size` is wrong, percent outside 0 .. 100, min_interval negative.  Needs no
 * encoder and no device. */
int thor_hip_scene_cut_check(const thor_hip_scene_cut* sc);
/* Legal where thor_hip_set_rate_control is: before the stream's first frame and right after thor_hip_begin_sequence, which keeps the setting.  Returns 0; 1 for
 * a bad argument or a refused *sc; 2 in the middle of a sequence or when the parameter set is not low delay.  While no request is pending and scene cuts are off
 * for every stream the encoder launches, copies, allocates and synchronises exactly as before. */
int thor_hip_set_scene_cut(thor_hip_encoder* e, int stream, const thor_hip_scene_cut* sc);
/* The analysis as a call of its own, for a caller that keeps the rungs of a ladder aligned: analyse one rung, apply the rule above, and call
 * thor_hip_force_key_frame on every rung.  sums = sum_intra, sum_best, n_intra of the STAGED original in `slot` against the one in prev_slot (-1: no
 * predecessor, inter = intra) - bit for bit what the stream's own analysis finds for the same two frames.  The kernel's second instantiation halves the
 * previous original while it loads it: neither the stream's two half-size planes nor its controller are touched, and the call may come at any time between
 * encode calls.  Returns 0; 1: bad argument or a slot that is not staged; 2: not low delay. */
int thor_hip_scene_cost(thor_hip_encoder* e, int stream, int slot, int prev_slot, unsigned long long sums[3]);
typedef struct thor_hip_frame_key {
  int reason;                      /* 0: the schedule's own frame type; 1: a forced key frame; 2: a scene cut.  1 when both apply */
  unsigned long long sum_intra, sum_best, n_intra;   /* the frame's analysis; zero when the frame was not analysed */
} thor_hip_frame_key;
/* Record i (coding order, the index of thor_hip_get_frame_stats) of a stream.  Returns 0; 1 on a bad argument. */
int thor_hip_get_frame_key(const thor_hip_encoder* e, int stream, int i, thor_hip_frame_key* out);

/* Temporal noise filter: the staged original of one frame filtered against up to four other staged originals of the same stream - past and / or future frames -
 * with block motion compensation, into another staging slot at the engine's depth.  The filter is NOT recursive: its inputs are originals only and its output is
 * a pure function of them.  A filtered frame is an ordinary staged frame: the encoder codes it like any other, and every frame's distortion (sse, psnr, the
 * report) is measured against the slot that was coded - the FILTERED frame, not the source.  Integers only; everything below is normative, and
 * tests/tf_model.py restates it.  s = strength (1 .. 16), sh = bitdepth - 8; samples are at the engine's depth (after the widening of a lower input depth).
 *
 * Luma search.  The luma plane is cut into 8x8 blocks (width and height are multiples of 8).  For each neighbour k the block's vector is the candidate (dx, dy)
 * of [-8, 8]^2, full-pel, with the least (SAD, rank): SAD = sum |cur(x, y) - nb_k(x + dx, y + dy)| over the block; rank = 0 for the zero vector, otherwise
 * 1 + (dy + 8) * 17 + (dx + 8).  A candidate whose displaced block leaves the plane is skipped (no padding; the zero vector never is).  Flat content therefore
 * keeps the zero vector, and the order of the candidates is total.
 * Block weight.  m = SAD >> sh, Tb = 128 * s, wb = B[dist] * max(0, Tb - m) / Tb (integer division), B[1] = 192, B[2] = 128 (Q8), dist = ref_dist[k].
 * A neighbour that does not show the scene (beyond a scene cut, say) matches no block within Tb - an average difference of 2 s per sample - so every wb is 0
 * and the frame comes out unchanged.
 * Sample weight.  For the current sample c and the motion-compensated neighbour sample r = nb_k(x + dx, y + dy): d = |c - r| >> sh, Ts = 4 * s,
 * ws = max(0, Ts - d), w = wb * ws.
 * Output sample.  (c * W0 + sum_k r_k * w_k + D / 2) / D with W0 = 256 * Ts and D = W0 + sum_k w_k (integer division of non-negative values).  D <= 2^16 and
 * the numerator stays below 2^29: 32 bits suffice.  Identical neighbours give back c exactly; nrefs = 0 copies the frame.
 * Chroma.  Each 8x8 luma block owns one 4x4 block per chroma plane; its vector is (dx >> 1, dy >> 1) with arithmetic shifts, full-pel - that block lies inside
 * the chroma plane whenever the luma block lies inside the luma plane; it takes the same wb, and ws comes from the chroma difference.
 * Sub-pel vectors, a hierarchical search and overlapped blocks are deliberately left out.
 * Device: k_tf_search (one workgroup per 32x32 luma tile and neighbour, the tile and the neighbour's 48x48 window in LDS, one lane per candidate) and
 * k_tf_blend (one lane per four samples): two launches for all requests of a call, one synchronisation. */
typedef struct thor_hip_temporal_filter {
  int size;       /* sizeof(thor_hip_temporal_filter) */
  int strength;   /* 1 .. 16 */
} thor_hip_temporal_filter;
typedef struct thor_hip_tf_request {
  int stream;
  int dst_slot;      /* receives the filtered frame; allocated on demand like any slot */
  int slot;          /* the frame to filter */
  int nrefs;         /* 0 .. 4 */
  int ref_slot[4];   /* the neighbours, staged originals of the same stream */
  int ref_dist[4];   /* their temporal distance from `slot`, 1 or 2, in either direction */
} thor_hip_tf_request;
/* 0 when thor_hip_filter_staged would accept *tf; 1 otherwise: NULL, a wrong `size`, a strength outside 1 .. 16.  Needs no encoder and no device. */
int thor_hip_temporal_filter_check(const thor_hip_temporal_filter* tf);
/* Filter `n` requests in one call - different streams, or several frames of one stream; a request's neighbour may be another request's source.  Synchronous at
 * return.  Returns 0; 1 for a bad argument (n outside 1 .. 4096, a stream, nrefs or ref_dist out of range), a refused *tf, a source or neighbour slot that is
 * not staged, a dst_slot that is a source or a neighbour of any request of the call, or two requests of one stream with the same destination - all found before
 * the device is touched, and nothing is written or allocated then.  While nobody calls it the encoder launches, copies, allocates and synchronises exactly as
 * before. */
int thor_hip_filter_staged(thor_hip_encoder* e, const thor_hip_tf_request* req, int n, const thor_hip_temporal_filter* tf);
/* The staged frame in `slot`, as it would be coded: packed planar 4:2:0 at the ENGINE's depth (bytes for bitdepth 8, little-endian uint16 otherwise: width *
 * height * 3 / 2 samples).  Returns 0; 1 for a bad argument or a slot that is not staged. */
int thor_hip_get_staged(thor_hip_encoder* e, int stream, int slot, void* yuv_out);

/* HIP-event time (ms) and launch count of the superblock kernel accumulated since the last
 * reset; used by bench.py for the roofline figure. */
void thor_hip_kernel_time(thor_hip_encoder* e, double* sb_ms, long* sb_launches, double* filter_ms);
void thor_hip_kernel_time_reset(thor_hip_encoder* e);
/* Content statistics of the inter frames coded since the last reset ("always log the fraction of SBs that
 * early-skipped"; reference shortcut enc/encode_block.c:2231,2440-2480): out[0] luma pixels coded by the early-skip
 * shortcut (any block size), out[1] superblocks early-skipped as a whole, out[2] superblocks processed, out[3] luma
 * pixels processed.  reset != 0 clears the counters. */
void thor_hip_read_stats(thor_hip_encoder* e, unsigned long long out[4], int reset);
/* Per-frame log and the encoder report (enc/mainenc.c:219-226, :553-591, :642-666).  Every coded frame of a stream appends one record
 * (thor_hip_begin_sequence empties the log).  With frame distortion on, one more kernel per frame group sums (original - final
 * reconstruction)^2 per plane on the device - after deblocking, CDEF and CLPF - and the sums travel with the frame's bit counts; off (the
 * default) a frame's launches and copies are unchanged and sse / psnr stay 0 (the reference's -snrcalc 0). */
void thor_hip_set_frame_distortion(thor_hip_encoder* e, int on);
typedef struct thor_hip_frame_stats {
  int display_index;          /* absolute input frame index, as the reference prints it (the -skip 3 chunk starts at 3) */
  int frame_type;             /* 0 = I, 1 = P, 2 = B */
  int qp;
  int num_bits;               /* bits of the frame before the 4-byte framing; the sequence header is not counted */
  int num_ref;
  int ref_array[4];           /* window indices as coded; -1 = the interpolated frame, built from the next two entries */
  int ref_frame_num[4];       /* chunk-relative frame number of the frame each ref_array entry points at (-1 for the -1 entry) */
  int has_sse;                /* 1 when the frame's distortion was measured */
  unsigned long long sse[3];  /* Y, U, V: exact sums of squared differences, at the input bit depth */
  double psnr[3];             /* snr_yuv's formula on sse (common/snr.c:32-99), maxsignal from input_bitdepth; inf when sse == 0; 0 when not measured */
} thor_hip_frame_stats;
int thor_hip_frame_stats_count(const thor_hip_encoder* e, int stream);
/* Record i (coding order) of a stream.  Returns 0, 1 on a bad argument. */
int thor_hip_get_frame_stats(const thor_hip_encoder* e, int stream, int i, thor_hip_frame_stats* out);
/* The reference's stdout for the stream so far, byte for byte ("SH:" line, one line per coded frame, average block), written to buf like
 * snprintf: at most n bytes including the terminating NUL; returns the length of the whole report. */
int thor_hip_report(const thor_hip_encoder* e, int stream, char* buf, size_t n);
/* The line the reference appends to its -stat file for the stream so far (without the header " NFR     kbps     PSNRY  PSNRU  PSNRV"
 * that starts a new file); num_frames: the -n value.  snprintf semantics as above. */
int thor_hip_stat_line(const thor_hip_encoder* e, int stream, int num_frames, char* buf, size_t n);

/* Development aid: 32 shader-cycle / event counters summed over all superblock wavefronts (all zero unless
 * the library was built with -DTHOR_PROF). */
void thor_hip_read_prof(thor_hip_encoder* e, long long out[32]);

/* ---- (3) kernel-level batch entry points (known-answer tests) ------------------------------- */
/* SAD of `n` candidate positions: org is a compact w x h block (stride w); ref points at the
 * frame sample co-located with the block, stride rstride; cand[2*i],cand[2*i+1] = full-pel (dx,dy).
 * w, h: powers of two >= 4 (PU sizes).  Follows sad_calc (enc/encode_block.c:417-428). out[i] = SAD. */
int thor_hip_sad_batch(const uint8_t* org, int w, int h, const uint8_t* ref_plane, int plane_w, int plane_h,
                       int rstride, int bx, int by, const int* cand, int n, uint32_t* out);
/* Quarter-pel luma prediction (get_inter_prediction_luma, common/inter_prediction.c:117-181) of a
 * w x h block at (bx,by) for `n` motion vectors (mv[2*i]=x, mv[2*i+1]=y in 1/4 pel); out: n*w*h. */
int thor_hip_interp_luma(const uint8_t* ref_plane, int plane_w, int plane_h, int rstride, int pad, int bx, int by,
                         int w, int h, const int16_t* mv, int n, int bipred, uint8_t* out);
/* residual -> transform -> quantize -> dequantize -> inverse -> reconstruct of `n` size x size
 * blocks (transform.c:245, encode_block.c:84, common_block.c:45/75, transform.c:467).
 * org/pred/rec: n*size*size samples; coefq: n*min(size,16)^2; cbp: n flags. */
int thor_hip_code_tu_batch(const uint8_t* org, const uint8_t* pred, int size, int qp, int coeff_type, int fast, int n,
                           int16_t* coefq, uint8_t* rec, int* cbp);
/* In-loop deblocking of one 8-bit planar 4:2:0 frame in place (deblock_frame_y + deblock_frame_uv,
 * common/common_frame.c:47,354; chroma QP through chroma_qp[]).  cells: (height/4) x (width/4) records, the
 * device-side compact form of deblock_data_t (common/types.h:178-187): mode = block_mode_t, size = CB size,
 * tbpb = tb_split | pb_part << 1, cbp bit 0/1/2 = Y/U/V coefficients present. */
typedef struct thor_hip_cell {
  int16_t mv0x, mv0y, mv1x, mv1y;
  uint8_t mode, size, tbpb, cbp;
  int8_t ref0, ref1, dir;
  uint8_t pad;
} thor_hip_cell;
int thor_hip_deblock_frame(uint8_t* yuv, int width, int height, int qp, const thor_hip_cell* cells);

/* The same four entry points on 16-bit samples = the reference's _hbd instances (SAMPLE = uint16_t: enc/enc_kernels_hbd.c,
 * common/inter_prediction_hbd.c, common/common_block_hbd.c, common/common_frame_hbd.c); bitdepth 9..12, strides and sizes in
 * samples.  Known answers recorded from those reference functions: tests/golden/kat4.npz (bitdepth 10). */
int thor_hip_sad_batch_hbd(const uint16_t* org, int w, int h, const uint16_t* ref_plane, int plane_w, int plane_h,
                           int rstride, int bx, int by, const int* cand, int n, uint32_t* out);
int thor_hip_interp_luma_hbd(const uint16_t* ref_plane, int plane_w, int plane_h, int rstride, int pad, int bx, int by,
                             int w, int h, const int16_t* mv, int n, int bipred, int bitdepth, uint16_t* out);
int thor_hip_code_tu_batch_hbd(const uint16_t* org, const uint16_t* pred, int size, int qp, int coeff_type, int fast, int n,
                               int bitdepth, int16_t* coefq, uint16_t* rec, int* cbp);
int thor_hip_deblock_frame_hbd(uint16_t* yuv, int width, int height, int qp, int bitdepth, const thor_hip_cell* cells);

/* ---- (3b) round 6: known-answer entry points for the remaining sample kernels.  `bitdepth` 8: samples are uint8_t (the reference's _lbd
 * instances); 9..12: uint16_t (_hbd).  Every call runs the device function the encoder itself calls, one wavefront per item; known answers are
 * recorded from the reference functions named below (tests/golden/gen_kat5.py -> kat5.npz).  Return 0, 1 = bad argument, 2 = an item reads outside
 * the given frame, 3 = no usable device. */
/* make_top_and_left + get_intra_prediction (common/intra_prediction.c:57-183, :403-428) of `n` transform units of `size` x `size` samples.
 * plane: a reconstructed plane (stride in samples).  par[7*i..]: ypos, xpos of the CODING block, its upright / downleft availability, the intra
 * mode (0..9), and the unit's offset (i, j) inside the block.  tb_split 0: the unit IS the block (i = j = 0).  tb_split 1: the block is
 * 2*size wide, rblocks holds `n` block-local reconstructions of (2*size)^2 samples (what the units coded earlier left there).  out: n*size*size. */
int thor_hip_kat_intra(const void* plane, int width, int height, int stride, int bitdepth, int size, int tb_split, int n, const int* par,
                       const void* rblocks, void* out);
/* get_inter_prediction_yuv (common/inter_prediction.c:185-226: clip_mv, quarter-pel luma, eighth-pel chroma, one PU or four quadrant PUs) of `n`
 * blocks of `size` from a planar 4:2:0 reference frame (the library pads it like a reference picture).  par[5*i..]: ypos, xpos, sign,
 * enable_bipred, split; mv[8*i..]: four vectors (x, y).  out: n blocks of size*size luma + 2 * (size/2)^2 chroma samples. */
int thor_hip_kat_inter_yuv(const void* yuv, int width, int height, int bitdepth, int size, int n, const int* par, const int16_t* mv, void* out);
/* average_blocks_all (common/inter_prediction.c:228-247): truncating average of two yuv blocks (layout as above). */
int thor_hip_kat_average(const void* a, const void* b, int size, int bitdepth, int n, void* out);
/* improve_uv_prediction (common/common_block.c:347-428), 4:2:0: y = luma prediction, ry = reconstructed luma (both n_luma^2, stride n_luma),
 * uv = chroma predictions U then V ((n_luma/2)^2 each), updated in place. */
int thor_hip_kat_cfl(const void* y, void* uv, const void* ry, int n_luma, int bitdepth, int n);
/* cdef_find_dir (common/common_block.c:94-162) on `n` 8x8 blocks (64 samples each, coeff_shift = bitdepth - 8). */
int thor_hip_kat_cdef_dir(const void* blocks, int bitdepth, int n, int* dir, int* var);
/* cdef_filter_block (common/common_block.c:224-279) of `n` bsize x bsize blocks (8 luma, 4 chroma) of a plane; samples outside the plane count as
 * CDEF_VERY_LARGE (cdef_prepare_input, common/common_frame.c:766).  par[7*i..]: x0, y0, pri_strength, sec_strength, dir, pri_damping, sec_damping. */
int thor_hip_kat_cdef_filter(const void* plane, int width, int height, int stride, int bitdepth, int bsize, int n, const int* par, void* out);
/* The CDEF strength search and frame filter (cdef_search + cdef_frame for the three planes, enc/encode_frame.c:228-489, :768-774, common/common_frame.c:826-1003)
 * of `n_jobs` frames of one size through the encoder's own launch sequence (copy, flags, direction / variance, distortions, joint strength selection, apply -
 * one launch each for all jobs).  rec_yuv / org_yuv: n_jobs packed planar 4:2:0 frames (deblocked / original); mode: per job (height / 4) x (width / 4)
 * block_mode_t bytes; qp, speed, cdef_bits: one entry per job - speed = -cdef minus 1 (0..2), cdef_bits the frame-level guess (0 = fixed strengths from qp); damping 5.  Returned per job: dir (int8) and
 * var per 8x8 luma block in raster order (0 where the passes wrote none); fb_compact per 64x64 filter block (its index among the live ones or -1); mse
 * [2][filter blocks][64]; result = 34 ints: nb_bits, strengths[8], uv_strengths[8], sb_count, 16 ints of scratch; fb_sel per filter block (the preset chosen);
 * out_yuv: the filtered frames.  width, height: multiples of 8, at least 8; qp 0..51; cdef_bits 0..3.  Known answers: tests/golden/gen_kat10.py -> kat10.npz. */
int thor_hip_kat_cdef_frame(int n_jobs, const void* rec_yuv, const void* org_yuv, const uint8_t* mode, int width, int height, int bitdepth, const int* qp,
                            const int* speed, const int* cdef_bits, int8_t* dir, int* var, int* fb_compact, unsigned long long* mse, int* result, int* fb_sel, void* out_yuv);
/* CLPF on one planar 4:2:0 frame: the per-8x8-block squared errors of detect_multi_clpf (enc/encode_block.c:2556-2621; stats[4*b..]: unfiltered,
 * strength 1, 2, 4; blocks in luma raster order, then U, then V; a block whose top-left cell is skip-coded reports {0, 0xffffffff, 0, 0}) and the
 * filtered frame of clpf_frame / clpf_block (common/common_frame.c:1005-1163, common/common_block.c:325-345) for the given per-plane strengths
 * (0 = off, else 1 / 2 / 4), luma filter-block size 1 << fb_log2 and per-filter-block switches fb_on. */
int thor_hip_kat_clpf(const void* rec_yuv, const void* org_yuv, int width, int height, int bitdepth, int qp, const thor_hip_cell* cells,
                      const int* strength, int fb_log2, const uint8_t* fb_on, uint32_t* stats, void* out_yuv);
/* interpolate_frames(new, ref0, ref1, 2, 1) (common/temporal_interp.c:909: the frame half way between two reference pictures; luma pyramid,
 * block motion estimation per level, merge, motion-compensated average) through the engine's own device path (tk_interp_dev.h). */
int thor_hip_kat_interpolate(const void* yuv0, const void* yuv1, int width, int height, int bitdepth, void* out_yuv);
/* The same path stage by stage, for `n_streams` (1..4) reference pairs of one geometry in ONE Engine::make_interp_frames call (every launch covers all streams;
 * each stream has its own row dispenser and progress counters).  yuv0 / yuv1: n_streams packed planar 4:2:0 frames each.  levels: the number of pyramid
 * levels, min(4, (int)(log2(min(width, height)) - 4)) - the caller sizes the buffers with it, a different count in the engine returns 2.  Copied back per
 * stream, streams one after the other:
 *   pyramid     reference 0 then 1, for each level l = 1 .. levels-1 its luma plane with the padding of 32: (height >> l) + 64 rows of (width >> l) + 64 samples;
 *   nmv         for each level l = 0 .. levels-1 the final fields nmv[0] then nmv[1] (after the merge pass): bw * bh (x, y) pairs each, bw = 2 * ceil((width >> l) / 16);
 *   out_padded  the interpolated picture with its borders: Y (height + 320 rows of width + 320), then U and V (height / 2 + 160 rows of width / 2 + 160).
 * width, height: multiples of 8, 64..8192.  Known answers recorded from the reference stage by stage: tests/golden/gen_kat12.py -> kat12*.npz. */
int thor_hip_kat_interp_stages(int n_streams, const void* yuv0, const void* yuv1, int width, int height, int bitdepth, int levels, void* pyramid, int16_t* nmv,
                               void* out_padded);

/* The motion search of one prediction unit - motion_estimate (enc/encode_block.c:517-711: telescope, candidate list incl. the 5-offset widesad of 16x16
 * blocks, hexagon refinement, half- and quarter-pel passes, the encoder_speed 1 / 2 approximations) - on `n` items of one current / reference luma frame pair
 * (width x height samples, no padding: the library pads the reference like a reference picture).  Each item runs the throughput build's device function in a
 * workgroup of one wavefront with the superblock kernel's workspace (LDS search window included).  par[17*i..]: cb_x, cb_y, cb (coding block), pu_dx, pu_dy,
 * pw, ph (prediction unit inside it), mvc.x, mvc.y, mvp.x, mvp.y (quarter-pel), sign, enable_bipred, encoder_speed, ncand, cand_off, stage (1: stage the
 * coding block's search window around mvc first, as the HOR / VER / QUAD searches find it).  lambda[i]: the search's lambda.  cand: ncand_total full-pel list
 * entries (x, y); item i owns [cand_off, cand_off + ncand).  out[3*i..]: mv.x, mv.y, cost.  Known answers recorded from the reference function:
 * tests/golden/gen_kat8.py -> kat8.npz. */
int thor_hip_kat_motion_estimate(const void* cur, const void* ref, int width, int height, int bitdepth, int n, const int* par, const double* lambda,
                                 const int16_t* cand, int ncand_total, int* out);
/* motion_estimate_bi (enc/encode_block.c:798-913): one vector used as +mv on ref0 and -mv on ref1.  par as above (pu = the coding block, stage ignored,
 * cand_off = 6*i); cand: six list slots per item, the first ncand are the list on entry; list_out[12*i..]: the six slots as the call leaves them. */
int thor_hip_kat_motion_estimate_bi(const void* cur, const void* ref0, const void* ref1, int width, int height, int bitdepth, int n, const int* par,
                                    const double* lambda, const int16_t* cand, int* out, int16_t* list_out);
/* The two sub-block tests of the early-skip check (enc/encode_block.c:2146-2229: check_early_skip_sub_block / _sub_blockC as the encoder executes them) on `n`
 * items: chroma[i] 0 luma / 1 chroma, size[i] (luma 8 / 16 / 32, chroma 4 / 8 / 16), qp[i], thr[i] (early_skip_thr); org / pred: n blocks of 32x32 samples
 * holding the size x size block in their top-left corner.  out[i]: 1 = significant.  Known answers: tests/golden/gen_kat7.py -> kat7.npz. */
int thor_hip_kat_early_skip(const int* chroma, const void* org, const void* pred, const int* size, const int* qp, const float* thr, int bitdepth, int n, int* out);
/* The neighbour context of a coding block (thor_amd/csrc/tk_block_ctx.h) on `n` items of one cell grid, one wavefront per item, against the reference's
 * get_mv_pred, get_mv_skip / get_mv_merge (common/inter_prediction.c:413-834), find_block_contexts (common/common_block.c:283) and get_upright_available /
 * get_downleft_available (common/common_block.h:60-95): tests/golden/gen_kat11.py -> kat11.npz.  cells: ncells records in raster order, cell_stride per row
 * (rows past the frame's height / 4 are what a block that hangs over the bottom edge reads).  par[6*i..]: ypos, xpos, size (8..sb), frame width (= 4 *
 * cell_stride), frame height, superblock size (64 / 128); positions lie on the size grid inside the frame and ncells covers the rows down to ypos + size.
 * out[23*i..]: get_mv_pred x, y; number of candidates; candidate 0 and 1 as mv0.x, mv0.y, mv1.x, mv1.y, ref0, ref1, dir (zeros when not returned);
 * ctx_cbp, ctx_index with enable 0, then with enable 1; up-right and down-left availability. */
int thor_hip_kat_block_ctx(const thor_hip_cell* cells, long long ncells, int cell_stride, int n, const int* par, int* out);
/* ssd_part / ssd_total / rd_cost (thor_amd/csrc/tk_block_rd.h) on `n` items against cost_calc (enc/encode_block.c:916-926): tests/golden/gen_kat11.py.  org / rec:
 * pools of nsamp samples; item i owns a compact 4:2:0 block at par's `off` (Y size x size, U, V, stride = size) in both.  par[7*i..]: size (8..128), bw, bh
 * (multiples of 8 up to size: the part inside the frame), nbits (0..2^20), off (multiple of 16), skew (bytes from a 16-byte boundary to the original's first
 * sample, a whole number of samples below 16), stride (of the original's luma rows in samples, even, at least bw).  The originals are laid out as planes with
 * that skew and stride; blocks up to the size the engine keeps in LDS are copied there as the engine does.  out[4*i..]: luma SSD from the global-memory
 * instance, from the LDS instance (all ones for larger blocks), rd_cost, rd_cost with the luma SSD passed in. */
/* Largest coding-block size whose sample buffers this build keeps in LDS (16 or 32): the blocks for which thor_hip_kat_block_cost runs the LDS instances. */
int thor_hip_kat_lds_block(void);
int thor_hip_kat_block_cost(int n, const int* par, const double* lambda, const void* org, const void* rec, long long nsamp, int bitdepth, unsigned long long* out);
/* intra_sad_search (thor_amd/csrc/tk_block_search.h) on `n` items against search_intra_prediction_params (enc/encode_block.c:928-1031): tests/golden/gen_kat11.py.
 * plane: the reconstructed luma plane, width x height samples (multiples of 8), stride = width; org: pool of nsamp samples holding each item's compact original
 * block (stride = size).  par[6*i..]: ypos, xpos (on the size grid, the block inside the plane), size (8..64), superblock size (64 / 128), num_intra_modes
 * (4 / 10), off (multiple of 16).  Up-right / down-left availability comes from the position, as in the encoder.  out[2*i..]: intra mode, SAD. */
int thor_hip_kat_intra_search(int n, const int* par, const void* plane, int width, int height, const void* org, long long nsamp, int bitdepth, int* out);
/* build_org8 (2 * org - pred, saturated: the original of a bi-prediction search step) on `n` items.  org / pred: pools of nsamp samples, item i owns a compact
 * size x size block at par's `off` in both; par[4*i..]: size (8..128), off (multiple of 16), skew, stride (of the original, laid out as for
 * thor_hip_kat_block_cost).  out_global / out_lds: pools of nsamp samples, read and written back whole; the item's result lands at `off` - out_global from the
 * global-memory instance, out_lds from the LDS instance (blocks up to thor_hip_kat_lds_block() only; larger ones leave it untouched). */
int thor_hip_kat_build_org8(int n, const int* par, const void* org, const void* pred, long long nsamp, int bitdepth, void* out_global, void* out_lds);
/* The block syntax writer and its bit counter (thor_amd/csrc/tk_bits.h) on `n` items, one wavefront per item, against bit strings recorded from the reference's
 * put_vlc (enc/putvlc.c:73-160), write_mv (enc/write_bits.c:123-143), write_coeff (:145-241), write_super_mode (:257-358) and write_block (:360-600):
 * tests/golden/gen_kat9.py -> kat9.npz.  Bit strings are arrays of 32-bit words, word w = bits [32w, 32w + 32), first bit in the MSB; every item owns `words`
 * words of each buffer.  Return 0, 1 = bad argument, 2 = an item reaches outside a given buffer, 3 = no usable device.
 * The two syntax entry points run a compilation of tk_bits.h of their own (thor_amd/csrc/thor_hip_katbits.cpp: same source, flags and parameters as the throughput
 * build, kept apart so that the superblock kernels' code stays what it was); the throughput build's own binary of these functions is covered by the stream goldens.
 * write_coeff: par[4*i..]: size (4 .. 128, the transform unit's; min(size, 16)^2 coefficients are coded), type (bit 0 chroma, bit 1 intra block), the bit
 * position the string starts at (0 .. 63), the capacity in bits (<= 32 * words).  coef: 256 coefficients per item, row-major in the first min(size, 16)^2.
 * buf_single / buf_team (in / out, pre-filled by the caller): written by bs_coeff on one lane / by bs_coeff_team on 64 lanes between bs_open and bs_close.
 * out[6*i..]: coeff_bits_team<SP_LDS>, coeff_bits_team<SP_GLOBAL>, final position and overflow flag of bs_coeff, the same of bs_coeff_team. */
int thor_hip_kat_coeff_syntax(int n, const int* par, const int16_t* coef, int words, uint32_t* buf_single, uint32_t* buf_team, int* out);
/* write_block / write_super_mode / one put_vlc codeword / one write_mv.  par[57*i..] and out[10*i..]: the rows thor_amd/csrc/tk_kat_bits.h describes (SynCtx and
 * BlkParam flat, then the index into `pool` of each transform unit's coefficients; counts of bs_block_head_t<false>, of bs_block_t<false, SP_LDS / SP_GLOBAL>
 * without and with ybits, length and overflow flag of the cooperative and of the single-lane emission).  pool: npool blocks of 256 coefficients.  buf_coop /
 * buf_single (in / out): written from bit 0 by bs_block_t<true> with a team / by one lane, capacity 32 * words bits. */
int thor_hip_kat_block_syntax(int n, const int* par, const int16_t* pool, int npool, int words, uint32_t* buf_coop, uint32_t* buf_single, int* out);
/* k_gather_bits, the kernel that concatenates the superblocks' strings into a frame payload: string i = nbits[i] bits starting at word src_off[i] of `src`
 * (src_words words; bits of its last word beyond nbits are arbitrary), placed at bit dst_bit[i] of a zeroed destination of dst_words words.  Return 0, 1 = bad argument, 2 = a string reaches outside
 * `src` or the destination, 3 = no usable device. */
int thor_hip_kat_gather_bits(int n, const uint32_t* src, int src_words, const int* src_off, const int* nbits, const long long* dst_bit, uint32_t* dst, int dst_words);

/* Per-plane sums of squared differences between two planar 4:2:0 frames a and b (w x h; bitdepth 8: bytes, 9..12: uint16_t) through the
 * encoder's own kernel (k_frame_sse): out[0] Y, out[1] U, out[2] V, exact.  w, h: multiples of 8.  Returns 0, 1 = bad argument, 3 = no device. */
int thor_hip_frame_sse(const void* a, const void* b, int w, int h, int bitdepth, unsigned long long out[3]);
/* The three kernels behind input_bitdepth < bitdepth, each on one host frame (packed planar 4:2:0, w and h multiples of 8; input-depth samples are
 * bytes for depth 8 and uint16_t otherwise, engine-depth samples uint16_t).  (bitdepth, input_bitdepth): (10, 8), (12, 8) or (12, 10).
 * Returns 0, 1 = bad argument, 3 = no device.
 * thor_hip_kat_depth_up: read_yuv_frame's widening (common/common_frame.c:491-499), out = in << (bitdepth - input_bitdepth).
 * thor_hip_kat_depth_down: write_yuv_frame's rounding (:557-575), out = saturate((in + half) >> shift, input_bitdepth).
 * thor_hip_frame_sse_depth: the sums of snr_yuv (common/snr.c:39-99) of two frames a and b at `bitdepth`: both rounded as above, then subtracted,
 * squared and added, exact.  With bitdepth == input_bitdepth it is thor_hip_frame_sse. */
int thor_hip_kat_depth_up(const void* in, int w, int h, int bitdepth, int input_bitdepth, uint16_t* out);
int thor_hip_kat_depth_down(const uint16_t* in, int w, int h, int bitdepth, int input_bitdepth, void* out);
int thor_hip_frame_sse_depth(const void* a, const void* b, int w, int h, int bitdepth, int input_bitdepth, unsigned long long out[3]);
/* The two kernels behind thor_hip_stage_frame_layout / thor_hip_get_recon_layout (k_layout_in, k_layout_out) on host buffers, without an encoder.
 * `planar_*`: a packed planar 4:2:0 frame at `bitdepth` (bytes for 8, uint16_t otherwise); `src` / `dst`: thor_hip_layout_bytes_for(w, h,
 * input_bitdepth, layout) bytes in `layout`.  Depths: 8, 10 or 12 with input_bitdepth <= bitdepth.  The device copy of the layout buffer keeps the
 * host pointer's offset from a 16-byte boundary, so a base that is off such a boundary takes the kernel's sample-by-sample path.
 * thor_hip_kat_layout_out's `dst` holds 64 guard bytes after the layout; all of it is uploaded before the kernel runs and downloaded afterwards, so a byte
 * the kernel must not write (row padding, gaps between planes, the guard) comes back as it was.
 * Returns 0, 1 = bad argument or refused layout (before the device is touched), 3 = no device. */
int thor_hip_kat_layout_in(const void* src, const thor_hip_frame_layout* layout, int w, int h, int input_bitdepth, int bitdepth, void* planar_out);
int thor_hip_kat_layout_out(const void* planar_in, const thor_hip_frame_layout* layout, int w, int h, int input_bitdepth, int bitdepth, void* dst);
/* k_scale_in on host buffers without an encoder: `src` holds thor_hip_scale_bytes_for(w, h, input_bitdepth, scale, layout) bytes; planar_out receives
 * the packed planar w x h frame at `bitdepth`.  Same return values. */
int thor_hip_kat_scale_in(const void* src, const thor_hip_scale* scale, const thor_hip_frame_layout* layout, int w, int h, int input_bitdepth, int bitdepth,
                          void* planar_out);
/* k_rc_cost, the frame analysis of rate control, as the engine launches it for two consecutive frames of one stream: first on `prev` (when given) without a
 * previous plane, then on `cur` against the half-size plane the first launch wrote.  cur / prev_or_null: luma planes of w x h samples, w samples per row (bytes
 * for bitdepth 8, uint16_t for 10 / 12); w, h: multiples of 8, at least 16.  out: sum_intra, sum_best, n_intra of `cur`; half_out: its half-size plane, w / 2 x
 * h / 2 samples of the same type.  Returns 0, 1 = bad argument, 3 = no device. */
int thor_hip_kat_rc_cost(const void* cur, const void* prev_or_null, int w, int h, int bitdepth, unsigned long long out[3], void* half_out);
/* The kernel's other instantiation, the one behind thor_hip_scene_cost: one launch on `cur` with `prev_or_null` as a full-size original that the kernel halves
 * while it loads it.  The planes are copied into device frames whose rows start 16-byte aligned, as staged frames do.  Same arguments and return values. */
int thor_hip_kat_scene_cost(const void* cur, const void* prev_or_null, int w, int h, int bitdepth, unsigned long long out[3]);
/* k_tf_search and k_tf_blend, the temporal filter, as the engine launches them for one request.  cur: a packed planar 4:2:0 frame of w x h samples at `bitdepth`
 * (bytes for 8, uint16_t for 10 / 12); refs: nrefs (0 .. 4) such frames one after the other; dists: 1 or 2 each.  The frames are copied into device frames laid
 * out like staging slots.  out: the filtered frame; mv: per neighbour and 8x8 block (raster order) dx, dy; wb: per neighbour and block the block weight - so
 * that a mismatch names its stage.  w, h: multiples of 8, at least 16.  Returns 0, 1 = bad argument, 3 = no device. */
int thor_hip_kat_temporal_filter(const void* cur, const void* refs, const int* dists, int nrefs, int w, int h, int bitdepth, int strength, void* out, int* mv,
                                 int* wb);
/* The same for k_rgb_in / k_rgb_out: `src` / `dst` hold thor_hip_rgb_bytes_for(w, h, fmt) bytes in `fmt` (dst: plus 64 guard bytes, all of it uploaded
 * before the kernel runs and downloaded afterwards); the planar frames are at `bitdepth` (k_rgb_out rounds back to input_bitdepth first).  Any depth
 * of `fmt` goes with any input_bitdepth <= bitdepth.  Same return values. */
int thor_hip_kat_rgb_in(const void* src, const thor_hip_rgb_format* fmt, int w, int h, int input_bitdepth, int bitdepth, void* planar_out);
int thor_hip_kat_rgb_out(const void* planar_in, const thor_hip_rgb_format* fmt, int w, int h, int input_bitdepth, int bitdepth, void* dst);

/* Resources of the persistent superblock kernel (sample_bytes 1: 8-bit kernel, 2: 16-bit kernel, 0: the 8-bit kernel's second build for runs of few
 * streams - 256 registers, two workgroups per CU, chosen by the library when a run cannot fill more; THOR_HIP_KERNEL=std|lat|wide forces one; 3: its third build - eight wavefronts per workgroup, one workgroup per CU, for runs of very few streams) as the HIP runtime reports them: registers per lane,
 * static LDS and private (scratch) bytes, and how many workgroups of it fit one CU - what the resident-workgroup count of every launch derives from. */
int thor_hip_superblock_kernel_info(int sample_bytes, int* num_regs, int* lds_bytes, int* private_bytes, int* workgroups_per_cu);
/* The build of the 8-bit superblock kernel the most recently configured engine launches: 0 = throughput build (168 registers, three four-wavefront
 * workgroups per CU), 1 = latency build (sample_bytes 0 above), 2 = eight wavefronts per workgroup, one workgroup per CU (sample_bytes 3 above: chosen while
 * all streams of a run together offer at most 2.5 superblocks per CU; the latency build runs only when THOR_HIP_KERNEL=lat forces it).  Valid after the engine's first encode call. */
int thor_hip_superblock_kernel_in_use(void);

#ifdef __cplusplus
}
#endif
#endif
