/* thorenc_hip.c - minimal C front end over the libthor_hip.so sequence API (include/thor_hip.h).
 * Usage mirrors the reference Thorenc (enc/strings.c:287-356) for the options this path honours:
 *   thorenc_hip -cf config.txt -if in.yuv -width W -height H -qp Q -n N [-skip K] [-f fps]
 *               [-of str.bit] [-rf rec.yuv] [-streams S] [-snrcalc 0|1] [-stat file] [-pixfmt i420|nv12|nv21|p010|rgba|bgra|rgb24|bgr24] [-name value ...]
 *               [-rgbmatrix 601|709|2020] [-rgbrange limited|full] [-rgbsite centre|left]
 *               [-src_width W -src_height H] [-scale_filter bilinear|bicubic] [-scale_site left|centre]
 *               [-rc_bitrate N] [-rc_buffer_ms M] [-rc_min_qp Q -rc_max_qp Q] [-rc_min_qpI Q -rc_max_qpI Q] [-rc_initial_qp Q]
 *               [-key_frames a,b,c] [-key_scenecut PCT] [-key_min_interval N]
 *               [-tf_strength S] [-tf_past P] [-tf_future F]
 * -pixfmt: the layout of the -if and -rf files, rows tight (default i420: planar).  nv12 / nv21 interleave the chroma samples; p010 does so with
 * the samples in the high bits of 16-bit words and serves any input depth above 8.  The frames are staged and fetched in that layout
 * (thor_hip_stage_frame_layout / thor_hip_get_recon_layout): the device converts.
 * rgba / bgra / rgb24 / bgr24: the files hold RGB frames - one byte per channel with 8-bit input, else 16-bit words with the value in the low
 * bits - converted on the device (thor_hip_stage_frame_rgb / thor_hip_get_recon_rgb) with -rgbmatrix (default 709), -rgbrange (limited) and
 * -rgbsite (left).
 * -src_width / -src_height: the -if frames have that size (in the -pixfmt layout, which must not be RGB) and are resampled to -width x -height on
 * the device while they are staged (thor_hip_stage_frame_scaled; defaults bicubic, left); -rf stays at the coded size.
 * -rc_bitrate N: the library's rate control (thor_hip_set_rate_control) at N bits per second, the same target for every stream; the other -rc_ options are
 * the fields of thor_hip_rate_control.  They are not the reference's -bitrate / -max_qp ..., which stay refused.
 * -key_frames a,b,c: key frames at these frames of every stream's chunk (thor_hip_force_key_frame); -key_scenecut PCT [-key_min_interval N]: scene cuts
 * (thor_hip_set_scene_cut; no default, 0 is off).  Low-delay configurations only.
 * -tf_strength S (1 .. 16; 0, the default, is off): the temporal noise filter (thor_hip_filter_staged) of every frame against its -tf_past P previous and
 * -tf_future F next frames of the stream's chunk (each 0 .. 2, default 0; frames beyond the ends of the chunk are dropped from the list).  The originals are
 * staged in slots beyond the chunk and filtered into the slots the encoder reads, all streams of a frame in one call.  The report's PSNR is then measured
 * against the filtered frames: they are what is coded.
 * With -streams S > 1, stream s encodes frames [skip + s*N, skip + (s+1)*N) as its own closed
 * stream and writes <of>.<s> / <rf>.<s> (the reference's -skip/-n chunking).
 * stdout: the reference's report (enc/mainenc.c:219-226, :553-591, :642-650; PSNR measured on the GPU unless -snrcalc 0) - with
 * S > 1 every stream's, in stream order, each after a line "stream <s>" - then the throughput line.  -stat appends the reference's
 * summary line of every stream to the file.
 * THOR_STAGGER=1 in the environment (S > 1): the streams are coded in two groups half a frame apart (thor_hip_encode_staged_run) instead of
 * frame by frame in lock step; the files written are the same.
 * All input frames are staged in HBM first; the timed region covers the encode loop only. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "../include/thor_hip.h"

static double now_s(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

/* thor_hip_encode_staged_run's callback: keep the reconstructions of the frames that just completed (display order) */
struct done_ctx { thor_hip_encoder* e; unsigned char** recs; FILE** fr; int n; size_t fsz; const thor_hip_frame_layout* lay; const thor_hip_rgb_format* rgb; };
static void get_recon(thor_hip_encoder* e, int s, unsigned char* r, const thor_hip_frame_layout* lay, const thor_hip_rgb_format* rgb) {
  if (rgb) thor_hip_get_recon_rgb(e, s, r, rgb, 0); else if (lay) thor_hip_get_recon_layout(e, s, r, lay, 0); else thor_hip_get_recon(e, s, r);
}
static void frames_done(void* user, int first, int count) {
  struct done_ctx* c = (struct done_ctx*)user;
  for (int s = first; s < first + count; s++)
    if (c->fr[s]) {
      unsigned char* r = (unsigned char*)malloc(c->fsz);
      get_recon(c->e, s, r, c->lay, c->rgb);
      c->recs[(size_t)s * c->n + thor_hip_last_display_index(c->e, s)] = r;
    }
}

int main(int argc, char** argv) {
  thor_hip_params p;
  const char *inf = NULL, *of = NULL, *rf = NULL;
  const char* statf = NULL;
  const char* pixfmt = "i420";
  const char *rgbmatrix = "709", *rgbrange = "limited", *rgbsite = "left";
  const char *scalefilter = "bicubic", *scalesite = "left";
  int src_w = 0, src_h = 0, scaled = 0;
  thor_hip_rate_control rc = {sizeof(thor_hip_rate_control), 0, 0, 0, 0, 0, 0, 0};
  thor_hip_scene_cut sc = {sizeof(thor_hip_scene_cut), 0, 0};
  const char* key_frames = NULL;
  int key_given = 0;
  thor_hip_temporal_filter tf = {sizeof(thor_hip_temporal_filter), 0};
  int tf_past = 0, tf_future = 0;
  int n = 600, skip = 0, S = 1, i, wrap = 0, snrcalc = 1;
  thor_hip_params_from_config(&p, NULL);
  /* config files first, explicit options afterwards (same precedence as the reference) */
  for (i = 1; i + 1 < argc; i += 2)
    if (!strcmp(argv[i], "-cf") && thor_hip_params_from_config(&p, argv[i + 1])) return 2;
  for (i = 1; i + 1 < argc; i += 2) {
    const char *k = argv[i], *v = argv[i + 1];
    if (!strcmp(k, "-cf")) continue;
    else if (!strcmp(k, "-if")) inf = v;
    else if (!strcmp(k, "-of")) of = v;
    else if (!strcmp(k, "-rf")) rf = v;
    else if (!strcmp(k, "-n")) n = atoi(v);
    else if (!strcmp(k, "-skip")) skip = atoi(v);
    else if (!strcmp(k, "-streams")) S = atoi(v);
    else if (!strcmp(k, "-snrcalc")) snrcalc = atoi(v);
    else if (!strcmp(k, "-stat")) statf = v;
    else if (!strcmp(k, "-pixfmt")) pixfmt = v;
    else if (!strcmp(k, "-rgbmatrix")) rgbmatrix = v;
    else if (!strcmp(k, "-rgbrange")) rgbrange = v;
    else if (!strcmp(k, "-rgbsite")) rgbsite = v;
    else if (!strcmp(k, "-src_width")) { src_w = atoi(v); scaled = 1; }
    else if (!strcmp(k, "-src_height")) { src_h = atoi(v); scaled = 1; }
    else if (!strcmp(k, "-scale_filter")) { scalefilter = v; scaled = 1; }
    else if (!strcmp(k, "-scale_site")) { scalesite = v; scaled = 1; }
    else if (!strcmp(k, "-rc_bitrate")) rc.bitrate = atoi(v);
    else if (!strcmp(k, "-rc_buffer_ms")) rc.buffer_ms = atoi(v);
    else if (!strcmp(k, "-rc_min_qp")) rc.min_qp = atoi(v);
    else if (!strcmp(k, "-rc_max_qp")) rc.max_qp = atoi(v);
    else if (!strcmp(k, "-rc_min_qpI")) rc.min_qp_i = atoi(v);
    else if (!strcmp(k, "-rc_max_qpI")) rc.max_qp_i = atoi(v);
    else if (!strcmp(k, "-rc_initial_qp")) rc.initial_qp = atoi(v);
    else if (!strcmp(k, "-key_frames")) { key_frames = v; key_given = 1; }
    else if (!strcmp(k, "-key_scenecut")) { sc.percent = atoi(v); key_given = 1; }
    else if (!strcmp(k, "-key_min_interval")) { sc.min_interval = atoi(v); key_given = 1; }
    else if (!strcmp(k, "-tf_strength")) tf.strength = atoi(v);
    else if (!strcmp(k, "-tf_past")) tf_past = atoi(v);
    else if (!strcmp(k, "-tf_future")) tf_future = atoi(v);
    else if (!strcmp(k, "-wrap")) wrap = atoi(v); /* clip length: frame index taken modulo this (throughput tests) */
    else if (!strcmp(k, "-log2_sb_size") ? thor_hip_params_set_sb_size(&p, atoi(v)) : thor_hip_params_set(&p, k, v)) { fprintf(stderr, "Run-time error...\noption %s %s is unknown or not implemented by this path\n...now exiting to system...\n", k, v); return 2; }
  }
  if (!inf) { fprintf(stderr, "usage: %s -cf cfg -if in.yuv -width W -height H -qp Q -n N ...\n", argv[0]); return 2; }
  FILE* fi = fopen(inf, "rb");
  if (!fi) { fprintf(stderr, "cannot open %s\n", inf); return 2; }
  if (p.input_bitdepth > p.bitdepth) { fprintf(stderr, "Run-time error...\ninput_bitdepth %d above bitdepth %d is not implemented by this path\n...now exiting to system...\n", p.input_bitdepth, p.bitdepth); return 2; }
  thor_hip_frame_layout layout = {sizeof(thor_hip_frame_layout), THOR_HIP_CHROMA_PLANAR, 0, 0, 0, 0, 0};
  const thor_hip_frame_layout* lay = strcmp(pixfmt, "i420") ? &layout : NULL; /* i420: the calls the files always took */
  thor_hip_rgb_format rgbfmt = {sizeof(thor_hip_rgb_format), 0, 8, 0, 0, 0, 0, 0, 0};
  const thor_hip_rgb_format* rgb = NULL; /* -pixfmt rgba|bgra|rgb24|bgr24: the files hold RGB frames, the device converts */
  if (!strcmp(pixfmt, "nv12")) layout.chroma = THOR_HIP_CHROMA_UV;
  else if (!strcmp(pixfmt, "nv21")) layout.chroma = THOR_HIP_CHROMA_VU;
  else if (!strcmp(pixfmt, "p010")) { layout.chroma = THOR_HIP_CHROMA_UV; layout.msb_aligned = 1; }
  else if (!strcmp(pixfmt, "rgba") || !strcmp(pixfmt, "bgra") || !strcmp(pixfmt, "rgb24") || !strcmp(pixfmt, "bgr24")) {
    lay = NULL;
    rgb = &rgbfmt;
    rgbfmt.order = !strcmp(pixfmt, "rgba") ? THOR_HIP_RGB_RGBA : !strcmp(pixfmt, "bgra") ? THOR_HIP_RGB_BGRA : !strcmp(pixfmt, "rgb24") ? THOR_HIP_RGB_RGB : THOR_HIP_RGB_BGR;
    rgbfmt.depth = p.input_bitdepth > 8 ? 16 : 8;
    rgbfmt.matrix = !strcmp(rgbmatrix, "601") ? THOR_HIP_MATRIX_BT601 : !strcmp(rgbmatrix, "709") ? THOR_HIP_MATRIX_BT709 : !strcmp(rgbmatrix, "2020") ? THOR_HIP_MATRIX_BT2020 : -1;
    rgbfmt.full_range = !strcmp(rgbrange, "full") ? 1 : !strcmp(rgbrange, "limited") ? 0 : -1;
    rgbfmt.chroma_site = !strcmp(rgbsite, "left") ? 1 : !strcmp(rgbsite, "centre") ? 0 : -1;
    if (!thor_hip_rgb_bytes_for(p.width, p.height, &rgbfmt)) { fprintf(stderr, "Run-time error...\n-pixfmt %s with -rgbmatrix %s -rgbrange %s -rgbsite %s is not a format of this path\n...now exiting to system...\n", pixfmt, rgbmatrix, rgbrange, rgbsite); return 2; }
  }
  else if (lay) { fprintf(stderr, "Run-time error...\noption -pixfmt %s is unknown\n...now exiting to system...\n", pixfmt); return 2; }
  if (lay && p.input_bitdepth <= 8 && layout.msb_aligned) { fprintf(stderr, "Run-time error...\n-pixfmt %s needs input_bitdepth above 8\n...now exiting to system...\n", pixfmt); return 2; }
  thor_hip_scale scale = {sizeof(thor_hip_scale), src_w ? src_w : p.width, src_h ? src_h : p.height,
                          !strcmp(scalefilter, "bicubic") ? THOR_HIP_SCALE_BICUBIC : !strcmp(scalefilter, "bilinear") ? THOR_HIP_SCALE_BILINEAR : -1,
                          !strcmp(scalesite, "left") ? 1 : !strcmp(scalesite, "centre") ? 0 : -1};
  if (scaled && (scale.filter < 0 || scale.chroma_site < 0)) { fprintf(stderr, "Run-time error...\noption -scale_filter %s -scale_site %s is unknown\n...now exiting to system...\n", scalefilter, scalesite); return 2; }
  if (scaled && (rgb || !thor_hip_scale_bytes_for(p.width, p.height, p.input_bitdepth, &scale, lay))) { fprintf(stderr, "Run-time error...\n-src_width %d -src_height %d with -pixfmt %s cannot be resampled to %dx%d\n...now exiting to system...\n", scale.src_width, scale.src_height, pixfmt, p.width, p.height); return 2; }
  if (thor_hip_rate_control_check(&rc)) { fprintf(stderr, "Run-time error...\nthe -rc_ options do not describe a rate control (a negative value, a minimum above its maximum, a QP above 51)\n...now exiting to system...\n"); return 2; }
  if (key_given && p.num_reorder_pics != 0) { fprintf(stderr, "Run-time error...\nthe -key_ options need a low-delay configuration (num_reorder_pics 0)\n...now exiting to system...\n"); return 2; }
  if (thor_hip_scene_cut_check(&sc) || (key_frames && key_frames[strspn(key_frames, "0123456789,")])) { fprintf(stderr, "Run-time error...\nthe -key_ options do not describe key frames (-key_scenecut 0 .. 100, -key_min_interval >= 0, -key_frames a,b,c)\n...now exiting to system...\n"); return 2; }
  if ((tf.strength && thor_hip_temporal_filter_check(&tf)) || tf_past < 0 || tf_past > 2 || tf_future < 0 || tf_future > 2) { fprintf(stderr, "Run-time error...\nthe -tf_ options do not describe a temporal filter (-tf_strength 0 .. 16, -tf_past and -tf_future 0 .. 2)\n...now exiting to system...\n"); return 2; }
  thor_hip_encoder* e = thor_hip_open(&p, S, 0);
  if (!e) { fprintf(stderr, "thor_hip_open failed\n"); return 3; }
  size_t fsz = rgb ? thor_hip_rgb_bytes(e, rgb) : thor_hip_frame_bytes(e); /* -if and -rf hold samples of the INPUT bit depth, or RGB frames */
  size_t isz = scaled ? thor_hip_scale_bytes(e, &scale, lay) : fsz;        /* -if at the source size */
  unsigned char* frame = (unsigned char*)malloc(isz);
  thor_hip_set_frame_distortion(e, snrcalc != 0);
  const int tfo = tf.strength ? n : 0; /* with the filter the originals go to slots n .. 2n - 1 and the filtered frames to the slots the encoder reads */
  for (int s = 0; s < S; s++)
    for (int f = 0; f < n; f++) {
      size_t idx = (size_t)skip + (size_t)s * n + f;
      if (wrap > 0) idx %= (size_t)wrap;
      if (fseek(fi, (long)(idx * isz), SEEK_SET) || fread(frame, 1, isz, fi) != isz) { fprintf(stderr, "short read at frame %zu\n", idx); return 4; }
      if (scaled ? thor_hip_stage_frame_scaled(e, s, tfo + f, frame, &scale, lay, 0) : rgb ? thor_hip_stage_frame_rgb(e, s, tfo + f, frame, rgb, 0) : lay ? thor_hip_stage_frame_layout(e, s, tfo + f, frame, lay, 0) : thor_hip_stage_frame(e, s, tfo + f, frame)) { fprintf(stderr, "staging failed\n"); return 4; }
    }
  double ttf = 0;
  if (tf.strength) { /* one call per frame: the requests of all streams */
    thor_hip_tf_request* req = (thor_hip_tf_request*)calloc(S, sizeof(thor_hip_tf_request));
    double a = now_s();
    for (int f = 0; f < n; f++) {
      for (int s = 0; s < S; s++) {
        thor_hip_tf_request* r = &req[s];
        r->stream = s; r->dst_slot = f; r->slot = tfo + f; r->nrefs = 0;
        for (int d = 1; d <= tf_past; d++) if (f - d >= 0) { r->ref_slot[r->nrefs] = tfo + f - d; r->ref_dist[r->nrefs++] = d; }
        for (int d = 1; d <= tf_future; d++) if (f + d < n) { r->ref_slot[r->nrefs] = tfo + f + d; r->ref_dist[r->nrefs++] = d; }
      }
      if (thor_hip_filter_staged(e, req, S, &tf)) { fprintf(stderr, "temporal filter refused\n"); return 4; }
    }
    ttf = now_s() - a;
    free(req);
  }
  FILE** fr = (FILE**)calloc(S, sizeof(FILE*));
  char name[4096];
  for (int s = 0; s < S && rf; s++) {
    if (S == 1) snprintf(name, sizeof name, "%s", rf); else snprintf(name, sizeof name, "%s.%d", rf, s);
    fr[s] = fopen(name, "wb");
  }
  int* slots = (int*)malloc(S * sizeof(int));
  /* coding-order schedule (B frames are coded out of display order); recon is written in display order */
  fseek(fi, 0, SEEK_END);
  long file_frames = wrap > 0 ? (long)skip + (long)S * n : (long)(ftell(fi) / (long)isz);
  for (int s = 0; s < S; s++)
    if (thor_hip_begin_sequence(e, s, skip + s * n, n, (int)file_frames)) { fprintf(stderr, "bad sequence bounds\n"); return 5; }
  for (int s = 0; s < S && rc.bitrate; s++)
    if (thor_hip_set_rate_control(e, s, &rc)) { fprintf(stderr, "rate control refused\n"); return 5; }
  for (int s = 0; s < S && key_given; s++) {
    /* THOR_KEY_SHIFT=k (tests): stream s asks for its key frames k * s frames later */
    int shift = getenv("THOR_KEY_SHIFT") ? atoi(getenv("THOR_KEY_SHIFT")) * s : 0;
    for (const char* q = key_frames; q && *q; q += strcspn(q, ","), q += *q == ',') {
      int f = atoi(q) + shift;
      if (f < n && thor_hip_force_key_frame(e, s, f)) { fprintf(stderr, "Run-time error...\n-key_frames: frame %d cannot be a key frame\n...now exiting to system...\n", f); return 2; }
    }
    if (sc.percent && thor_hip_set_scene_cut(e, s, &sc)) { fprintf(stderr, "scene cut refused\n"); return 5; }
  }
  unsigned char** recs = (unsigned char**)calloc((size_t)S * n, sizeof(unsigned char*));
  double t0 = now_s(), tenc = 0;
  int coded = 0;
  if (S > 1 && getenv("THOR_STAGGER") && atoi(getenv("THOR_STAGGER"))) {
    struct done_ctx ctx = {e, recs, fr, n, fsz, lay, rgb};
    double a = now_s();
    if (thor_hip_encode_staged_run(e, n, frames_done, &ctx)) { fprintf(stderr, "encode failed\n"); return 5; }
    tenc = now_s() - a;
    coded = n;
  } else
  for (;;) {
    int active = 0;
    for (int s = 0; s < S; s++) active += thor_hip_next_frame(e, s, &slots[s]);
    if (!active) break;
    if (active != S) { fprintf(stderr, "streams out of step\n"); return 5; }
    double a = now_s();
    if (thor_hip_encode_staged(e, slots)) { fprintf(stderr, "encode failed\n"); return 5; }
    tenc += now_s() - a;
    coded++;
    for (int s = 0; s < S; s++)
      if (fr[s]) {
        unsigned char* r = (unsigned char*)malloc(fsz);
        get_recon(e, s, r, lay, rgb);
        recs[(size_t)s * n + slots[s]] = r;
      }
  }
  for (int s = 0; s < S; s++)
    if (fr[s])
      for (int f = 0; f < n; f++)
        if (recs[(size_t)s * n + f]) fwrite(recs[(size_t)s * n + f], 1, fsz, fr[s]);
  for (int s = 0; s < S; s++) {
    int len = thor_hip_report(e, s, NULL, 0);
    char* rep = (char*)malloc((size_t)len + 1);
    thor_hip_report(e, s, rep, (size_t)len + 1);
    if (S > 1) fprintf(stdout, "stream %d\n", s);
    fputs(rep, stdout);
    free(rep);
    if (statf) {
      char line[256];
      FILE* sf = fopen(statf, "r");
      int not_exists = !sf;
      if (sf) fclose(sf);
      thor_hip_stat_line(e, s, n, line, sizeof line);
      if ((sf = fopen(statf, "a")) != NULL) {
        if (not_exists) fputs(" NFR     kbps     PSNRY  PSNRU  PSNRV\n", sf);
        fputs(line, sf);
        fclose(sf);
      }
    }
  }
  if (getenv("THOR_KEY_LOG")) { /* tests: one line per coded frame of every stream: stream, display, type, reason, the analysis sums */
    FILE* fl = fopen(getenv("THOR_KEY_LOG"), "w");
    if (!fl) { fprintf(stderr, "cannot open %s\n", getenv("THOR_KEY_LOG")); return 5; }
    for (int s = 0; s < S; s++)
      for (int f = 0; f < thor_hip_frame_stats_count(e, s); f++) {
        thor_hip_frame_stats fs;
        thor_hip_frame_key fk;
        if (thor_hip_get_frame_stats(e, s, f, &fs) || thor_hip_get_frame_key(e, s, f, &fk)) return 5;
        fprintf(fl, "%d %d %d %d %llu %llu %llu\n", s, fs.display_index, fs.frame_type, fk.reason, fk.sum_intra, fk.sum_best, fk.n_intra);
      }
    fclose(fl);
  }
  n = coded;
  double sb_ms = 0, filt_ms = 0; long launches = 0;
  thor_hip_kernel_time(e, &sb_ms, &launches, &filt_ms);
  double mpx = (double)p.width * p.height * n * S / 1e6;
  if (tf.strength) fprintf(stdout, "thorenc_hip: temporal filter strength %d, %d past / %d future: %.3f s for %d call(s)\n", tf.strength, tf_past, tf_future, ttf, n);
  fprintf(stdout, "thorenc_hip: %d stream(s) x %d frame(s) %dx%d: encode %.3f s (%.3f Mpx/s), total %.3f s; superblock kernels %.1f ms in %ld launches, filters %.1f ms\n",
          S, n, p.width, p.height, tenc, mpx / tenc, now_s() - t0, sb_ms, launches, filt_ms);
  if (getenv("THOR_PROF")) {
    static const char* nm[32] = {"sb_total", "early_skip", "me_fullpel", "me_subpel", "pred_inter", "md_worker_all_waves", "code_tu", "bits", "cost", "final", "subpel_loop",
                                 "me_calls(n)", "quant", "me_telescope", "me_cands", "me_hex", "tu4", "tu8", "tu16", "tu32", "tu64+",
                                 "tu4(n)", "tu8(n)", "tu16(n)", "tu32(n)", "tu64+(n)", "wg_barrier_wait(all waves)", "bipred_lockstep(all waves, incl. barriers)", "helpers_parked(master alone)", "md_fork_to_join(master)", "tu_fwd", "tu_inv"};
    /* THOR_PROF=md: the library was built with -DTHOR_PROF_MD (slots 16..25 = work-queue items by kind / master-alone phases, tk_block_ws.h);
       THOR_PROF=me: -DTHOR_PROF_ME (motion-search cycles and calls by coding-block size) */
    static const char* nm_md[10] = {"items skip/merge", "items intra", "items search (MD_REF)", "items trial (incl. wait)", "trial items: wait for vectors", "queue set-up (master)",
                                    "block entry (master)", "early-skip path (master)", "final encode of decided blocks: emission (master)", "final encode of decided blocks: whole (master)"};
    static const char* nm_me[10] = {"me cb8", "me cb16", "me cb32", "me cb64", "me cb128", "me cb8(n)", "me cb16(n)", "me cb32(n)", "me cb64(n)", "me cb128(n)"};
    if (!strcmp(getenv("THOR_PROF"), "md")) for (int k = 0; k < 10; k++) nm[16 + k] = nm_md[k];
    if (!strcmp(getenv("THOR_PROF"), "me")) for (int k = 0; k < 10; k++) nm[16 + k] = nm_me[k];
    long long pr[32];
    thor_hip_read_prof(e, pr);
    for (int k = 0; k < 32; k++) fprintf(stdout, "prof %-40s %16lld %6.2f%%\n", nm[k], pr[k], pr[0] ? 100.0 * pr[k] / pr[0] : 0.0);
  }
  for (int s = 0; s < S; s++) {
    if (fr[s]) fclose(fr[s]);
    if (of) {
      if (S == 1) snprintf(name, sizeof name, "%s", of); else snprintf(name, sizeof name, "%s.%d", of, s);
      FILE* fo = fopen(name, "wb");
      fwrite(thor_hip_stream_data(e, s), 1, thor_hip_stream_bytes(e, s), fo);
      fclose(fo);
    }
  }
  thor_hip_close(e);
  fclose(fi);
  return 0;
}
