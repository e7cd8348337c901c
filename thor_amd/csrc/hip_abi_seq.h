// hip_abi_seq.h - C ABI, sequence API of include/thor_hip.h: thor_hip_open ... thor_hip_stat_line (part of the translation unit thor_hip.cpp).
#pragma once
using namespace tk;

template <typename PIX> struct EncT {
  Engine<PIX> eng;
  std::vector<char> pending;  // thor_hip_next_frame already scheduled the stream's next frame
  std::vector<std::vector<DevFrame<PIX>>> staged;  // [stream][slot]
};
struct thor_hip_encoder {
  SeqParams sp;
  int S = 0;
  bool hbd = false;          // samples are uint16_t (bitdepth > 8)
  EncT<uint8_t>* e8 = nullptr;
  EncT<uint16_t>* e16 = nullptr;
};
#define ENC_DISPATCH(e, body)                                   \
  do {                                                          \
    if ((e)->hbd) { auto& E = *(e)->e16; typedef uint16_t PIXT; body; } \
    else { auto& E = *(e)->e8; typedef uint8_t PIXT; body; }            \
  } while (0)

// stream `s` of whichever engine the encoder has: ENC_STREAM(e, s, out.size())
#define ENC_STREAM(e, s, member) ((e)->hbd ? (e)->e16->eng.st[s].member : (e)->e8->eng.st[s].member)

// The encoder parameters, each named once.  SEAM: the fields thor_hip_params, SeqParams and the reference's enc_params (thor_enc_params, the drop-in
// seam) share under one name and the seam copies as they are; SEQ_ONLY: the fields the seam sets by its own rules or leaves at their defaults.
#define TK_PARAMS_SEAM(X)                                                                                                             \
  X(bitdepth) X(input_bitdepth) X(frame_rate) X(lambda_coeffI) X(lambda_coeffP) X(early_skip_thr) X(enable_tb_split) X(enable_pb_split) \
  X(max_num_ref) X(num_reorder_pics) X(interp_ref) X(dqpP) X(dqpI) X(mqpP) X(intra_period) X(intra_rdo) X(encoder_speed) X(deblocking)  \
  X(cdef) X(clpf) X(use_block_contexts) X(enable_bipred) X(cfl_intra) X(cfl_inter) X(max_clpf_strength) X(log2_sb_size)
#define TK_PARAMS_SEQ_ONLY(X)                                                                                                         \
  X(width) X(height) X(qp) X(HQperiod) X(dyadic_coding)                                                                               \
  X(lambda_coeffB) X(lambda_coeffB0) X(lambda_coeffB1) X(lambda_coeffB2) X(lambda_coeffB3)                                            \
  X(dqpB) X(dqpB0) X(dqpB1) X(dqpB2) X(dqpB3) X(mqpB) X(mqpB0) X(mqpB1) X(mqpB2) X(mqpB3)
#define TK_PARAM_COPY(f) dst.f = src.f;
#define TK_PARAM_COUNT(f) +1
static_assert(sizeof(thor_hip_params) == 4 * (0 TK_PARAMS_SEAM(TK_PARAM_COUNT) TK_PARAMS_SEQ_ONLY(TK_PARAM_COUNT)),
              "a field of thor_hip_params (all int / float) is missing from the lists above");
static SeqParams to_seq(const thor_hip_params& src) {
  SeqParams dst;
  TK_PARAMS_SEAM(TK_PARAM_COPY) TK_PARAMS_SEQ_ONLY(TK_PARAM_COPY)
  return dst;
}
static void from_seq(thor_hip_params* p, const SeqParams& src) {
  thor_hip_params& dst = *p;
  TK_PARAMS_SEAM(TK_PARAM_COPY) TK_PARAMS_SEQ_ONLY(TK_PARAM_COPY)
}

static int unsupported(const SeqParams& s) {
  // This path implements the high-efficiency low-delay operating point family; reject the rest
  // loudly rather than silently producing a different stream.
  // input at a lower depth is widened on the way in (v << shift) and the reconstruction rounded back on the way out, as the reference does; the other
  // direction is refused: the reference reads two-byte samples into one-byte frames there unless further options are given
  auto depth_ok = [](int d) { return d == 8 || d == 10 || d == 12; };
  if (!depth_ok(s.bitdepth) || !depth_ok(s.input_bitdepth) || s.input_bitdepth > s.bitdepth)
    return fprintf(stderr, "thor_hip: need bitdepth and input_bitdepth in {8, 10, 12} with input_bitdepth <= bitdepth\n"), 1;
  if (s.num_reorder_pics != 0 && !s.dyadic_coding) return fprintf(stderr, "thor_hip: non-dyadic frame reordering is not implemented\n"), 1;
  if (s.num_reorder_pics < 0 || s.num_reorder_pics > 15 || (s.num_reorder_pics & (s.num_reorder_pics + 1)))
    return fprintf(stderr, "thor_hip: num_reorder_pics must be 0, 1, 3, 7 or 15\n"), 1;
  if (s.interp_ref != 0 && s.interp_ref != 1) return fprintf(stderr, "thor_hip: interp_ref must be 0 or 1\n"), 1;
  if (s.encoder_speed < 0 || s.encoder_speed > 2) return fprintf(stderr, "thor_hip: encoder_speed must be 0, 1 or 2\n"), 1;
  if (s.width % 8 || s.height % 8 || s.width < 16 || s.height < 16) return fprintf(stderr, "thor_hip: bad geometry\n"), 1;
  if (s.max_num_ref < 1 || s.max_num_ref > 4) return fprintf(stderr, "thor_hip: max_num_ref out of range\n"), 1;
  // remaining guards of check_parameters (enc/strings.c:470-555) that matter without rate control / qmtx
  if (s.HQperiod < 1 || s.HQperiod >= 33) return fprintf(stderr, "thor_hip: HQperiod must be in 1..32\n"), 1;
  if (s.num_reorder_pics > 0 && s.HQperiod > 1 && (s.HQperiod % (s.num_reorder_pics + 1)) != 0)
    return fprintf(stderr, "thor_hip: sub-GOP length (num_reorder_pics+1) must divide HQperiod\n"), 1;
  if (s.num_reorder_pics > 0 && s.max_num_ref < 2) return fprintf(stderr, "thor_hip: reordered pictures need more than one reference frame\n"), 1;
  if (s.intra_period < 0 || (s.intra_period % (s.num_reorder_pics + 1)) != 0)
    return fprintf(stderr, "thor_hip: intra_period must be a multiple of the sub-GOP size\n"), 1;
  if (s.qp < 0 || s.qp > 51) return fprintf(stderr, "thor_hip: qp out of range\n"), 1;
  if (s.cdef < 0 || s.cdef > 3 || s.clpf < 0 || s.clpf > 2) return fprintf(stderr, "thor_hip: cdef / clpf out of range\n"), 1;
  if (s.log2_sb_size != 6 && s.log2_sb_size != 7) return fprintf(stderr, "thor_hip: log2_sb_size must be 6 or 7 (64x64 or 128x128 superblocks)\n"), 1;
  return 0;
}

// The caller's layout against a width x height picture of input_bitdepth samples; false: refused (a wrong `size` included).  Touches no device.
static bool layout_resolved(const thor_hip_frame_layout* l, int width, int height, int input_bitdepth, PixLayout& L) {
  if (!l || l->size != (int)sizeof(thor_hip_frame_layout)) return false;
  return resolve_layout(l->chroma, l->msb_aligned, l->pitch_y, l->pitch_c, l->offset_u, l->offset_v, width, height, input_bitdepth, L);
}

// The caller's RGB format against a width x height picture of input_bitdepth samples; false: refused (a wrong `size` included).  Touches no device.
static bool rgb_resolved(const thor_hip_rgb_format* f, int width, int height, int input_bitdepth, RgbFormat& R) {
  if (!f || f->size != (int)sizeof(thor_hip_rgb_format)) return false;
  return resolve_rgb(f->order, f->depth, f->msb_aligned, f->matrix, f->full_range, f->chroma_site, f->pitch, f->plane_stride, width, height, input_bitdepth, R);
}

extern "C" {

int thor_hip_params_from_config(thor_hip_params* p, const char* cfg_path) {
  CliArgs a;
  a.sp.width = 1920; a.sp.height = 1080; a.sp.frame_rate = 60.f;  // enc/strings.c defaults
  if (cfg_path) {
    std::vector<std::string> t = {"-cf", cfg_path};
    cli_apply(a, t);
  }
  from_seq(p, a.sp);
  if (!a.unknown.empty()) return fprintf(stderr, "thor_hip: unknown option %s in %s\n", a.unknown.c_str(), cfg_path), 1;
  if (!a.unsupported.empty()) return fprintf(stderr, "thor_hip: %s (in %s) is not implemented by this path\n", a.unsupported.c_str(), cfg_path), 2;
  return 0;
}

int thor_hip_params_set(thor_hip_params* p, const char* name, const char* value) {
  if (!p || !name || !value) return 1;
  // This door keeps its contract for -log2_sb_size: the default passes, any other value is "not implemented" and *p stays as it is
  // (tests/test_params.py pins that for 6).  The superblock size is chosen with thor_hip_params_set_sb_size or in a config file.
  if (!strcmp(name, "-log2_sb_size") && atoi(value) != kLog2MaxSb) return 2;
  CliArgs a;
  a.sp = to_seq(*p);
  std::vector<std::string> t = {name, value};
  cli_apply(a, t);
  from_seq(p, a.sp);
  if (!a.unknown.empty()) return 1;      // not an option of the reference's table
  if (!a.unsupported.empty()) return 2;  // known, but this value is not implemented (qmtx, rate control, 4:4:4 ...)
  if (!a.infile.empty() || !a.outfile.empty() || !a.recfile.empty() || a.num_frames != 600 || a.skip != 0 || a.streams != 1 || a.pixfmt != "i420" || a.rgb_given || a.scale_given || a.rc_given || a.key_given || a.tf_given) return 3;  // front-end option, not an encoder parameter
  return 0;
}

int thor_hip_params_set_sb_size(thor_hip_params* p, int log2_sb_size) {
  if (!p) return 1;
  if (log2_sb_size != 6 && log2_sb_size != 7) return 2;  // the same code thor_hip_params_set gives a value that is not implemented
  p->log2_sb_size = log2_sb_size;
  return 0;
}

int thor_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

thor_hip_encoder* thor_hip_open(const thor_hip_params* p, int num_streams, int device) {
  if (!p || num_streams < 1) return nullptr;
  SeqParams s = to_seq(*p);
  if (unsupported(s)) return nullptr;
  // A parameter set that is in order still cannot be opened on a machine without a device: the constructor says so through its own failure channel
  // (NULL and a message) and leaves the caller's process alive.  There is no CPU path; the entry points that compute keep ending the process.
  if (thor_hip_device_count() < 1) return fprintf(stderr, "thor_hip: no HIP device available - this library has no CPU path\n"), nullptr;
  if (!ensure_init(device)) return nullptr;
  thor_hip_encoder* e = new thor_hip_encoder;
  e->sp = s;
  e->S = num_streams;
  e->hbd = s.bitdepth > 8;
  if (e->hbd) e->e16 = new EncT<uint16_t>; else e->e8 = new EncT<uint8_t>;
  ENC_DISPATCH(e, { E.eng.open(s, num_streams); E.staged.resize(num_streams); E.pending.assign(num_streams, 0); });
  return e;
}

void thor_hip_close(thor_hip_encoder* e) {
  if (!e) return;
  ENC_DISPATCH(e, {
    for (auto& v : E.staged)
      for (auto& f : v)
        if (f.base_y) f.release();
    E.eng.close();
  });
  delete e->e8;
  delete e->e16;
  delete e;
}

int thor_hip_begin_sequence(thor_hip_encoder* e, int stream, int skip, int num_frames, int file_frames) {
  if (!e || stream < 0 || stream >= e->S || skip < 0 || num_frames < 1 || file_frames < skip + num_frames) return 1;
  ENC_DISPATCH(e, { E.eng.begin_sequence(stream, skip, num_frames, file_frames); E.pending[stream] = 0; });
  return 0;
}

int thor_hip_next_frame(thor_hip_encoder* e, int stream, int* display_index) {
  if (!e || stream < 0 || stream >= e->S) return 0;
  int ok = 0;
  ENC_DISPATCH(e, {
    if (E.pending[stream]) ok = 1;
    else ok = E.eng.schedule(stream) ? 1 : 0;
    E.pending[stream] = (char)ok;
    if (ok && display_index) *display_index = E.eng.st[stream].cur.frame_num;
  });
  return ok;
}

int thor_hip_stage_frame(thor_hip_encoder* e, int stream, int slot, const void* yuv) {
  if (!e || stream < 0 || stream >= e->S || slot < 0 || !yuv) return 1;
  ENC_DISPATCH(e, {
    auto& v = E.staged[stream];
    if ((int)v.size() <= slot) v.resize(slot + 1);
    if (!v[slot].base_y) v[slot].alloc(e->sp.width, e->sp.height, 0);
    DevFrame<PIXT> keep = E.eng.st[stream].orig;
    E.eng.st[stream].orig = v[slot];
    E.eng.upload_orig(stream, yuv);
    E.eng.st[stream].orig = keep;
  });
  return 0;
}

// Same as thor_hip_stage_frame for a frame that already lives in HBM (e.g. a torch CUDA tensor the caller derived from a
// clip broadcast over RCCL): three device-to-device 2-D copies on the library's stream; the source may be released
// when the call returns.  With input_bitdepth < bitdepth the widen kernel reads the caller's buffer and writes the slot: no copy.
int thor_hip_stage_frame_device(thor_hip_encoder* e, int stream, int slot, const void* dev_yuv) {
  if (!e || stream < 0 || stream >= e->S || slot < 0 || !dev_yuv) return 1;
  ENC_DISPATCH(e, {
    auto& v = E.staged[stream];
    if ((int)v.size() <= slot) v.resize(slot + 1);
    if (!v[slot].base_y) v[slot].alloc(e->sp.width, e->sp.height, 0);
    if (E.eng.depth_shift() > 0) {
      // the kernel reads vectors (tk_filters.h: depth_up_rows); frame sizes are multiples of 96 bytes, so the frames of an aligned clip all are
      if ((uintptr_t)dev_yuv & 15) {
        fprintf(stderr, "thor_hip: thor_hip_stage_frame_device needs a 16-byte aligned frame when input_bitdepth < bitdepth\n");
        return 1;
      }
      E.eng.widen(dev_yuv, v[slot].p);
      HIPCHECK(hipStreamSynchronize(g_stream));
      return 0;
    }
    const PIXT* src = (const PIXT*)dev_yuv;
    const size_t B = sizeof(PIXT);
    for_yuv_planes(v[slot].p, e->sp.width, e->sp.height, [&](PIXT* d, int ds, size_t off, int pw, int ph) {
      HIPCHECK(hipMemcpy2DAsync(d, ds * B, src + off, pw * B, pw * B, ph, hipMemcpyDeviceToDevice, g_stream));
    });
    HIPCHECK(hipStreamSynchronize(g_stream));
  });
  return 0;
}

int thor_hip_encode_staged(thor_hip_encoder* e, const int* slots) {
  if (!e || !slots) return 1;
  int rc = 0;
  ENC_DISPATCH(e, {
    std::vector<DevFrame<PIXT>> keep(e->S);
    std::vector<FrameParams> fp(e->S);
    for (int s = 0; s < e->S && !rc; s++)
      if (slots[s] < 0 || slots[s] >= (int)E.staged[s].size() || !E.staged[s][slots[s]].base_y) rc = 2;
    if (!rc) {
      for (int s = 0; s < e->S; s++) {
        keep[s] = E.eng.st[s].orig;
        E.eng.st[s].orig = E.staged[s][slots[s]];
        if (!E.pending[s] && !E.eng.schedule(s)) { fprintf(stderr, "thor_hip: stream %d has no frame left to code\n", s); abort(); }
        E.pending[s] = 0;
        fp[s] = E.eng.st[s].cur;
      }
      E.eng.encode_frames(fp);
      for (int s = 0; s < e->S; s++) E.eng.st[s].orig = keep[s];
    }
  });
  return rc;
}

int thor_hip_encode_staged_run(thor_hip_encoder* e, int nframes, thor_hip_frames_done_fn done, void* user) {
  if (!e || nframes < 0) return 1;
  int rc = 0;
  ENC_DISPATCH(e, {
    // Validate BEFORE the first launch (a failure inside encode_run would leave half-frames in flight): dry-run every stream's coding-order
    // schedule on a copy - the sequence of display indices does not depend on the reference ring - and check that each of the next `nframes`
    // frames exists (rc 2) and is staged (rc 3).  Nothing is touched when the run is refused.
    for (int s = 0; s < e->S && !rc; s++) {
      GopScheduler g = E.eng.st[s].gop;
      if (!g.started) g.init(E.eng.sp, 0, 1 << 28, 1 << 28);
      for (int f = 0; f < nframes && !rc; f++) {
        FrameParams fpar;
        int abs_frame = 0;
        if (f == 0 && E.pending[s]) fpar = E.eng.st[s].cur;   // already scheduled by thor_hip_next_frame
        else if (!g.next(fpar, abs_frame, [&](int idx) { return E.eng.st[s].ring[idx].frame_num; })) { rc = 2; break; }
        g.advance(fpar);   // the engine advances the schedule when the frame is finished (tk_encoder.h:finish_frames)
        const int slot = fpar.frame_num;
        if (slot < 0 || slot >= (int)E.staged[s].size() || !E.staged[s][slot].base_y) {
          fprintf(stderr, "thor_hip: stream %d: frame %d is not staged\n", s, slot);
          rc = 3;
        }
      }
    }
    if (rc) return rc;
    std::vector<DevFrame<PIXT>> keep(e->S);
    for (int s = 0; s < e->S; s++) keep[s] = E.eng.st[s].orig;
    E.eng.encode_run(nframes,
        [&](int s) -> bool {
          if (!E.pending[s] && !E.eng.schedule(s)) { rc = 2; return false; }
          E.pending[s] = 0;
          const int slot = E.eng.st[s].cur.frame_num;
          if (slot < 0 || slot >= (int)E.staged[s].size() || !E.staged[s][slot].base_y) {
            fprintf(stderr, "thor_hip: stream %d: frame %d is not staged\n", s, slot);
            rc = 3;
            return false;
          }
          E.eng.st[s].orig = E.staged[s][slot];
          return true;
        },
        [&](int first, int count) { if (done) done(user, first, count); });
    for (int s = 0; s < e->S; s++) E.eng.st[s].orig = keep[s];
  });
  return rc;
}
int thor_hip_last_display_index(const thor_hip_encoder* e, int stream) {
  if (!e || stream < 0 || stream >= e->S) return -1;
  if (ENC_STREAM(e, stream, num_encoded) < 1) return -1;
  return ENC_STREAM(e, stream, cur.frame_num);
}

int thor_hip_encode_frame(thor_hip_encoder* e, const void* const* yuv) {
  if (!e || !yuv) return 1;
  ENC_DISPATCH(e, {
    std::vector<FrameParams> fp(e->S);
    for (int s = 0; s < e->S; s++) {
      E.eng.upload_orig(s, yuv[s]);
      if (!E.pending[s] && !E.eng.schedule(s)) { fprintf(stderr, "thor_hip: stream %d has no frame left to code\n", s); abort(); }
      E.pending[s] = 0;
      fp[s] = E.eng.st[s].cur;
    }
    E.eng.encode_frames(fp);
  });
  return 0;
}

size_t thor_hip_stream_bytes(const thor_hip_encoder* e, int stream) {
  if (!e || stream < 0 || stream >= e->S) return 0;
  return ENC_STREAM(e, stream, out.size());
}
const uint8_t* thor_hip_stream_data(const thor_hip_encoder* e, int stream) {
  if (!e || stream < 0 || stream >= e->S) return nullptr;
  return ENC_STREAM(e, stream, out.data());
}
size_t thor_hip_frame_bytes(const thor_hip_encoder* e) {
  if (!e) return 0;
  return (size_t)e->sp.width * e->sp.height * 3 / 2 * (e->sp.input_bitdepth > 8 ? 2 : 1);
}
int thor_hip_get_recon(thor_hip_encoder* e, int stream, void* yuv_out) {
  if (!e || stream < 0 || stream >= e->S || !yuv_out) return 1;
  ENC_DISPATCH(e, { E.eng.download_rec(stream, yuv_out); });
  return 0;
}

// ---- frames in a caller's layout (NV12 / NV21 / P010 ..., a row pitch): tk_filters.h PixLayout, k_layout_in / k_layout_out ----
size_t thor_hip_layout_bytes_for(int width, int height, int input_bitdepth, const thor_hip_frame_layout* layout) {
  PixLayout L;
  if (width < 16 || height < 16 || width % 8 || height % 8 || (input_bitdepth != 8 && input_bitdepth != 10 && input_bitdepth != 12)) return 0;
  return layout_resolved(layout, width, height, input_bitdepth, L) ? L.bytes : 0;
}
size_t thor_hip_layout_bytes(const thor_hip_encoder* e, const thor_hip_frame_layout* layout) {
  return e ? thor_hip_layout_bytes_for(e->sp.width, e->sp.height, e->sp.input_bitdepth, layout) : 0;
}
int thor_hip_stage_frame_layout(thor_hip_encoder* e, int stream, int slot, const void* frame, const thor_hip_frame_layout* layout, int on_device) {
  PixLayout L;
  if (!e || stream < 0 || stream >= e->S || slot < 0 || !frame) return 1;
  if (!layout_resolved(layout, e->sp.width, e->sp.height, e->sp.input_bitdepth, L) || (uintptr_t)frame % (e->sp.input_bitdepth > 8 ? 2 : 1)) return 1;
  ENC_DISPATCH(e, {
    auto& v = E.staged[stream];
    if ((int)v.size() <= slot) v.resize(slot + 1);
    if (!v[slot].base_y) v[slot].alloc(e->sp.width, e->sp.height, 0);
    if (on_device) {  // the kernel reads the caller's buffer and writes the slot
      E.eng.layout_in(frame, L, v[slot].p);
      HIPCHECK(hipStreamSynchronize(g_stream));
    } else
      E.eng.stage_layout_host(frame, L, v[slot].p);
  });
  return 0;
}
int thor_hip_get_recon_layout(thor_hip_encoder* e, int stream, void* frame, const thor_hip_frame_layout* layout, int on_device) {
  PixLayout L;
  if (!e || stream < 0 || stream >= e->S || !frame) return 1;
  if (!layout_resolved(layout, e->sp.width, e->sp.height, e->sp.input_bitdepth, L) || (uintptr_t)frame % (e->sp.input_bitdepth > 8 ? 2 : 1)) return 1;
  ENC_DISPATCH(e, {
    if (on_device) {
      E.eng.layout_out(E.eng.st[stream].rec.p, frame, L);
      HIPCHECK(hipStreamSynchronize(g_stream));
    } else
      E.eng.fetch_layout_host(E.eng.st[stream].rec.p, frame, L);
  });
  return 0;
}

// ---- RGB frames: tk_filters.h RgbFormat, k_rgb_in / k_rgb_out ----
size_t thor_hip_rgb_bytes_for(int width, int height, const thor_hip_rgb_format* fmt) {
  RgbFormat R;
  return rgb_resolved(fmt, width, height, 8, R) ? R.bytes : 0;  // the size does not depend on the input depth
}
size_t thor_hip_rgb_bytes(const thor_hip_encoder* e, const thor_hip_rgb_format* fmt) {
  return e ? thor_hip_rgb_bytes_for(e->sp.width, e->sp.height, fmt) : 0;
}
int thor_hip_stage_frame_rgb(thor_hip_encoder* e, int stream, int slot, const void* frame, const thor_hip_rgb_format* fmt, int on_device) {
  RgbFormat R;
  if (!e || stream < 0 || stream >= e->S || slot < 0 || !frame) return 1;
  if (!rgb_resolved(fmt, e->sp.width, e->sp.height, e->sp.input_bitdepth, R) || (uintptr_t)frame % R.sbytes) return 1;
  ENC_DISPATCH(e, {
    auto& v = E.staged[stream];
    if ((int)v.size() <= slot) v.resize(slot + 1);
    if (!v[slot].base_y) v[slot].alloc(e->sp.width, e->sp.height, 0);
    if (on_device) {  // the kernel reads the caller's buffer and writes the slot
      E.eng.rgb_in(frame, R, v[slot].p);
      HIPCHECK(hipStreamSynchronize(g_stream));
    } else
      E.eng.stage_rgb_host(frame, R, v[slot].p);
  });
  return 0;
}
int thor_hip_get_recon_rgb(thor_hip_encoder* e, int stream, void* frame, const thor_hip_rgb_format* fmt, int on_device) {
  RgbFormat R;
  if (!e || stream < 0 || stream >= e->S || !frame) return 1;
  if (!rgb_resolved(fmt, e->sp.width, e->sp.height, e->sp.input_bitdepth, R) || (uintptr_t)frame % R.sbytes) return 1;
  ENC_DISPATCH(e, {
    if (on_device) {
      E.eng.rgb_out(E.eng.st[stream].rec.p, frame, R);
      HIPCHECK(hipStreamSynchronize(g_stream));
    } else
      E.eng.fetch_rgb_host(E.eng.st[stream].rec.p, frame, R);
  });
  return 0;
}
// ---- frames of another size: tk_scale.h ScalePlan, k_scale_in ----
// The caller's two structures against a width x height engine; false: refused (a wrong `size` included).  Touches no device, builds no table.
static bool scale_args_resolved(const thor_hip_scale* sc, const thor_hip_frame_layout* l, int width, int height, int input_bitdepth, PixLayout& L) {
  static const thor_hip_frame_layout packed = {sizeof(thor_hip_frame_layout), THOR_HIP_CHROMA_PLANAR, 0, 0, 0, 0, 0};
  if (!sc || sc->size != (int)sizeof(thor_hip_scale)) return false;
  if (!l) l = &packed;
  if (l->size != (int)sizeof(thor_hip_frame_layout)) return false;
  return resolve_scale_args(sc->src_width, sc->src_height, sc->filter, sc->chroma_site, l->chroma, l->msb_aligned, l->pitch_y, l->pitch_c, l->offset_u, l->offset_v,
                            width, height, input_bitdepth, L);
}
size_t thor_hip_scale_bytes_for(int width, int height, int input_bitdepth, const thor_hip_scale* scale, const thor_hip_frame_layout* layout) {
  PixLayout L;
  return scale_args_resolved(scale, layout, width, height, input_bitdepth, L) ? L.bytes : 0;
}
size_t thor_hip_scale_bytes(const thor_hip_encoder* e, const thor_hip_scale* scale, const thor_hip_frame_layout* layout) {
  return e ? thor_hip_scale_bytes_for(e->sp.width, e->sp.height, e->sp.input_bitdepth, scale, layout) : 0;
}
int thor_hip_scale_taps(int S, int T, int filter, int cosited, int i, int* first, short* coeff, int cap) {
  int16_t c[SCALE_MAX_TAPS];
  int f = 0;
  if (!first || !coeff || cap < 1) return 0;
  const int n = scale_taps(S, T, filter, cosited, i, &f, c, cap < SCALE_MAX_TAPS ? cap : SCALE_MAX_TAPS);
  for (int j = 0; j < n; j++) coeff[j] = c[j];
  if (n) *first = f;
  return n;
}
int thor_hip_stage_frame_scaled(thor_hip_encoder* e, int stream, int slot, const void* frame, const thor_hip_scale* scale, const thor_hip_frame_layout* layout,
                                int on_device) {
  PixLayout L;
  if (!e || stream < 0 || stream >= e->S || slot < 0 || !frame) return 1;
  if (!scale_args_resolved(scale, layout, e->sp.width, e->sp.height, e->sp.input_bitdepth, L) || (uintptr_t)frame % (e->sp.input_bitdepth > 8 ? 2 : 1)) return 1;
  static const thor_hip_frame_layout packed = {sizeof(thor_hip_frame_layout), THOR_HIP_CHROMA_PLANAR, 0, 0, 0, 0, 0};
  const thor_hip_frame_layout* l = layout ? layout : &packed;
  ENC_DISPATCH(e, {
    // the tap tables: kept from the last call with this geometry, else built now - still before the device is touched
    if (!E.eng.resolve_scaled(scale->src_width, scale->src_height, scale->filter, scale->chroma_site, l->chroma, l->msb_aligned, l->pitch_y, l->pitch_c,
                              l->offset_u, l->offset_v))
      return 1;
    auto& v = E.staged[stream];
    if ((int)v.size() <= slot) v.resize(slot + 1);
    if (!v[slot].base_y) v[slot].alloc(e->sp.width, e->sp.height, 0);
    if (on_device) {  // the kernel reads the caller's buffer and writes the slot
      E.eng.scale_in(frame, v[slot].p);
      HIPCHECK(hipStreamSynchronize(g_stream));
    } else
      E.eng.stage_scaled_host(frame, v[slot].p);
  });
  return 0;
}
// ---- rate control: tk_rc.h, k_rc_cost ----
// The caller's structure as an RcConfig; false: refused (a wrong `size` included).  NULL is a config that is off.  Touches no device.
static bool rc_resolved(const thor_hip_rate_control* rc, RcConfig& c) {
  if (!rc) { c = RcConfig(); return true; }
  if (rc->size != (int)sizeof(thor_hip_rate_control)) return false;
  return rc_resolve(rc->bitrate, rc->buffer_ms, rc->min_qp, rc->max_qp, rc->min_qp_i, rc->max_qp_i, rc->initial_qp, c);
}
int thor_hip_rate_control_check(const thor_hip_rate_control* rc) {
  RcConfig c;
  return rc_resolved(rc, c) ? 0 : 1;
}
int thor_hip_set_rate_control(thor_hip_encoder* e, int stream, const thor_hip_rate_control* rc) {
  RcConfig c;
  if (!e || stream < 0 || stream >= e->S || !rc_resolved(rc, c)) return 1;
  if (!ENC_STREAM(e, stream, log.empty())) return 2;   // in the middle of a sequence
  ENC_DISPATCH(e, { E.eng.set_rate_control(stream, c); });
  return 0;
}
int thor_hip_get_frame_rc(const thor_hip_encoder* e, int stream, int i, thor_hip_frame_rc* out) {
  if (!e || stream < 0 || stream >= e->S || !out) return 1;
  const std::vector<RcStat>& log = ENC_STREAM(e, stream, rclog);
  if (i < 0 || i >= (int)log.size()) return 1;
  const RcStat& r = log[i];
  memset(out, 0, sizeof(*out));
  out->base_qp = r.base_qp; out->frame_class = r.frame_class;
  out->sum_intra = r.sum_intra; out->sum_best = r.sum_best; out->n_intra = r.n_intra;
  out->fullness = r.fullness; out->buffer_bits = r.buffer_bits; out->target_bits = r.target_bits; out->overflows = r.overflows;
  return 0;
}
// ---- key frames: GopScheduler::promote, tk_rc.h ScConfig, k_rc_cost<PIX, true> ----
int thor_hip_force_key_frame(thor_hip_encoder* e, int stream, int display_index) {
  if (!e) return 1;
  if (e->sp.num_reorder_pics != 0) return 2;   // low delay only
  if (stream < 0 || stream >= e->S) return 1;
  int r = 1;
  ENC_DISPATCH(e, { r = E.eng.force_key_frame(stream, display_index, E.pending[stream] != 0); });
  return r;
}
static bool sc_resolved(const thor_hip_scene_cut* sc, ScConfig& c) {
  if (!sc) { c = ScConfig(); return true; }
  if (sc->size != (int)sizeof(thor_hip_scene_cut)) return false;
  return sc_resolve(sc->percent, sc->min_interval, c);
}
int thor_hip_scene_cut_check(const thor_hip_scene_cut* sc) {
  ScConfig c;
  return sc_resolved(sc, c) ? 0 : 1;
}
int thor_hip_set_scene_cut(thor_hip_encoder* e, int stream, const thor_hip_scene_cut* sc) {
  ScConfig c;
  if (!e) return 1;
  if (e->sp.num_reorder_pics != 0) return 2;   // low delay only
  if (stream < 0 || stream >= e->S || !sc_resolved(sc, c)) return 1;
  if (!ENC_STREAM(e, stream, log.empty())) return 2;   // in the middle of a sequence
  ENC_DISPATCH(e, { E.eng.set_scene_cut(stream, c); });
  return 0;
}
int thor_hip_scene_cost(thor_hip_encoder* e, int stream, int slot, int prev_slot, unsigned long long sums[3]) {
  if (!e || !sums) return 1;
  if (e->sp.num_reorder_pics != 0) return 2;   // low delay only
  if (stream < 0 || stream >= e->S) return 1;
  int r = 0;
  ENC_DISPATCH(e, {
    auto& v = E.staged[stream];
    auto staged = [&](int i) { return i >= 0 && i < (int)v.size() && v[i].base_y; };
    if (!staged(slot) || (prev_slot != -1 && !staged(prev_slot))) r = 1;
    else E.eng.scene_cost(v[slot], prev_slot == -1 ? nullptr : &v[prev_slot], sums);
  });
  return r;
}
int thor_hip_get_frame_key(const thor_hip_encoder* e, int stream, int i, thor_hip_frame_key* out) {
  if (!e || stream < 0 || stream >= e->S || !out) return 1;
  const std::vector<FrameStat>& log = ENC_STREAM(e, stream, log);
  if (i < 0 || i >= (int)log.size()) return 1;
  memset(out, 0, sizeof(*out));
  out->reason = log[i].key_reason;
  out->sum_intra = log[i].key_sums[0]; out->sum_best = log[i].key_sums[1]; out->n_intra = log[i].key_sums[2];
  return 0;
}
// ---- temporal filter: tk_tf.h, k_tf_search / k_tf_blend ----
static_assert(sizeof(thor_hip_tf_request) == sizeof(TfRequest), "thor_hip_tf_request and tk::TfRequest are one layout");
int thor_hip_temporal_filter_check(const thor_hip_temporal_filter* tf) {
  return tf && tf->size == (int)sizeof(thor_hip_temporal_filter) && tf_strength_ok(tf->strength) ? 0 : 1;
}
int thor_hip_filter_staged(thor_hip_encoder* e, const thor_hip_tf_request* req, int n, const thor_hip_temporal_filter* tf) {
  if (!e || !req || n < 1 || n > 4096 || thor_hip_temporal_filter_check(tf)) return 1;
  const TfRequest* rq = (const TfRequest*)req;
  ENC_DISPATCH(e, {
    auto staged = [&](int s, int i) { return i >= 0 && i < (int)E.staged[s].size() && E.staged[s][i].base_y; };
    if (!tf_requests_ok(rq, n, e->S, staged)) return 1;
    for (int i = 0; i < n; i++) {   // the destinations first: growing a stream's slot array moves its frames' records
      auto& v = E.staged[rq[i].stream];
      if ((int)v.size() <= rq[i].dst_slot) v.resize(rq[i].dst_slot + 1);
      if (!v[rq[i].dst_slot].base_y) v[rq[i].dst_slot].alloc(e->sp.width, e->sp.height, 0);
    }
    std::vector<typename Engine<PIXT>::TfItem> it(n);
    for (int i = 0; i < n; i++) {
      auto& v = E.staged[rq[i].stream];
      it[i].cur = &v[rq[i].slot]; it[i].dst = &v[rq[i].dst_slot]; it[i].nrefs = rq[i].nrefs;
      for (int k = 0; k < rq[i].nrefs; k++) { it[i].ref[k] = &v[rq[i].ref_slot[k]]; it[i].dist[k] = rq[i].ref_dist[k]; }
    }
    E.eng.filter_frames(it.data(), n, tf->strength);
  });
  return 0;
}
int thor_hip_get_staged(thor_hip_encoder* e, int stream, int slot, void* yuv_out) {
  if (!e || stream < 0 || stream >= e->S || slot < 0 || !yuv_out) return 1;
  ENC_DISPATCH(e, {
    auto& v = E.staged[stream];
    if (slot >= (int)v.size() || !v[slot].base_y) return 1;
    HIPCHECK(hipStreamSynchronize(g_stream));
    download_yuv(v[slot], (PIXT*)yuv_out, e->sp.width, e->sp.height);
  });
  return 0;
}
void thor_hip_kernel_time(thor_hip_encoder*, double* sb_ms, long* sb_launches, double* filter_ms) {
  if (sb_ms) *sb_ms = g_clk.sb_ms;
  if (sb_launches) *sb_launches = g_clk.sb_launches;
  if (filter_ms) *filter_ms = g_clk.filt_ms;
}
void thor_hip_read_prof(thor_hip_encoder* e, long long out[32]) { if (!e || !out) return; ENC_DISPATCH(e, { backend::d2h(out, E.eng.d_prof, 32 * sizeof(long long)); }); }
void thor_hip_kernel_time_reset(thor_hip_encoder*) { g_clk.sb_ms = g_clk.filt_ms = 0; g_clk.sb_launches = 0; }
void thor_hip_read_stats(thor_hip_encoder* e, unsigned long long out[4], int reset) {
  if (!e || !out) return;
  ENC_DISPATCH(e, { backend::d2h(out, E.eng.d_stats, 4 * sizeof(unsigned long long)); if (reset) backend::dev_memset(E.eng.d_stats, 0, 8 * sizeof(unsigned long long)); });
}

void thor_hip_set_frame_distortion(thor_hip_encoder* e, int on) {
  if (!e) return;
  ENC_DISPATCH(e, { E.eng.frame_distortion = on != 0; });
}
static const std::vector<FrameStat>* stream_log(const thor_hip_encoder* e, int stream) {
  if (!e || stream < 0 || stream >= e->S) return nullptr;
  return &ENC_STREAM(e, stream, log);
}
static int stream_sh_bits(const thor_hip_encoder* e, int stream) { return ENC_STREAM(e, stream, sh_bits); }
static int copy_out(const std::string& r, char* buf, size_t n) {
  if (buf && n) { const size_t k = r.size() < n - 1 ? r.size() : n - 1; memcpy(buf, r.data(), k); buf[k] = 0; }
  return (int)r.size();
}
int thor_hip_frame_stats_count(const thor_hip_encoder* e, int stream) {
  const std::vector<FrameStat>* log = stream_log(e, stream);
  return log ? (int)log->size() : 0;
}
int thor_hip_get_frame_stats(const thor_hip_encoder* e, int stream, int i, thor_hip_frame_stats* out) {
  const std::vector<FrameStat>* log = stream_log(e, stream);
  if (!log || !out || i < 0 || i >= (int)log->size()) return 1;
  const FrameStat& f = (*log)[i];
  memset(out, 0, sizeof(*out));
  out->display_index = f.display; out->frame_type = f.frame_type; out->qp = f.qp; out->num_bits = f.num_bits; out->num_ref = f.num_ref;
  for (int k = 0; k < 4; k++) { out->ref_array[k] = f.ref_array[k]; out->ref_frame_num[k] = f.ref_array[k] < 0 ? -1 : f.ref_frame_num[k]; }
  out->has_sse = f.has_sse;
  for (int k = 0; k < 3; k++) out->sse[k] = f.sse[k];
  frame_psnr(f, e->sp.width, e->sp.height, e->sp.input_bitdepth, out->psnr);
  return 0;
}
int thor_hip_report(const thor_hip_encoder* e, int stream, char* buf, size_t n) {
  const std::vector<FrameStat>* log = stream_log(e, stream);
  if (!log) return -1;
  return copy_out(format_report(*log, stream_sh_bits(e, stream), e->sp.max_num_ref, e->sp.frame_rate, e->sp.width, e->sp.height, e->sp.input_bitdepth), buf, n);
}
int thor_hip_stat_line(const thor_hip_encoder* e, int stream, int num_frames, char* buf, size_t n) {
  const std::vector<FrameStat>* log = stream_log(e, stream);
  if (!log) return -1;
  return copy_out(format_stat_line(*log, stream_sh_bits(e, stream), e->sp.frame_rate, e->sp.width, e->sp.height, e->sp.input_bitdepth, num_frames), buf, n);
}

}  // extern "C"
