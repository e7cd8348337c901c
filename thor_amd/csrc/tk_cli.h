// tk_cli.h - minimal Thorenc-compatible option/config-file reader for the test drivers.
// Same surface as enc/strings.c:287-356 for the options this path honours: "-name value" tokens,
// ';' starts a comment, "-cf file" includes a config file (command line wins over later files,
// like the reference, because explicit arguments are applied after the config contents).
#pragma once
#include <map>
#include <string>
#include <vector>
#include <fstream>
#include <sstream>
#include <cstdlib>
#include "tk_encoder.h"

namespace tk {

struct CliArgs {
  SeqParams sp;
  std::string infile, outfile, recfile;
  int num_frames = 600, skip = 0, streams = 1;
  int snrcalc = 1;           // -snrcalc (enc/strings.c:340): PSNR of every frame in the report
  std::string statfile;      // -stat FILE: one summary line per stream appended (enc/mainenc.c:652-667)
  std::string pixfmt = "i420";  // -pixfmt i420|nv12|nv21|p010|rgba|bgra|rgb24|bgr24: layout of the -if and -rf files (tight rows; not an option of the reference)
  // RGB files (-pixfmt rgba|bgra|rgb24|bgr24; one byte per channel with 8-bit input, else 16-bit words with the value in the low bits):
  int rgb_matrix = 1;        // -rgbmatrix 601|709|2020 -> 0, 1, 2
  int rgb_full = 0;          // -rgbrange limited|full
  int rgb_site = 1;          // -rgbsite centre|left
  bool rgb_given = false;    // one of the three was given: front-end options like -pixfmt
  // -if frames of another size, resampled to -width x -height on the device (tk_scale.h); -pixfmt then describes them at that size, -rf stays at the coded size
  int src_w = 0, src_h = 0;  // -src_width, -src_height (0: the coded size)
  int scale_filter = 1;      // -scale_filter bilinear|bicubic
  int scale_site = 1;        // -scale_site left|centre
  bool scale_given = false;  // one of the four was given: front-end options like -pixfmt
  // -rc_bitrate N [-rc_buffer_ms -rc_min_qp -rc_max_qp -rc_min_qpI -rc_max_qpI -rc_initial_qp]: the library's rate control (tk_rc.h), the same target for every
  // stream.  Not options of the reference: its -bitrate / -max_qp ... keep their handling below.
  int rc[7] = {0, 0, 0, 0, 0, 0, 0};  // bitrate, buffer_ms, min_qp, max_qp, min_qp_i, max_qp_i, initial_qp
  bool rc_given = false;     // one of the seven was given: front-end options like -pixfmt
  // -key_frames a,b,c: key frames at these chunk-relative frames; -key_scenecut PCT [-key_min_interval N]: scene cuts (tk_rc.h: ScConfig).  The same for every
  // stream, low delay only.  -key_scenecut has no default: 0 is off.
  std::vector<int> key_frames;
  int key_scenecut = 0, key_min_interval = 0;
  bool key_given = false;    // one of the three was given: front-end options like -pixfmt
  // -tf_strength S [-tf_past P -tf_future F]: the temporal noise filter (tk_tf.h) of every frame against its P previous and F next frames of the chunk (each 0 .. 2;
  // frames beyond the ends of the chunk are dropped from the list) before it is coded.  S = 0 (the default) is off; P and F default to 0.
  int tf_strength = 0, tf_past = 0, tf_future = 0;
  bool tf_given = false;     // one of the three was given: front-end options like -pixfmt
  // Options of the reference's table (enc/strings.c:287-356) this path does not implement.  A value other than
  // the reference's default would change the bitstream, so it is recorded here and rejected by the caller
  // (thor_hip_params_set / thor_hip_params_from_config return non-zero, the CLI tools exit) - never ignored.
  std::string unsupported;   // first "-name value" that cannot be honoured
  std::string unknown;       // first option that is not in the reference's table at all
};

static inline void cli_tokens_from_file(const std::string& path, std::vector<std::string>& out) {
  std::ifstream f(path);
  if (!f) { fprintf(stderr, "cannot open config %s\n", path.c_str()); exit(2); }
  std::string line;
  while (std::getline(f, line)) {
    size_t sc = line.find(';');
    if (sc != std::string::npos) line.resize(sc);
    std::istringstream is(line);
    std::string tok;
    while (is >> tok) out.push_back(tok);
  }
}

// -pixfmt rgba|bgra|rgb24|bgr24 as an order of RgbFormat (resolve_rgb); -1: not an RGB format
static inline int cli_rgb_order(const std::string& pixfmt) { return pixfmt == "rgba" ? 0 : pixfmt == "bgra" ? 1 : pixfmt == "rgb24" ? 4 : pixfmt == "bgr24" ? 5 : -1; }

static inline void cli_apply(CliArgs& a, const std::vector<std::string>& t) {
  for (size_t i = 0; i + 1 < t.size(); i += 2) {
    const std::string& k = t[i];
    const std::string& v = t[i + 1];
    SeqParams& p = a.sp;
    auto I = [&]() { return atoi(v.c_str()); };
    auto F = [&]() { return (float)atof(v.c_str()); };
    if (k == "-cf") { std::vector<std::string> sub; cli_tokens_from_file(v, sub); cli_apply(a, sub); }
    else if (k == "-if") a.infile = v;
    else if (k == "-of") a.outfile = v;
    else if (k == "-rf") a.recfile = v;
    else if (k == "-n") a.num_frames = I();
    else if (k == "-skip") a.skip = I();
    else if (k == "-streams") a.streams = I();
    else if (k == "-snrcalc") a.snrcalc = I();
    else if (k == "-stat") a.statfile = v;
    else if (k == "-pixfmt") {
      a.pixfmt = v;
      if (v != "i420" && v != "nv12" && v != "nv21" && v != "p010" && cli_rgb_order(v) < 0 && a.unsupported.empty()) a.unsupported = k + " " + v;
    }
    else if (k == "-rgbmatrix" || k == "-rgbrange" || k == "-rgbsite") {
      a.rgb_given = true;
      bool ok = true;
      if (k == "-rgbmatrix") { a.rgb_matrix = v == "601" ? 0 : v == "709" ? 1 : 2; ok = v == "601" || v == "709" || v == "2020"; }
      else if (k == "-rgbrange") { a.rgb_full = v == "full"; ok = v == "full" || v == "limited"; }
      else { a.rgb_site = v == "left"; ok = v == "left" || v == "centre"; }
      if (!ok && a.unsupported.empty()) a.unsupported = k + " " + v;
    }
    else if (k == "-src_width" || k == "-src_height" || k == "-scale_filter" || k == "-scale_site") {
      a.scale_given = true;
      bool ok = true;
      if (k == "-src_width") { a.src_w = I(); ok = a.src_w > 0; }
      else if (k == "-src_height") { a.src_h = I(); ok = a.src_h > 0; }
      else if (k == "-scale_filter") { a.scale_filter = v == "bicubic"; ok = v == "bicubic" || v == "bilinear"; }
      else { a.scale_site = v == "left"; ok = v == "left" || v == "centre"; }
      if (!ok && a.unsupported.empty()) a.unsupported = k + " " + v;
    }
    else if (k.compare(0, 4, "-rc_") == 0) {
      static const char* const names[7] = {"-rc_bitrate", "-rc_buffer_ms", "-rc_min_qp", "-rc_max_qp", "-rc_min_qpI", "-rc_max_qpI", "-rc_initial_qp"};
      int which = -1;
      for (int j = 0; j < 7; j++) if (k == names[j]) which = j;
      if (which < 0) { if (a.unknown.empty()) a.unknown = k; }
      else {
        a.rc_given = true;
        a.rc[which] = I();
        if ((a.rc[which] < 0 || (which >= 2 && a.rc[which] > 51)) && a.unsupported.empty()) a.unsupported = k + " " + v;   // the set as a whole: cli_parse
      }
    }
    else if (k == "-key_frames" || k == "-key_scenecut" || k == "-key_min_interval") {
      a.key_given = true;
      bool ok = true;
      if (k == "-key_frames") {
        a.key_frames.clear();
        std::istringstream is(v);
        std::string tok;
        while (std::getline(is, tok, ',')) {
          ok = ok && !tok.empty() && tok.find_first_not_of("0123456789") == std::string::npos;
          if (ok) a.key_frames.push_back(atoi(tok.c_str()));
        }
        ok = ok && !a.key_frames.empty() && (int)a.key_frames.size() <= kMaxKeyRequests;
      }
      else if (k == "-key_scenecut") { a.key_scenecut = I(); ok = a.key_scenecut >= 0 && a.key_scenecut <= 100; }
      else { a.key_min_interval = I(); ok = a.key_min_interval >= 0; }
      if (!ok && a.unsupported.empty()) a.unsupported = k + " " + v;
    }
    else if (k == "-tf_strength" || k == "-tf_past" || k == "-tf_future") {
      a.tf_given = true;
      bool ok = true;
      if (k == "-tf_strength") { a.tf_strength = I(); ok = a.tf_strength == 0 || tf_strength_ok(a.tf_strength); }
      else if (k == "-tf_past") { a.tf_past = I(); ok = a.tf_past >= 0 && a.tf_past <= 2; }
      else { a.tf_future = I(); ok = a.tf_future >= 0 && a.tf_future <= 2; }
      if (!ok && a.unsupported.empty()) a.unsupported = k + " " + v;
    }
    else if (k == "-width") p.width = I();
    else if (k == "-height") p.height = I();
    else if (k == "-qp") p.qp = I();
    else if (k == "-f") p.frame_rate = F();
    else if (k == "-lambda_coeffI") p.lambda_coeffI = F();
    else if (k == "-lambda_coeffP") p.lambda_coeffP = F();
    else if (k == "-early_skip_thr") p.early_skip_thr = F();
    else if (k == "-enable_tb_split") p.enable_tb_split = I();
    else if (k == "-enable_pb_split") p.enable_pb_split = I();
    else if (k == "-max_num_ref") p.max_num_ref = I();
    else if (k == "-HQperiod") p.HQperiod = I();
    else if (k == "-num_reorder_pics") p.num_reorder_pics = I();
    else if (k == "-interp_ref") p.interp_ref = I();
    else if (k == "-max_clpf_strength") p.max_clpf_strength = I();
    else if (k == "-dqpP") p.dqpP = I();
    else if (k == "-dqpB") p.dqpB = I();
    else if (k == "-dqpB0") p.dqpB0 = I();
    else if (k == "-dqpB1") p.dqpB1 = I();
    else if (k == "-dqpB2") p.dqpB2 = I();
    else if (k == "-dqpB3") p.dqpB3 = I();
    else if (k == "-mqpB") p.mqpB = F();
    else if (k == "-mqpB0") p.mqpB0 = F();
    else if (k == "-mqpB1") p.mqpB1 = F();
    else if (k == "-mqpB2") p.mqpB2 = F();
    else if (k == "-mqpB3") p.mqpB3 = F();
    else if (k == "-lambda_coeffB") p.lambda_coeffB = F();
    else if (k == "-lambda_coeffB0") p.lambda_coeffB0 = F();
    else if (k == "-lambda_coeffB1") p.lambda_coeffB1 = F();
    else if (k == "-lambda_coeffB2") p.lambda_coeffB2 = F();
    else if (k == "-lambda_coeffB3") p.lambda_coeffB3 = F();
    else if (k == "-dyadic_coding") p.dyadic_coding = I();
    else if (k == "-dqpI") p.dqpI = I();
    else if (k == "-mqpP") p.mqpP = F();
    else if (k == "-intra_period") p.intra_period = I();
    else if (k == "-intra_rdo") p.intra_rdo = I();
    else if (k == "-encoder_speed") p.encoder_speed = I();
    else if (k == "-deblocking") p.deblocking = I();
    else if (k == "-cdef") p.cdef = I();
    else if (k == "-clpf") p.clpf = I();
    else if (k == "-use_block_contexts") p.use_block_contexts = I();
    else if (k == "-enable_bipred") p.enable_bipred = I();
    else if (k == "-enable_cfl_intra") p.cfl_intra = I();
    else if (k == "-enable_cfl_inter") p.cfl_inter = I();
    else if (k == "-bitdepth") p.bitdepth = I();
    else if (k == "-input_bitdepth") p.input_bitdepth = I();
    else if (k == "-log2_sb_size") {
      // 64x64 or 128x128 superblocks.  The reference's own range check (enc/strings.c:527) compares against MAX_SB_SIZE instead of its
      // logarithm and lets 8 and more through into buffers sized for 128; here everything but 6 and 7 is refused.
      p.log2_sb_size = I();
      if (p.log2_sb_size != 6 && p.log2_sb_size != 7 && a.unsupported.empty()) a.unsupported = k + " " + v;
    }
    else {
      // the rest of the reference's table: harmless at their defaults (or never read by the block path), fatal otherwise
      struct Opt { const char* name; const char* dflt; };  // dflt == nullptr: any value is fine (I/O and reporting options)
      static const Opt rest[] = {{"-ph", "0"}, {"-fh", "0"},
                                 {"-max_delta_qp", "0"}, {"-delta_qp_step", nullptr}, {"-sync", "0"}, {"-bitrate", "0"},
                                 {"-max_qp", nullptr}, {"-min_qp", nullptr}, {"-max_qpI", nullptr}, {"-min_qpI", nullptr},
                                 {"-qmtx", "0"}, {"-qmtx_offset", nullptr}, {"-subsample", "420"}, {"-frame_bitdepth", nullptr}};
      bool found = false;
      for (const Opt& o : rest)
        if (k == o.name) {
          found = true;
          if (o.dflt && atoi(v.c_str()) != atoi(o.dflt) && a.unsupported.empty()) a.unsupported = k + " " + v;
        }
      if (!found && a.unknown.empty()) a.unknown = k;
    }
  }
  if (t.size() & 1) { if (a.unknown.empty()) a.unknown = t.back() + " (no value)"; }
}

static inline CliArgs cli_parse(int argc, char** argv) {
  CliArgs a;
  std::vector<std::string> t;
  for (int i = 1; i < argc; i++) t.push_back(argv[i]);
  // config files first, explicit arguments afterwards (enc/strings.c:196-265 applies argv last)
  std::vector<std::string> files, rest;
  for (size_t i = 0; i + 1 < t.size(); i += 2) {
    if (t[i] == "-cf") { files.push_back(t[i]); files.push_back(t[i + 1]); }
    else { rest.push_back(t[i]); rest.push_back(t[i + 1]); }
  }
  cli_apply(a, files);
  cli_apply(a, rest);
  if (!a.unknown.empty()) { fprintf(stderr, "Run-time error...\nunknown option %s\n...now exiting to system...\n", a.unknown.c_str()); exit(2); }
  if (!a.unsupported.empty()) { fprintf(stderr, "Run-time error...\noption %s is not implemented by this path (it changes the bitstream)\n...now exiting to system...\n", a.unsupported.c_str()); exit(2); }
  RcConfig rcc;
  if (a.rc_given && !rc_resolve(a.rc[0], a.rc[1], a.rc[2], a.rc[3], a.rc[4], a.rc[5], a.rc[6], rcc)) { fprintf(stderr, "Run-time error...\nthe -rc_ options do not describe a rate control (a minimum above its maximum)\n...now exiting to system...\n"); exit(2); }
  if (a.key_given && a.sp.num_reorder_pics != 0) { fprintf(stderr, "Run-time error...\nthe -key_ options need a low-delay configuration (num_reorder_pics 0)\n...now exiting to system...\n"); exit(2); }
  return a;
}

// -pixfmt as a tight layout of a width x height picture: nv12 / nv21 interleave the chroma samples, p010 does so with the samples in the high bits
// of 16-bit words (any input depth above 8).  false: the format cannot hold input of this depth (p010 with 8-bit input).
static inline bool cli_pixfmt_layout(const std::string& pixfmt, int width, int height, int input_bitdepth, PixLayout& L) {
  const int chroma = pixfmt == "i420" ? 0 : pixfmt == "nv21" ? 2 : 1;
  return resolve_layout(chroma, pixfmt == "p010", 0, 0, 0, 0, width, height, input_bitdepth, L);
}

// Encode `num_frames` frames of a raw 4:2:0 file with S identical-geometry streams: stream s
// codes frames [skip + s*num_frames, skip + (s+1)*num_frames) as its own closed stream (what the
// reference produces with -skip/-n).  Outputs "<of>" for S==1, "<of>.<s>" otherwise.
// stdout: the reference's report (tk_report.h); with S > 1 every stream's, in stream order, each after a line "stream <s>".
template <typename PIX> int cli_run(const CliArgs& a) {
  const SeqParams& p = a.sp;
  PixLayout lay;
  RgbFormat rgb;
  const bool use_rgb = cli_rgb_order(a.pixfmt) >= 0;   // tight rows, a byte per channel with 8-bit input, else 16-bit words with the value in the low bits
  if (use_rgb && !resolve_rgb(cli_rgb_order(a.pixfmt), p.input_bitdepth > 8 ? 16 : 8, 0, a.rgb_matrix, a.rgb_full, a.rgb_site, 0, 0, p.width, p.height, p.input_bitdepth, rgb)) {
    fprintf(stderr, "Run-time error...\n-pixfmt %s cannot hold this picture\n...now exiting to system...\n", a.pixfmt.c_str());
    return 2;
  }
  const bool use_layout = a.pixfmt != "i420" && !use_rgb;   // i420 is the path the files always took
  if (!use_rgb && !cli_pixfmt_layout(a.pixfmt, p.width, p.height, p.input_bitdepth, lay)) {
    fprintf(stderr, "Run-time error...\n-pixfmt %s needs input_bitdepth above 8\n...now exiting to system...\n", a.pixfmt.c_str());
    return 2;
  }
  // -src_width / -src_height: the -if frames have that size, in the -pixfmt layout, and are resampled while they are staged
  const bool use_scale = a.scale_given;
  const int src_w = a.src_w ? a.src_w : p.width, src_h = a.src_h ? a.src_h : p.height;
  const int src_chroma = a.pixfmt == "i420" ? 0 : a.pixfmt == "nv21" ? 2 : 1, src_msb = a.pixfmt == "p010";
  PixLayout slay;
  if (use_scale && (use_rgb || !resolve_scale_args(src_w, src_h, a.scale_filter, a.scale_site, src_chroma, src_msb, 0, 0, 0, 0, p.width, p.height, p.input_bitdepth, slay))) {
    fprintf(stderr, "Run-time error...\n-src_width %d -src_height %d with -pixfmt %s cannot be resampled to %dx%d\n...now exiting to system...\n", src_w, src_h,
            a.pixfmt.c_str(), p.width, p.height);
    return 2;
  }
  FILE* fi = fopen(a.infile.c_str(), "rb");
  if (!fi) { fprintf(stderr, "cannot open %s\n", a.infile.c_str()); return 2; }
  Engine<PIX> eng;
  eng.frame_distortion = a.snrcalc != 0;
  eng.open(p, a.streams);
  if (use_scale && !eng.resolve_scaled(src_w, src_h, a.scale_filter, a.scale_site, src_chroma, src_msb, 0, 0, 0, 0)) {
    fprintf(stderr, "Run-time error...\nno tap table for %dx%d -> %dx%d\n...now exiting to system...\n", src_w, src_h, p.width, p.height);
    return 2;
  }
  const size_t rsz = use_rgb ? rgb.bytes : eng.frame_bytes();  // the files hold input-depth samples (-if and -rf: common/common_frame.c:484-650), or RGB frames
  const size_t fsz = use_scale ? slay.bytes : rsz;             // -if at the source size
  std::vector<uint8_t> frame(fsz), rec(rsz);
  std::vector<FILE*> fr(a.streams, nullptr);
  auto name = [&](const std::string& base, int s) { return a.streams == 1 ? base : base + "." + std::to_string(s); };
  for (int s = 0; s < a.streams; s++)
    if (!a.recfile.empty()) fr[s] = fopen(name(a.recfile, s).c_str(), "wb");
  // all streams run in lock step through their (identical) coding-order schedules
  fseek(fi, 0, SEEK_END);
  const int file_frames = (int)(ftell(fi) / (long)fsz);
  for (int s = 0; s < a.streams; s++) eng.begin_sequence(s, a.skip + s * a.num_frames, a.num_frames, file_frames);
  RcConfig rcc;
  if (a.rc_given && rc_resolve(a.rc[0], a.rc[1], a.rc[2], a.rc[3], a.rc[4], a.rc[5], a.rc[6], rcc) && rcc.on())
    for (int s = 0; s < a.streams; s++) {
      RcConfig c = rcc;
      // THOR_RC_SCALE=k (tests): stream s aims at (1 + k * s) times the bitrate, so that one engine holds streams with different targets
      if (const char* sc = getenv("THOR_RC_SCALE")) c.bitrate = (int)((long long)c.bitrate * (1 + atoi(sc) * s));
      eng.set_rate_control(s, c);
    }
  if (a.key_given)
    for (int s = 0; s < a.streams; s++) {
      // THOR_KEY_SHIFT=k (tests): stream s asks for its key frames k * s frames later, so that one engine holds streams with different requests
      const int shift = getenv("THOR_KEY_SHIFT") ? atoi(getenv("THOR_KEY_SHIFT")) * s : 0;
      for (int f : a.key_frames)
        if (f + shift < a.num_frames && eng.force_key_frame(s, f + shift, false)) { fprintf(stderr, "Run-time error...\n-key_frames: frame %d cannot be a key frame\n...now exiting to system...\n", f + shift); return 2; }
      ScConfig scc;
      if (sc_resolve(a.key_scenecut, a.key_min_interval, scc) && scc.on()) eng.set_scene_cut(s, scc);
    }
  std::vector<std::vector<uint8_t>> recs((size_t)a.streams * a.num_frames);  // recon in display order
  auto upload_plain = [&](int s) { if (use_scale) eng.stage_scaled_host(frame.data(), eng.st[s].orig.p); else if (use_rgb) eng.stage_rgb_host(frame.data(), rgb, eng.st[s].orig.p); else if (use_layout) eng.stage_layout_host(frame.data(), lay, eng.st[s].orig.p); else eng.upload_orig(s, frame.data()); };
  auto read_frame = [&](size_t idx) {
    if (fseek(fi, (long)(idx * fsz), SEEK_SET) || fread(frame.data(), 1, fsz, fi) != fsz) { fprintf(stderr, "short read at frame %zu\n", idx); return false; }
    return true;
  };
  // The scheduled frame of stream s into its original.  -tf_strength: the frame and its neighbours of the chunk are staged in frames of their own and the filter
  // writes the stream's original - what thorenc_hip does with staging slots beyond the chunk.
  std::vector<DevFrame<PIX>> tfbuf;
  auto load = [&](int s) -> bool {
    if (a.tf_strength == 0) {
      if (!read_frame((size_t)eng.st[s].cur_abs)) return false;
      upload_plain(s);
      return true;
    }
    if (tfbuf.empty()) {
      tfbuf.resize(1 + TF_MAX_REFS);
      for (auto& b : tfbuf) b.alloc(p.width, p.height, 0);
    }
    const int f = eng.st[s].cur.frame_num;
    const size_t base = (size_t)eng.st[s].cur_abs - (size_t)f;
    typename Engine<PIX>::TfItem it;
    it.cur = &tfbuf[0]; it.dst = &eng.st[s].orig; it.nrefs = 0;
    int nb[TF_MAX_REFS];
    for (int d = 1; d <= a.tf_past; d++) if (f - d >= 0) { nb[it.nrefs] = f - d; it.dist[it.nrefs++] = d; }
    for (int d = 1; d <= a.tf_future; d++) if (f + d < a.num_frames) { nb[it.nrefs] = f + d; it.dist[it.nrefs++] = d; }
    const DevFrame<PIX> keep = eng.st[s].orig;
    for (int k = 0; k <= it.nrefs; k++) {
      if (!read_frame(base + (size_t)(k ? nb[k - 1] : f))) return false;
      eng.st[s].orig = tfbuf[k];
      upload_plain(s);
      if (k) it.ref[k - 1] = &tfbuf[k];
    }
    eng.st[s].orig = keep;
    eng.filter_frames(&it, 1, a.tf_strength);
    return true;
  };
  auto download = [&](int s) { if (use_rgb) eng.fetch_rgb_host(eng.st[s].rec.p, rec.data(), rgb); else if (use_layout) eng.fetch_layout_host(eng.st[s].rec.p, rec.data(), lay); else eng.download_rec(s, rec.data()); };
  // THOR_STAGGER=1 (tests): the streams in two groups half a frame apart (Engine::encode_run) instead of lock step
  if (getenv("THOR_STAGGER") && atoi(getenv("THOR_STAGGER")) && a.streams > 1) {
    int rc = 0;
    eng.encode_run(a.num_frames,
        [&](int s) -> bool {
          if (!eng.schedule(s)) return false;
          if (!load(s)) { rc = 3; return false; }
          return true;
        },
        [&](int first, int count) {
          for (int s = first; s < first + count; s++)
            if (fr[s]) { download(s); recs[(size_t)s * a.num_frames + eng.st[s].cur.frame_num] = rec; }
        });
    if (rc) return rc;
  } else
  for (;;) {
    std::vector<FrameParams> fp(a.streams);
    int active = 0;
    for (int s = 0; s < a.streams; s++) {
      if (!eng.schedule(s)) continue;
      active++;
      if (!load(s)) return 3;
      fp[s] = eng.st[s].cur;
    }
    if (!active) break;
    if (active != a.streams) { fprintf(stderr, "streams out of step\n"); return 4; }
    eng.encode_frames(fp);
    if (const char* ddp = getenv("THOR_DD_DUMP")) {   // tests: stream 0's block data in the record format of oracle/dd_shim.c
      std::vector<DbCell> cells(eng.num_cells());
      eng.download_cells(0, cells.data());
      FILE* fd = fopen(ddp, "ab");
      if (!fd) { fprintf(stderr, "cannot open %s\n", ddp); return 5; }
      const int32_t hdr[3] = {0x44444444, fp[0].frame_num, (int32_t)cells.size()};
      fwrite(hdr, sizeof hdr, 1, fd);
      for (const DbCell& c : cells) {
        const DdFields d = dd_fields(c);
        const int32_t r[14] = {d.mode, d.cbp_y, d.cbp_u, d.cbp_v, d.size, d.tb_split, d.pb_part, d.mv0x, d.mv0y, d.mv1x, d.mv1y, d.ref_idx0, d.ref_idx1, d.bipred_flag};
        fwrite(r, sizeof r, 1, fd);
      }
      fclose(fd);
    }
    for (int s = 0; s < a.streams; s++)
      if (fr[s]) {
        download(s);
        recs[(size_t)s * a.num_frames + fp[s].frame_num] = rec;
      }
  }
  for (int s = 0; s < a.streams; s++)
    if (fr[s])
      for (int n = 0; n < a.num_frames; n++) {
        const std::vector<uint8_t>& r = recs[(size_t)s * a.num_frames + n];
        if (!r.empty()) fwrite(r.data(), 1, rsz, fr[s]);
      }
  for (int s = 0; s < a.streams; s++) {
    if (fr[s]) fclose(fr[s]);
    if (!a.outfile.empty()) {
      FILE* fo = fopen(name(a.outfile, s).c_str(), "wb");
      fwrite(eng.st[s].out.data(), 1, eng.st[s].out.size(), fo);
      fclose(fo);
    }
  }
  if (const char* rlp = getenv("THOR_RC_LOG")) {   // tests: the controller's log, one line per coded frame of every rate-controlled stream
    FILE* fl = fopen(rlp, "w");
    if (!fl) { fprintf(stderr, "cannot open %s\n", rlp); return 5; }
    for (int s = 0; s < a.streams; s++)
      for (size_t i = 0; i < eng.st[s].rclog.size(); i++) {
        const RcStat& r = eng.st[s].rclog[i];
        const FrameStat& f = eng.st[s].log[i];
        fprintf(fl, "%d %d %d %d %d %d %d %d %llu %llu %llu %lld %d\n", s, f.display, f.frame_type, r.frame_class, r.qp_rule, r.base_qp, f.qp, f.num_bits, r.sum_intra, r.sum_best, r.n_intra,
                r.fullness, r.overflows);
      }
    fclose(fl);
  }
  if (const char* klp = getenv("THOR_KEY_LOG")) {   // tests: one line per coded frame of every stream: stream, display, type, reason, the analysis sums
    FILE* fl = fopen(klp, "w");
    if (!fl) { fprintf(stderr, "cannot open %s\n", klp); return 5; }
    for (int s = 0; s < a.streams; s++)
      for (const FrameStat& f : eng.st[s].log) fprintf(fl, "%d %d %d %d %llu %llu %llu\n", s, f.display, f.frame_type, f.key_reason, f.key_sums[0], f.key_sums[1], f.key_sums[2]);
    fclose(fl);
  }
  for (int s = 0; s < a.streams; s++) {
    if (a.streams > 1) printf("stream %d\n", s);
    fputs(format_report(eng.st[s].log, eng.st[s].sh_bits, p.max_num_ref, p.frame_rate, p.width, p.height, p.input_bitdepth).c_str(), stdout);
    if (!a.statfile.empty())
      append_stat_file(a.statfile.c_str(), format_stat_line(eng.st[s].log, eng.st[s].sh_bits, p.frame_rate, p.width, p.height, p.input_bitdepth, a.num_frames));
  }
  fflush(stdout);
  for (auto& b : tfbuf) b.release();
  eng.close();
  fclose(fi);
  return 0;
}

}  // namespace tk
