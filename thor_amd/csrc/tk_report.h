// tk_report.h - the per-frame log of a stream and the encoder report printed from it.
// Specification followed: enc/mainenc.c:219-226 (the "SH:" line), :553-591 (one line per coded frame: PSNR of snr_yuv,
// the reference list as coded and the frame numbers of the references), :642-666 (average block and the -stat line),
// common/snr.c:32-99 (PSNR from the sums of squared differences).  Host code only.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace tk {

struct FrameStat {
  int display = 0;                 // absolute input frame index (what the reference prints)
  int frame_type = 0, qp = 0;      // F_I / F_P / F_B
  int num_bits = 0;                // bits of the frame before the 4-byte framing (sequence header excluded)
  int num_ref = 0;
  int ref_array[6] = {0, 0, 0, 0, 0, 0};      // window indices as coded (-1: interpolated frame, built from the next two)
  int ref_frame_num[6] = {0, 0, 0, 0, 0, 0};  // chunk-relative frame_num of the window frame ref_array[i] points at
  int has_sse = 0;                 // sse measured (frame distortion on)
  unsigned long long sse[3] = {0, 0, 0};       // Y, U, V: sum over the plane of (original - final reconstruction)^2
  int key_reason = 0;              // KEY_* (tk_rc.h): 0 the schedule's own type, 1 a forced key frame, 2 a scene cut
  unsigned long long key_sums[3] = {0, 0, 0};  // sum_intra, sum_best, n_intra of the frame's analysis; zero when it was not analysed
};

// snr_yuv (common/snr.c:56-62): plse = sse / (maxsignal * maxsignal * ydim * xdim) in double, in that order; the Y loop's float cast
// of each square is exact (4095^2 < 2^24) and so is the double sum of integers below 2^53: the exact sum gives the same double.
// sse == 0 gives inf, as the reference prints it.  `bitdepth`, here and below, is the INPUT bit depth: snr_yuv takes maxsignal from it and, when the
// encoder works at a higher depth, rounds both frames back to it before it subtracts them (common/snr.c:39-61; the engine's sums are formed that way).
inline double psnr_of(unsigned long long sse, int bitdepth, unsigned int xdim, unsigned int ydim) {
  const double maxsignal = (double)((1 << bitdepth) - 1);
  const double plse = (double)sse / (maxsignal * maxsignal * ydim * xdim);
  return -10 * log10(plse);
}

inline void frame_psnr(const FrameStat& f, int width, int height, int bitdepth, double out[3]) {
  if (!f.has_sse) { out[0] = out[1] = out[2] = 0.0; return; }  // -snrcalc 0 (mainenc.c:559-561)
  out[0] = psnr_of(f.sse[0], bitdepth, (unsigned)width, (unsigned)height);
  out[1] = psnr_of(f.sse[1], bitdepth, (unsigned)width >> 1, (unsigned)height >> 1);
  out[2] = psnr_of(f.sse[2], bitdepth, (unsigned)width >> 1, (unsigned)height >> 1);
}

inline void report_printf(std::string& s, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  const int n = vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (n > 0) s.append(buf, (size_t)n < sizeof buf ? (size_t)n : sizeof buf - 1);
}

struct ReportTotals { double kbps = 0, psnr[3] = {0, 0, 0}; int frames = 0; };

// Averages of mainenc.c:642-647: acc_num_bits (uint32_t) holds the sequence header bits too; PSNRs are summed in coding order.
inline ReportTotals report_totals(const std::vector<FrameStat>& log, int sh_bits, float frame_rate, int width, int height, int bitdepth) {
  ReportTotals t;
  uint32_t acc_bits = (uint32_t)sh_bits;
  double acc[3] = {0, 0, 0};
  for (const FrameStat& f : log) {
    double p[3];
    frame_psnr(f, width, height, bitdepth, p);
    for (int k = 0; k < 3; k++) acc[k] += p[k];
    acc_bits += (uint32_t)f.num_bits;
  }
  t.frames = (int)log.size();
  t.kbps = 0.001 * frame_rate * (double)acc_bits / t.frames;
  for (int k = 0; k < 3; k++) t.psnr[k] = acc[k] / t.frames;
  return t;
}

// The reference's stdout for one stream, byte for byte: SH line, one line per coded frame (in coding order), average block.
inline std::string format_report(const std::vector<FrameStat>& log, int sh_bits, int max_num_ref, float frame_rate, int width, int height,
                                 int bitdepth) {
  std::string s;
  report_printf(s, "SH:  %4d bits\n", sh_bits);
  for (const FrameStat& f : log) {
    double p[3];
    frame_psnr(f, width, height, bitdepth, p);
    const char t = f.frame_type == 0 ? 'I' : f.frame_type == 1 ? 'P' : 'B';
    report_printf(s, "%4d %c %4d %10d %10.4f %8.4f %8.4f ", f.display, t, f.qp, f.num_bits, p[0], p[1], p[2]);
    for (int r = 0; r < f.num_ref; r++) {
      if (f.ref_array[r] == -1) report_printf(s, "I(%d,%d) ", f.ref_array[r + 1], f.ref_array[r + 2]);
      else report_printf(s, "%3d", f.ref_array[r]);
    }
    for (int r = f.num_ref; r < max_num_ref; r++) s += "   ";
    s += " | ";
    for (int r = 0; r < f.num_ref; r++) {
      if (f.ref_array[r] == -1) report_printf(s, "I(%d,%d)", f.ref_frame_num[r + 1], f.ref_frame_num[r + 2]);
      else report_printf(s, "%3d", f.ref_frame_num[r]);
    }
    s += "\n";
  }
  const ReportTotals t = report_totals(log, sh_bits, frame_rate, width, height, bitdepth);
  s += "------------------- Average data for all frames ------------------------------\n";
  report_printf(s, "kbps            : %12.3f\n", t.kbps);
  report_printf(s, "PSNR Y          : %12.3f\n", t.psnr[0]);
  report_printf(s, "PSNR U          : %12.3f\n", t.psnr[1]);
  report_printf(s, "PSNR V          : %12.3f\n", t.psnr[2]);
  s += "------------------------------------------------------------------------------\n";
  return s;
}

// -stat FILE (mainenc.c:652-667): the header line when the file is new, then one line per run.  num_frames: the -n value.
static const char kStatHeader[] = " NFR     kbps     PSNRY  PSNRU  PSNRV\n";
inline std::string format_stat_line(const std::vector<FrameStat>& log, int sh_bits, float frame_rate, int width, int height, int bitdepth,
                                    int num_frames) {
  const ReportTotals t = report_totals(log, sh_bits, frame_rate, width, height, bitdepth);
  std::string s;
  report_printf(s, "%4d %12.3f %6.3f %6.3f %6.3f\n", num_frames, t.kbps, t.psnr[0], t.psnr[1], t.psnr[2]);
  return s;
}

// Appends `line` to the -stat file, preceded by the header if the file does not exist yet.
inline void append_stat_file(const char* path, const std::string& line) {
  FILE* f = fopen(path, "r");
  const bool not_exists = !f;
  if (f) fclose(f);
  if ((f = fopen(path, "a")) != nullptr) {
    if (not_exists) fputs(kStatHeader, f);
    fputs(line.c_str(), f);
    fclose(f);
  }
}

}  // namespace tk
