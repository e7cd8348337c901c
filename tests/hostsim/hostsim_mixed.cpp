// hostsim_mixed.cpp - TEST INFRASTRUCTURE ONLY.
// The host simulation of hostsim.cpp (the same translation unit, its main() renamed) behind a main() that lets input at a lower bit depth than
// the engine's through: -bitdepth 10 / 12 with -input_bitdepth 8, or 12 with 10.  The files it reads and writes hold input-depth samples, the
// report's PSNRs are on the input-depth scale (tk_cli.h: cli_run).  input_bitdepth above bitdepth exits 2, as every front end does.
#define main hostsim_equal_depth_main
#include "hostsim.cpp"
#undef main

int main(int argc, char** argv) {
  tk::init_tables(&tk::g_tab);
  tk::CliArgs a = tk::cli_parse(argc, argv);
  auto depth_ok = [](int d) { return d == 8 || d == 10 || d == 12; };
  if (!depth_ok(a.sp.bitdepth) || !depth_ok(a.sp.input_bitdepth) || a.sp.input_bitdepth > a.sp.bitdepth) {
    fprintf(stderr, "need bitdepth and input_bitdepth in {8, 10, 12} with input_bitdepth <= bitdepth\n");
    return 2;
  }
  return a.sp.bitdepth > 8 ? tk::cli_run<uint16_t>(a) : tk::cli_run<uint8_t>(a);
}
