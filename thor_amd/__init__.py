"""thor_amd - Python host mirror of libthor_hip.so (MI355X-native Thor per-block encode path).

PyTorch is not involved in the data path; this module is a thin ctypes binding of the C ABI
declared in include/thor_hip.h (sequence API + kernel-level entry points).  There is no CPU
fallback: importing works anywhere, but every call that computes requires the HIP library and a
gfx950 device and fails loudly otherwise.
"""
from .binding import (ThorParams, Encoder, FrameLayout, RgbFormat, Scale, RateControl, SceneCut, TemporalFilter, lib, lib_path, load_config, sad_batch, interp_luma, code_tu_batch, deblock_frame,
                      frame_sse, frame_sse_depth, kat_depth_up, kat_depth_down, layout_bytes, kat_layout_in,
                      kat_layout_out, rgb_bytes, kat_rgb_in, kat_rgb_out, scale_bytes, scale_taps, kat_scale_in, kat_rc_cost, kat_scene_cost, kat_temporal_filter, build_native, REPO_ROOT)

__all__ = ['ThorParams', 'Encoder', 'FrameLayout', 'RgbFormat', 'Scale', 'RateControl', 'SceneCut', 'TemporalFilter', 'lib', 'lib_path', 'load_config', 'sad_batch', 'interp_luma', 'code_tu_batch', 'deblock_frame',
           'frame_sse', 'frame_sse_depth', 'kat_depth_up', 'kat_depth_down', 'layout_bytes', 'kat_layout_in', 'kat_layout_out', 'rgb_bytes', 'kat_rgb_in', 'kat_rgb_out', 'scale_bytes', 'scale_taps', 'kat_scale_in', 'kat_rc_cost', 'kat_scene_cost', 'kat_temporal_filter',
           'build_native', 'REPO_ROOT']
