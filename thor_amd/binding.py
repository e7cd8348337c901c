"""ctypes binding of libthor_hip.so (include/thor_hip.h)."""
import ctypes as C
import os
import subprocess
import numpy as np

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib_path():
    """In-tree library; THOR_HIP_LIB selects another build of it (A/B measurements of kernel variants)."""
    return os.environ.get('THOR_HIP_LIB') or os.path.join(REPO_ROOT, 'thor_amd', 'libthor_hip.so')


HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fno-strict-aliasing', '-fPIC', '-pthread']
NATIVE_SOURCES = ['thor_hip.cpp', 'thor_hip_lat.cpp', 'thor_hip_wide.cpp', 'thor_hip_katbits.cpp']   # the throughput build of the engine (with its hip_*.h parts) + its two builds for the few-stream operating points + the known-answer kernels of the block syntax


def build_native(force=False):
    """Compile libthor_hip.so (gfx950) and the C front end in-tree with hipcc/gcc: the translation units are compiled side by side, then linked."""
    csrc = os.path.join(REPO_ROOT, 'thor_amd', 'csrc')
    out = os.path.join(REPO_ROOT, 'thor_amd', 'libthor_hip.so')
    hdrs = [os.path.join(csrc, f) for f in os.listdir(csrc)]
    hdrs += [os.path.join(REPO_ROOT, 'include', f) for f in os.listdir(os.path.join(REPO_ROOT, 'include'))]
    newest = max(os.path.getmtime(h) for h in hdrs)
    if force or not os.path.exists(out) or os.path.getmtime(out) < newest:
        hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else 'hipcc'
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            objs = [os.path.join(d, f[:-4] + '.o') for f in NATIVE_SOURCES]
            procs = [subprocess.Popen([hipcc] + HIPCC_FLAGS + ['-c', '-o', o, os.path.join(csrc, f)]) for f, o in zip(NATIVE_SOURCES, objs)]
            rcs = [p.wait() for p in procs]
            if any(rcs):
                raise subprocess.CalledProcessError(max(rcs), 'hipcc -c ' + ' '.join(NATIVE_SOURCES))
            subprocess.check_call([hipcc, '--offload-arch=gfx950', '-shared', '-pthread', '-o', out] + objs)
    tool = os.path.join(REPO_ROOT, 'tools', 'thorenc_hip')
    tsrc = tool + '.c'
    if force or not os.path.exists(tool) or os.path.getmtime(tool) < os.path.getmtime(tsrc):
        subprocess.check_call(['gcc', '-O2', '-std=c99', '-D_POSIX_C_SOURCE=200809L', '-o', tool, tsrc,
                               '-L' + os.path.join(REPO_ROOT, 'thor_amd'), '-lthor_hip', '-Wl,-rpath,$ORIGIN/../thor_amd'])
    return out


class ThorParams(C.Structure):
    """thor_hip_params (include/thor_hip.h) == the enc_params fields this path honours."""
    _fields_ = [('width', C.c_int), ('height', C.c_int), ('qp', C.c_int), ('bitdepth', C.c_int), ('input_bitdepth', C.c_int),
                ('frame_rate', C.c_float), ('lambda_coeffI', C.c_float), ('lambda_coeffP', C.c_float),
                ('early_skip_thr', C.c_float), ('enable_tb_split', C.c_int), ('enable_pb_split', C.c_int),
                ('max_num_ref', C.c_int), ('HQperiod', C.c_int), ('num_reorder_pics', C.c_int), ('interp_ref', C.c_int),
                ('dqpP', C.c_int), ('dqpI', C.c_int), ('mqpP', C.c_float), ('intra_period', C.c_int), ('intra_rdo', C.c_int),
                ('encoder_speed', C.c_int), ('deblocking', C.c_int), ('cdef', C.c_int), ('clpf', C.c_int),
                ('use_block_contexts', C.c_int), ('enable_bipred', C.c_int), ('cfl_intra', C.c_int), ('cfl_inter', C.c_int),
                ('dyadic_coding', C.c_int), ('lambda_coeffB', C.c_float), ('lambda_coeffB0', C.c_float), ('lambda_coeffB1', C.c_float),
                ('lambda_coeffB2', C.c_float), ('lambda_coeffB3', C.c_float), ('dqpB', C.c_int), ('dqpB0', C.c_int), ('dqpB1', C.c_int),
                ('dqpB2', C.c_int), ('dqpB3', C.c_int), ('mqpB', C.c_float), ('mqpB0', C.c_float), ('mqpB1', C.c_float),
                ('mqpB2', C.c_float), ('mqpB3', C.c_float), ('max_clpf_strength', C.c_int), ('log2_sb_size', C.c_int)]


FRAMES_DONE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int)   # thor_hip_frames_done_fn


class FrameStats(C.Structure):
    """thor_hip_frame_stats (include/thor_hip.h): one coded frame of a stream's log."""
    _fields_ = [('display_index', C.c_int), ('frame_type', C.c_int), ('qp', C.c_int), ('num_bits', C.c_int), ('num_ref', C.c_int),
                ('ref_array', C.c_int * 4), ('ref_frame_num', C.c_int * 4), ('has_sse', C.c_int), ('sse', C.c_ulonglong * 3),
                ('psnr', C.c_double * 3)]


CHROMA_PLANAR, CHROMA_UV, CHROMA_VU = 0, 1, 2   # THOR_HIP_CHROMA_*


class FrameLayout(C.Structure):
    """thor_hip_frame_layout (include/thor_hip.h): where the samples of a 4:2:0 frame lie in a buffer.  Pitches and offsets in bytes, 0 = tight /
    adjacent.  Samples are input_bitdepth wide (one byte for 8 bits, two otherwise); msb_aligned: they sit in the high bits of 16-bit words."""
    _fields_ = [('size', C.c_int), ('chroma', C.c_int), ('msb_aligned', C.c_int), ('pitch_y', C.c_int), ('pitch_c', C.c_int),
                ('offset_u', C.c_size_t), ('offset_v', C.c_size_t)]

    def __init__(self, chroma=CHROMA_PLANAR, msb_aligned=0, pitch_y=0, pitch_c=0, offset_u=0, offset_v=0):
        super().__init__(C.sizeof(FrameLayout), chroma, msb_aligned, pitch_y, pitch_c, offset_u, offset_v)

    @classmethod
    def planar(cls, pitch_y=0, pitch_c=0, offset_u=0, offset_v=0, msb_aligned=0):
        """Y, U and V planes (I420; YV12 by giving offset_v below offset_u)."""
        return cls(CHROMA_PLANAR, msb_aligned, pitch_y, pitch_c, offset_u, offset_v)

    @classmethod
    def nv12(cls, pitch=None, offset_uv=0):
        """Luma plane, then one plane U0 V0 U1 V1 ...; `pitch`: bytes between the rows of both planes."""
        return cls(CHROMA_UV, 0, pitch or 0, pitch or 0, offset_uv)

    @classmethod
    def nv21(cls, pitch=None, offset_vu=0):
        """NV12 with V first in every pair."""
        return cls(CHROMA_VU, 0, pitch or 0, pitch or 0, offset_vu)

    @classmethod
    def p010(cls, pitch=None, offset_uv=0):
        """NV12 of 16-bit words with the sample in the high bits: P010, P012 or P016 for input_bitdepth 10, 12 (any depth above 8)."""
        return cls(CHROMA_UV, 1, pitch or 0, pitch or 0, offset_uv)


RGB_RGBA, RGB_BGRA, RGB_ARGB, RGB_ABGR, RGB_RGB, RGB_BGR, RGB_PLANAR = range(7)   # THOR_HIP_RGB_*
MATRIX_BT601, MATRIX_BT709, MATRIX_BT2020 = 0, 1, 2                                # THOR_HIP_MATRIX_*


class RgbFormat(C.Structure):
    """thor_hip_rgb_format (include/thor_hip.h): an RGB frame - channel order, bits per channel (8: bytes; 10 / 12 / 16: 16-bit words), conversion
    matrix, range, chroma siting, row pitch in bytes (0 = tight) and, for planar frames, the bytes between planes (0 = adjacent)."""
    _fields_ = [('size', C.c_int), ('order', C.c_int), ('depth', C.c_int), ('msb_aligned', C.c_int), ('matrix', C.c_int), ('full_range', C.c_int),
                ('chroma_site', C.c_int), ('pitch', C.c_int), ('plane_stride', C.c_size_t)]

    def __init__(self, order=RGB_RGBA, depth=8, msb_aligned=0, matrix=MATRIX_BT709, full_range=0, chroma_site=1, pitch=0, plane_stride=0):
        super().__init__(C.sizeof(RgbFormat), order, depth, msb_aligned, matrix, full_range, chroma_site, pitch, plane_stride)

    @classmethod
    def rgba(cls, depth=8, matrix=MATRIX_BT709, full_range=0, chroma_site=1, pitch=0, msb_aligned=0):
        return cls(RGB_RGBA, depth, msb_aligned, matrix, full_range, chroma_site, pitch)

    @classmethod
    def bgra(cls, depth=8, matrix=MATRIX_BT709, full_range=0, chroma_site=1, pitch=0, msb_aligned=0):
        return cls(RGB_BGRA, depth, msb_aligned, matrix, full_range, chroma_site, pitch)

    @classmethod
    def rgb24(cls, depth=8, matrix=MATRIX_BT709, full_range=0, chroma_site=1, pitch=0, msb_aligned=0):
        """Three samples per pixel, R first (of 16-bit words when depth is above 8)."""
        return cls(RGB_RGB, depth, msb_aligned, matrix, full_range, chroma_site, pitch)

    @classmethod
    def bgr24(cls, depth=8, matrix=MATRIX_BT709, full_range=0, chroma_site=1, pitch=0, msb_aligned=0):
        return cls(RGB_BGR, depth, msb_aligned, matrix, full_range, chroma_site, pitch)

    @classmethod
    def planar(cls, depth=8, matrix=MATRIX_BT709, full_range=0, chroma_site=1, pitch=0, msb_aligned=0, plane_stride=0):
        """Three planes R, G, B: a contiguous torch tensor of shape 3 x H x W."""
        return cls(RGB_PLANAR, depth, msb_aligned, matrix, full_range, chroma_site, pitch, plane_stride)


SCALE_BILINEAR, SCALE_BICUBIC = 0, 1   # THOR_HIP_SCALE_*


class Scale(C.Structure):
    """thor_hip_scale (include/thor_hip.h): the size of the frames handed over, the resampling filter and the horizontal position of the chroma
    samples (0 centre, 1 left).  Staging such a frame resamples it to the encoder's size on the device."""
    _fields_ = [('size', C.c_int), ('src_width', C.c_int), ('src_height', C.c_int), ('filter', C.c_int), ('chroma_site', C.c_int)]

    def __init__(self, src_width=0, src_height=0, filter=SCALE_BICUBIC, chroma_site=1):
        super().__init__(C.sizeof(Scale), src_width, src_height, filter, chroma_site)


class RateControl(C.Structure):
    """thor_hip_rate_control (include/thor_hip.h): a target bitrate in bits per second for one stream, the virtual buffer in milliseconds (0 = 1000),
    the base-QP ranges of inter and of I frames (0 / 0 = 0..51) and the base QP of a sequence's first frame (0 = the parameter set's qp)."""
    _fields_ = [('size', C.c_int), ('bitrate', C.c_int), ('buffer_ms', C.c_int), ('min_qp', C.c_int), ('max_qp', C.c_int), ('min_qp_i', C.c_int),
                ('max_qp_i', C.c_int), ('initial_qp', C.c_int)]

    def __init__(self, bitrate=0, buffer_ms=0, min_qp=0, max_qp=0, min_qp_i=0, max_qp_i=0, initial_qp=0):
        super().__init__(C.sizeof(RateControl), bitrate, buffer_ms, min_qp, max_qp, min_qp_i, max_qp_i, initial_qp)

    def ok(self):
        """thor_hip_rate_control_check: would thor_hip_set_rate_control accept it?  Needs no device."""
        return lib().thor_hip_rate_control_check(C.byref(self)) == 0


class FrameRc(C.Structure):
    """thor_hip_frame_rc (include/thor_hip.h): one coded frame of a rate-controlled stream."""
    _fields_ = [('base_qp', C.c_int), ('frame_class', C.c_int), ('sum_intra', C.c_ulonglong), ('sum_best', C.c_ulonglong), ('n_intra', C.c_ulonglong),
                ('fullness', C.c_longlong), ('buffer_bits', C.c_longlong), ('target_bits', C.c_longlong), ('overflows', C.c_int)]


class SceneCut(C.Structure):
    """thor_hip_scene_cut (include/thor_hip.h): a P frame whose sum_best reaches `percent` per cent of its sum_intra, at least max(1, min_interval) frames
    after the stream's last I frame, becomes a key frame.  percent has no default; 0 is off."""
    _fields_ = [('size', C.c_int), ('percent', C.c_int), ('min_interval', C.c_int)]

    def __init__(self, percent=0, min_interval=0):
        super().__init__(C.sizeof(SceneCut), percent, min_interval)

    def ok(self):
        """thor_hip_scene_cut_check: would thor_hip_set_scene_cut accept it?  Needs no device."""
        return lib().thor_hip_scene_cut_check(C.byref(self)) == 0


class FrameKey(C.Structure):
    """thor_hip_frame_key (include/thor_hip.h): why a coded frame is a key frame, and its analysis sums."""
    _fields_ = [('reason', C.c_int), ('sum_intra', C.c_ulonglong), ('sum_best', C.c_ulonglong), ('n_intra', C.c_ulonglong)]


class TemporalFilter(C.Structure):
    """thor_hip_temporal_filter (include/thor_hip.h): the strength, 1 .. 16, of the motion-compensated temporal noise filter of staged frames."""
    _fields_ = [('size', C.c_int), ('strength', C.c_int)]

    def __init__(self, strength=6):
        super().__init__(C.sizeof(TemporalFilter), strength)

    def ok(self):
        """thor_hip_temporal_filter_check: would thor_hip_filter_staged accept it?  Needs no device."""
        return lib().thor_hip_temporal_filter_check(C.byref(self)) == 0


class TfRequest(C.Structure):
    """thor_hip_tf_request (include/thor_hip.h): filter the staged frame `slot` of `stream` against the staged frames ref_slot (ref_dist 1 or 2 each) into dst_slot."""
    _fields_ = [('stream', C.c_int), ('dst_slot', C.c_int), ('slot', C.c_int), ('nrefs', C.c_int), ('ref_slot', C.c_int * 4), ('ref_dist', C.c_int * 4)]


def lib():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError(f'{p} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no CPU path')
        L = C.CDLL(p)
        L.thor_hip_open.restype = C.c_void_p
        L.thor_hip_open.argtypes = [C.POINTER(ThorParams), C.c_int, C.c_int]
        L.thor_hip_close.argtypes = [C.c_void_p]
        L.thor_hip_begin_sequence.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.thor_hip_next_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.thor_hip_stage_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_stage_frame_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_encode_staged.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.thor_hip_encode_frame.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.thor_hip_encode_staged_run.argtypes = [C.c_void_p, C.c_int, FRAMES_DONE_FN, C.c_void_p]
        L.thor_hip_last_display_index.argtypes = [C.c_void_p, C.c_int]
        L.thor_hip_stream_bytes.restype = C.c_size_t
        L.thor_hip_stream_bytes.argtypes = [C.c_void_p, C.c_int]
        L.thor_hip_stream_data.restype = C.c_void_p
        L.thor_hip_stream_data.argtypes = [C.c_void_p, C.c_int]
        L.thor_hip_get_recon.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.thor_hip_frame_bytes.restype = C.c_size_t
        L.thor_hip_frame_bytes.argtypes = [C.c_void_p]
        L.thor_hip_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double)]
        L.thor_hip_kernel_time_reset.argtypes = [C.c_void_p]
        L.thor_hip_read_stats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
        L.thor_hip_deblock_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_deblock_frame_hbd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_set_frame_distortion.argtypes = [C.c_void_p, C.c_int]
        L.thor_hip_frame_stats_count.argtypes = [C.c_void_p, C.c_int]
        L.thor_hip_get_frame_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(FrameStats)]
        L.thor_hip_report.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
        L.thor_hip_stat_line.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
        L.thor_hip_frame_sse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
        L.thor_hip_kat_depth_up.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_kat_depth_down.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_frame_sse_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
        LP = C.POINTER(FrameLayout)
        L.thor_hip_layout_bytes.restype = C.c_size_t
        L.thor_hip_layout_bytes.argtypes = [C.c_void_p, LP]
        L.thor_hip_layout_bytes_for.restype = C.c_size_t
        L.thor_hip_layout_bytes_for.argtypes = [C.c_int, C.c_int, C.c_int, LP]
        L.thor_hip_stage_frame_layout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, LP, C.c_int]
        L.thor_hip_get_recon_layout.argtypes = [C.c_void_p, C.c_int, C.c_void_p, LP, C.c_int]
        L.thor_hip_kat_layout_in.argtypes = [C.c_void_p, LP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_kat_layout_out.argtypes = [C.c_void_p, LP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        RP = C.POINTER(RgbFormat)
        L.thor_hip_rgb_bytes.restype = C.c_size_t
        L.thor_hip_rgb_bytes.argtypes = [C.c_void_p, RP]
        L.thor_hip_rgb_bytes_for.restype = C.c_size_t
        L.thor_hip_rgb_bytes_for.argtypes = [C.c_int, C.c_int, RP]
        L.thor_hip_stage_frame_rgb.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, RP, C.c_int]
        L.thor_hip_get_recon_rgb.argtypes = [C.c_void_p, C.c_int, C.c_void_p, RP, C.c_int]
        L.thor_hip_kat_rgb_in.argtypes = [C.c_void_p, RP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_kat_rgb_out.argtypes = [C.c_void_p, RP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        SP = C.POINTER(Scale)
        L.thor_hip_scale_bytes.restype = C.c_size_t
        L.thor_hip_scale_bytes.argtypes = [C.c_void_p, SP, LP]
        L.thor_hip_scale_bytes_for.restype = C.c_size_t
        L.thor_hip_scale_bytes_for.argtypes = [C.c_int, C.c_int, C.c_int, SP, LP]
        L.thor_hip_stage_frame_scaled.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, SP, LP, C.c_int]
        L.thor_hip_scale_taps.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_short), C.c_int]
        L.thor_hip_kat_scale_in.argtypes = [C.c_void_p, SP, LP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_rate_control_check.argtypes = [C.POINTER(RateControl)]
        L.thor_hip_set_rate_control.argtypes = [C.c_void_p, C.c_int, C.POINTER(RateControl)]
        L.thor_hip_get_frame_rc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(FrameRc)]
        L.thor_hip_kat_rc_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.c_void_p]
        L.thor_hip_kat_scene_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
        L.thor_hip_force_key_frame.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.thor_hip_scene_cut_check.argtypes = [C.POINTER(SceneCut)]
        L.thor_hip_set_scene_cut.argtypes = [C.c_void_p, C.c_int, C.POINTER(SceneCut)]
        L.thor_hip_scene_cost.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
        L.thor_hip_get_frame_key.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(FrameKey)]
        L.thor_hip_temporal_filter_check.argtypes = [C.POINTER(TemporalFilter)]
        L.thor_hip_filter_staged.argtypes = [C.c_void_p, C.POINTER(TfRequest), C.c_int, C.POINTER(TemporalFilter)]
        L.thor_hip_get_staged.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.thor_hip_kat_temporal_filter.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.thor_hip_params_from_config.argtypes = [C.POINTER(ThorParams), C.c_char_p]
        L.thor_hip_params_set.argtypes = [C.POINTER(ThorParams), C.c_char_p, C.c_char_p]
        L.thor_hip_params_set_sb_size.argtypes = [C.POINTER(ThorParams), C.c_int]
        _LIB = L
    return _LIB


def load_config(cfg_path=None, **overrides):
    """ThorParams from a Thorenc-style config file plus "-name value" overrides (width=..., qp=...)."""
    p = ThorParams()
    rc = lib().thor_hip_params_from_config(C.byref(p), cfg_path.encode() if cfg_path else None)
    if rc:
        raise ValueError(f'{cfg_path}: unknown or unsupported option (rc={rc}); this path rejects what it cannot encode bit-exactly')
    for k, v in overrides.items():
        if k == 'log2_sb_size':   # thor_hip_params_set passes only the default; the superblock size has its own call
            rc = lib().thor_hip_params_set_sb_size(C.byref(p), int(v))
        else:
            rc = lib().thor_hip_params_set(C.byref(p), ('-' + k).encode(), str(v).encode())
        if rc:
            raise ValueError(f'option -{k} {v}: ' + {1: 'unknown', 2: 'not implemented by this path', 3: 'front-end option, not an encoder parameter'}.get(rc, f'rc={rc}'))
    return p


class Encoder:
    """N independent closed streams encoded in lock step on one GPU (thor_hip_open ... thor_hip_close).  Frames go in (stage) and come out
    (recon) at the INPUT bit depth - `dtype` samples, `frame_bytes` bytes - also when params.bitdepth is higher (bitdepth=10, input_bitdepth=8)."""

    def __init__(self, params, num_streams=1, device=0):
        self.p = params
        self.S = num_streams
        self.h = lib().thor_hip_open(C.byref(params), num_streams, device)
        if not self.h:
            raise RuntimeError('thor_hip_open failed (unsupported parameters?)')
        self.dtype = _pix(params.input_bitdepth)
        self.sample_bytes = self.dtype().itemsize
        self.frame_bytes = lib().thor_hip_frame_bytes(self.h)

    def close(self):
        if self.h:
            lib().thor_hip_close(self.h)
            self.h = None

    def layout_bytes(self, layout):
        """Bytes a frame in `layout` (a FrameLayout) spans; raises for a layout the library refuses."""
        n = lib().thor_hip_layout_bytes(self.h, C.byref(layout))
        if not n:
            raise ValueError('frame layout refused (pitch below the row, pitch or offset no multiple of the sample size, msb_aligned with 8-bit input ...)')
        return n

    def stage(self, stream, slot, frame, layout=None):
        """Stage a host frame: packed planar 4:2:0 of input-depth samples, or, with a FrameLayout, layout_bytes(layout) bytes in that layout."""
        frame = np.ascontiguousarray(frame).view(np.uint8)
        if layout is not None:
            assert frame.size >= self.layout_bytes(layout)
            rc = lib().thor_hip_stage_frame_layout(self.h, stream, slot, frame.ctypes.data_as(C.c_void_p), C.byref(layout), 0)
            if rc:
                raise RuntimeError(f'thor_hip_stage_frame_layout rc={rc}')
            return
        assert frame.size == self.frame_bytes
        rc = lib().thor_hip_stage_frame(self.h, stream, slot, frame.ctypes.data_as(C.c_void_p))
        if rc:
            raise RuntimeError(f'thor_hip_stage_frame rc={rc}')

    def stage_device(self, stream, slot, dev_ptr, layout=None):
        """Stage a frame that already lives in HBM (device pointer to a contiguous planar 4:2:0 frame of input-depth samples; 16-byte aligned
        when input_bitdepth < bitdepth).  With a FrameLayout: device pointer to a frame in that layout (NV12, P010, a row pitch ...), read by
        the kernel that writes the slot; sample-aligned is enough."""
        if layout is not None:
            rc = lib().thor_hip_stage_frame_layout(self.h, stream, slot, C.c_void_p(dev_ptr), C.byref(layout), 1)
            if rc:
                raise RuntimeError(f'thor_hip_stage_frame_layout rc={rc}')
            return
        rc = lib().thor_hip_stage_frame_device(self.h, stream, slot, C.c_void_p(dev_ptr))
        if rc:
            raise RuntimeError(f'thor_hip_stage_frame_device rc={rc}')

    def rgb_bytes(self, fmt):
        """Bytes an RGB frame in `fmt` (an RgbFormat) spans; raises for a format the library refuses."""
        n = lib().thor_hip_rgb_bytes(self.h, C.byref(fmt))
        if not n:
            raise ValueError('RGB format refused (unknown order / depth / matrix, msb_aligned with depth 8 or 16, pitch below the row ...)')
        return n

    def stage_rgb(self, stream, slot, array, fmt):
        """Stage a host RGB frame (rgb_bytes(fmt) bytes in `fmt`): converted to 4:2:0 at input_bitdepth on the device, then staged."""
        frame = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert frame.size >= self.rgb_bytes(fmt)
        rc = lib().thor_hip_stage_frame_rgb(self.h, stream, slot, frame.ctypes.data_as(C.c_void_p), C.byref(fmt), 0)
        if rc:
            raise RuntimeError(f'thor_hip_stage_frame_rgb rc={rc}')

    def stage_rgb_device(self, stream, slot, dev_ptr, fmt):
        """Stage an RGB frame that lives in HBM (e.g. tensor.data_ptr()), read in place by the kernel that writes the slot."""
        rc = lib().thor_hip_stage_frame_rgb(self.h, stream, slot, C.c_void_p(dev_ptr), C.byref(fmt), 1)
        if rc:
            raise RuntimeError(f'thor_hip_stage_frame_rgb rc={rc}')

    def recon_rgb(self, stream, fmt):
        """Reconstruction of the stream's last coded frame as RGB: rgb_bytes(fmt) bytes (row padding and gaps between planes are zero)."""
        out = np.zeros(self.rgb_bytes(fmt), dtype=np.uint8)
        rc = lib().thor_hip_get_recon_rgb(self.h, stream, out.ctypes.data_as(C.c_void_p), C.byref(fmt), 0)
        if rc:
            raise RuntimeError(f'thor_hip_get_recon_rgb rc={rc}')
        return out

    def recon_rgb_device(self, stream, dev_ptr, fmt):
        """The same into device memory (rgb_bytes(fmt) bytes at dev_ptr); only the picture's samples are written.  Synchronous at return."""
        rc = lib().thor_hip_get_recon_rgb(self.h, stream, C.c_void_p(dev_ptr), C.byref(fmt), 1)
        if rc:
            raise RuntimeError(f'thor_hip_get_recon_rgb rc={rc}')

    def scale_bytes(self, scale, layout=None):
        """Bytes a source frame of `scale` (a Scale) spans in `layout` (a FrameLayout at the source size; None: packed planar); raises if refused."""
        n = lib().thor_hip_scale_bytes(self.h, C.byref(scale), C.byref(layout) if layout is not None else None)
        if not n:
            raise ValueError('scaled staging refused (odd or out-of-range source size, ratio above 8, unknown filter or site, layout refused at the source size)')
        return n

    def stage_scaled(self, stream, slot, array, scale, layout=None):
        """Stage a host frame of another size (scale_bytes(scale, layout) bytes): resampled to the encoder's size on the device, then staged."""
        frame = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert frame.size >= self.scale_bytes(scale, layout)
        rc = lib().thor_hip_stage_frame_scaled(self.h, stream, slot, frame.ctypes.data_as(C.c_void_p), C.byref(scale), C.byref(layout) if layout is not None else None, 0)
        if rc:
            raise RuntimeError(f'thor_hip_stage_frame_scaled rc={rc}')

    def stage_scaled_device(self, stream, slot, dev_ptr, scale, layout=None):
        """The same for a frame that lives in HBM (e.g. tensor.data_ptr()), read in place by the kernel that writes the slot."""
        rc = lib().thor_hip_stage_frame_scaled(self.h, stream, slot, C.c_void_p(dev_ptr), C.byref(scale), C.byref(layout) if layout is not None else None, 1)
        if rc:
            raise RuntimeError(f'thor_hip_stage_frame_scaled rc={rc}')

    def begin_sequence(self, stream, skip, num_frames, file_frames):
        """Fix the chunk [skip, skip+num_frames) of a file_frames-long input (thor_hip_begin_sequence)."""
        rc = lib().thor_hip_begin_sequence(self.h, stream, skip, num_frames, file_frames)
        if rc:
            raise RuntimeError(f'thor_hip_begin_sequence rc={rc}')

    def next_frame(self, stream):
        """Chunk-relative display index of the next frame to code, or None when the chunk is finished."""
        d = C.c_int()
        return d.value if lib().thor_hip_next_frame(self.h, stream, C.byref(d)) else None

    def encode_run(self, nframes, on_done=None):
        """thor_hip_encode_staged_run: the next nframes frames of every stream (inputs staged at their display index), the streams in two
        groups half a frame apart.  on_done(first_stream, num_streams) is called when the frames of those streams are complete (recon(s) and
        last_display_index(s) describe that frame inside the callback)."""
        err = []

        def _cb(_user, first, count):
            if on_done is not None and not err:
                try:
                    on_done(first, count)
                except BaseException as e:   # an exception must not unwind through the C frames
                    err.append(e)
        cb = FRAMES_DONE_FN(_cb)
        rc = lib().thor_hip_encode_staged_run(self.h, nframes, cb, None)
        if err:
            raise err[0]
        if rc:
            raise RuntimeError(f'thor_hip_encode_staged_run rc={rc}')

    def last_display_index(self, stream):
        return lib().thor_hip_last_display_index(self.h, stream)

    def encode_clips(self, clips, want_recon=True, skips=None, file_frames=None, staggered=False):
        """Encode clips[s] (equal-length lists of frames in display order) as closed streams in lock step - or, staggered=True, in two groups
        half a frame apart (encode_run) - following the coding-order schedule.  Stream s stands for frames [skips[s], skips[s]+n) of an input
        file holding file_frames frames (defaults: 0 and n).  Returns (bitstreams, recon[s][display index])."""
        n = len(clips[0])
        for s in range(self.S):
            for f in range(n):
                self.stage(s, f, clips[s][f])
            sk = skips[s] if skips else 0
            self.begin_sequence(s, sk, n, file_frames if file_frames else sk + n)
        recs = [[None] * n for _ in range(self.S)]
        if staggered:
            def done(first, count):
                if want_recon:
                    for s in range(first, first + count):
                        recs[s][self.last_display_index(s)] = self.recon(s)
            self.encode_run(n, done)
            return [self.bitstream(s) for s in range(self.S)], recs
        while True:
            idx = [self.next_frame(s) for s in range(self.S)]
            if idx[0] is None:
                break
            self.encode_staged(idx)
            if want_recon:
                for s in range(self.S):
                    recs[s][idx[s]] = self.recon(s)
        return [self.bitstream(s) for s in range(self.S)], recs

    def encode_staged(self, slots):
        arr = (C.c_int * self.S)(*slots)
        rc = lib().thor_hip_encode_staged(self.h, arr)
        if rc:
            raise RuntimeError(f'thor_hip_encode_staged rc={rc}')

    def bitstream(self, stream):
        n = lib().thor_hip_stream_bytes(self.h, stream)
        return C.string_at(lib().thor_hip_stream_data(self.h, stream), n)

    def recon(self, stream, layout=None):
        """Reconstruction of the stream's last coded frame: frame_bytes bytes (view them as self.dtype for the samples); with a FrameLayout,
        layout_bytes(layout) bytes in that layout (row padding and gaps between planes are zero)."""
        if layout is not None:
            out = np.zeros(self.layout_bytes(layout), dtype=np.uint8)
            rc = lib().thor_hip_get_recon_layout(self.h, stream, out.ctypes.data_as(C.c_void_p), C.byref(layout), 0)
            if rc:
                raise RuntimeError(f'thor_hip_get_recon_layout rc={rc}')
            return out
        out = np.empty(self.frame_bytes, dtype=np.uint8)
        rc = lib().thor_hip_get_recon(self.h, stream, out.ctypes.data_as(C.c_void_p))
        if rc:
            raise RuntimeError(f'thor_hip_get_recon rc={rc}')
        return out

    def recon_device(self, stream, dev_ptr, layout):
        """Reconstruction of the stream's last coded frame into device memory (layout_bytes(layout) bytes at dev_ptr) in `layout`; only the
        picture's samples are written.  Synchronous at return."""
        rc = lib().thor_hip_get_recon_layout(self.h, stream, C.c_void_p(dev_ptr), C.byref(layout), 1)
        if rc:
            raise RuntimeError(f'thor_hip_get_recon_layout rc={rc}')

    def recon_into(self, stream, ptr):
        """Reconstruction of the stream's last frame into a caller-owned host buffer of frame_bytes bytes (e.g. pinned memory that is reused)."""
        rc = lib().thor_hip_get_recon(self.h, stream, C.c_void_p(ptr))
        if rc:
            raise RuntimeError(f'thor_hip_get_recon rc={rc}')

    def kernel_time(self):
        a, b, c = C.c_double(), C.c_long(), C.c_double()
        lib().thor_hip_kernel_time(self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def kernel_time_reset(self):
        lib().thor_hip_kernel_time_reset(self.h)
        self.stats(reset=True)

    def stats(self, reset=False):
        """Early-skip statistics of the inter frames coded since the last reset (thor_hip_read_stats)."""
        a = (C.c_ulonglong * 4)()
        lib().thor_hip_read_stats(self.h, a, 1 if reset else 0)
        px, sb = max(int(a[3]), 1), max(int(a[2]), 1)
        return {'early_skip_pixel_fraction': round(int(a[0]) / px, 4), 'early_skip_sb128_fraction': round(int(a[1]) / sb, 4),
                'inter_superblocks': int(a[2]), 'inter_luma_pixels': int(a[3])}

    def set_frame_distortion(self, on=True):
        """Measure the per-plane SSE of every coded frame on the GPU (thor_hip_set_frame_distortion; off by default)."""
        lib().thor_hip_set_frame_distortion(self.h, 1 if on else 0)

    def frame_stats(self, stream):
        """The stream's log of coded frames in coding order (thor_hip_get_frame_stats): a list of dicts."""
        L, out, f = lib(), [], FrameStats()
        for i in range(L.thor_hip_frame_stats_count(self.h, stream)):
            if L.thor_hip_get_frame_stats(self.h, stream, i, C.byref(f)):
                raise RuntimeError('thor_hip_get_frame_stats failed')
            nr = f.num_ref
            out.append({'display_index': f.display_index, 'type': 'IPB'[f.frame_type], 'qp': f.qp, 'num_bits': f.num_bits,
                        'ref_array': list(f.ref_array)[:nr], 'ref_frame_num': list(f.ref_frame_num)[:nr], 'has_sse': bool(f.has_sse),
                        'sse': [int(v) for v in f.sse], 'psnr': [float(v) for v in f.psnr]})
        return out

    def set_rate_control(self, stream, rc):
        """Rate control of one stream (a RateControl; None or bitrate 0: off): thor_hip_set_rate_control.  Legal before the stream's first frame and
        right after begin_sequence; raises ValueError when the library refuses."""
        r = lib().thor_hip_set_rate_control(self.h, stream, C.byref(rc) if rc is not None else None)
        if r:
            raise ValueError('rate control refused: ' + ('the stream is in the middle of a sequence' if r == 2 else 'bad stream or values'))

    def frame_rc(self, stream):
        """The controller's log of a rate-controlled stream in coding order (thor_hip_get_frame_rc), index for index with frame_stats: a list of
        dicts; empty for a stream without rate control."""
        L, out, f = lib(), [], FrameRc()
        for i in range(L.thor_hip_frame_stats_count(self.h, stream)):
            if L.thor_hip_get_frame_rc(self.h, stream, i, C.byref(f)):
                break
            out.append({'base_qp': f.base_qp, 'frame_class': f.frame_class, 'sum_intra': int(f.sum_intra), 'sum_best': int(f.sum_best),
                        'n_intra': int(f.n_intra), 'fullness': int(f.fullness), 'buffer_bits': int(f.buffer_bits), 'target_bits': int(f.target_bits),
                        'overflows': f.overflows})
        return out

    def force_key_frame(self, stream, index):
        """A key frame at chunk-relative frame `index` of a low-delay stream (thor_hip_force_key_frame); raises ValueError when the library refuses."""
        r = lib().thor_hip_force_key_frame(self.h, stream, index)
        if r:
            raise ValueError('key frame refused: ' + ('the parameter set is not low delay' if r == 2 else 'bad stream, a frame already coded or too many requests'))

    def set_scene_cut(self, stream, sc):
        """Scene cuts of one stream (a SceneCut; None or percent 0: off): thor_hip_set_scene_cut.  Legal where set_rate_control is."""
        r = lib().thor_hip_set_scene_cut(self.h, stream, C.byref(sc) if sc is not None else None)
        if r:
            raise ValueError('scene cut refused: ' + ('the stream is in the middle of a sequence or not low delay' if r == 2 else 'bad stream or values'))

    def frame_key(self, stream):
        """Per coded frame, index for index with frame_stats: dict(reason, sum_intra, sum_best, n_intra) (thor_hip_get_frame_key)."""
        L, out, f = lib(), [], FrameKey()
        for i in range(L.thor_hip_frame_stats_count(self.h, stream)):
            if L.thor_hip_get_frame_key(self.h, stream, i, C.byref(f)):
                break
            out.append({'reason': f.reason, 'sum_intra': int(f.sum_intra), 'sum_best': int(f.sum_best), 'n_intra': int(f.n_intra)})
        return out

    def scene_cost(self, stream, slot, prev_slot=-1):
        """[sum_intra, sum_best, n_intra] of the staged frame `slot` against the staged frame prev_slot (-1: none): thor_hip_scene_cost."""
        sums = (C.c_ulonglong * 3)()
        r = lib().thor_hip_scene_cost(self.h, stream, slot, prev_slot, sums)
        if r:
            raise ValueError('scene cost refused: ' + ('the parameter set is not low delay' if r == 2 else 'bad stream or a slot that is not staged'))
        return [int(v) for v in sums]

    def filter_staged(self, requests, tf):
        """thor_hip_filter_staged: `requests` is a list of (stream, dst_slot, slot, [(ref_slot, ref_dist), ...]) with up to four neighbours each, all filtered in
        one call with the TemporalFilter `tf`.  Raises ValueError when the library refuses the call (nothing is written then)."""
        arr = (TfRequest * max(1, len(requests)))()
        for r, (stream, dst_slot, slot, refs) in zip(arr, requests):
            r.stream, r.dst_slot, r.slot, r.nrefs = stream, dst_slot, slot, len(refs)
            for k, (ref_slot, ref_dist) in enumerate(refs[:4]):
                r.ref_slot[k], r.ref_dist[k] = ref_slot, ref_dist
        if lib().thor_hip_filter_staged(self.h, arr, len(requests), C.byref(tf) if tf is not None else None):
            raise ValueError('temporal filter refused: a bad request or strength, a slot that is not staged, or a destination that is a source or is given twice')

    def staged(self, stream, slot):
        """The staged frame in `slot` as it would be coded (thor_hip_get_staged): a flat packed planar 4:2:0 array at the engine's depth."""
        out = np.zeros(self.p.width * self.p.height * 3 // 2, dtype=_pix(self.p.bitdepth))
        if lib().thor_hip_get_staged(self.h, stream, slot, _vp(out)):
            raise ValueError('bad stream or a slot that is not staged')
        return out

    def report(self, stream):
        """The reference encoder's stdout report for the stream so far (thor_hip_report)."""
        n = lib().thor_hip_report(self.h, stream, None, 0)
        if n < 0:
            raise ValueError('bad stream')
        buf = C.create_string_buffer(n + 1)
        lib().thor_hip_report(self.h, stream, buf, n + 1)
        return buf.value.decode()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _pix(bitdepth):
    return np.uint16 if bitdepth > 8 else np.uint8


def sad_batch(org, ref_plane, bx, by, cand, bitdepth=8):
    """SADs of the candidates (thor_hip_sad_batch; bitdepth > 8: thor_hip_sad_batch_hbd on uint16 samples)."""
    T = _pix(bitdepth)
    org = np.ascontiguousarray(org, dtype=T); ref_plane = np.ascontiguousarray(ref_plane, dtype=T)
    cand = np.ascontiguousarray(cand, dtype=np.int32)
    out = np.zeros(len(cand), dtype=np.uint32)
    fn = lib().thor_hip_sad_batch_hbd if bitdepth > 8 else lib().thor_hip_sad_batch
    rc = fn(_vp(org), org.shape[1], org.shape[0], _vp(ref_plane), ref_plane.shape[1], ref_plane.shape[0], ref_plane.shape[1], bx, by,
            _vp(cand), len(cand), _vp(out))
    if rc:
        raise RuntimeError(f'thor_hip_sad_batch rc={rc}')
    return out


def interp_luma(ref_padded, pad, pic_w, pic_h, bx, by, w, h, mvs, bipred, bitdepth=8):
    T = _pix(bitdepth)
    ref_padded = np.ascontiguousarray(ref_padded, dtype=T); mvs = np.ascontiguousarray(mvs, dtype=np.int16)
    out = np.zeros((len(mvs), h, w), dtype=T)
    if bitdepth > 8:
        rc = lib().thor_hip_interp_luma_hbd(_vp(ref_padded), pic_w, pic_h, ref_padded.shape[1], pad, bx, by, w, h, _vp(mvs), len(mvs),
                                            bipred, bitdepth, _vp(out))
    else:
        rc = lib().thor_hip_interp_luma(_vp(ref_padded), pic_w, pic_h, ref_padded.shape[1], pad, bx, by, w, h, _vp(mvs), len(mvs),
                                        bipred, _vp(out))
    if rc:
        raise RuntimeError(f'thor_hip_interp_luma rc={rc}')
    return out


def code_tu_batch(org, pred, qp, coeff_type, fast, bitdepth=8):
    T = _pix(bitdepth)
    org = np.ascontiguousarray(org, dtype=T); pred = np.ascontiguousarray(pred, dtype=T)
    n, size = org.shape[0], org.shape[1]
    q = min(size, 16)
    coefq = np.zeros((n, q, q), dtype=np.int16); rec = np.zeros_like(org); cbp = np.zeros(n, dtype=np.int32)
    if bitdepth > 8:
        rc = lib().thor_hip_code_tu_batch_hbd(_vp(org), _vp(pred), size, qp, coeff_type, fast, n, bitdepth, _vp(coefq), _vp(rec), _vp(cbp))
    else:
        rc = lib().thor_hip_code_tu_batch(_vp(org), _vp(pred), size, qp, coeff_type, fast, n, _vp(coefq), _vp(rec), _vp(cbp))
    if rc:
        raise RuntimeError(f'thor_hip_code_tu_batch rc={rc}')
    return coefq, rec, cbp


def deblock_frame(yuv, width, height, qp, cells, bitdepth=8):
    """In-loop deblocking of one planar 4:2:0 frame (thor_hip_deblock_frame / _hbd); cells: (h/4, w/4, 16) uint8 records."""
    yuv = np.ascontiguousarray(yuv, dtype=_pix(bitdepth)).copy()
    cells = np.ascontiguousarray(cells, dtype=np.uint8)
    assert yuv.size == width * height * 3 // 2 and cells.size == (width // 4) * (height // 4) * 16
    if bitdepth > 8:
        rc = lib().thor_hip_deblock_frame_hbd(_vp(yuv), width, height, qp, bitdepth, _vp(cells))
    else:
        rc = lib().thor_hip_deblock_frame(_vp(yuv), width, height, qp, _vp(cells))
    if rc:
        raise RuntimeError(f'thor_hip_deblock_frame rc={rc}')
    return yuv


# ---- round 6: known-answer entry points (include/thor_hip.h, section 3b) ----------------------------------------------------------
def _kat(name, *args):
    fn = getattr(lib(), name)
    fn.restype = C.c_int
    rc = fn(*args)
    if rc:
        raise RuntimeError(f'{name} rc={rc}')


def kat_intra(plane, size, par, bitdepth=8, rblocks=None):
    """Intra prediction of len(par) transform units (thor_hip_kat_intra); par rows: ypos, xpos, upright, downleft, mode, i, j."""
    T = _pix(bitdepth)
    plane = np.ascontiguousarray(plane, dtype=T); par = np.ascontiguousarray(par, dtype=np.int32)
    n = len(par)
    out = np.zeros((n, size, size), dtype=T)
    rb = np.ascontiguousarray(rblocks, dtype=T) if rblocks is not None else None
    _kat('thor_hip_kat_intra', _vp(plane), plane.shape[1], plane.shape[0], plane.shape[1], bitdepth, size, 1 if rb is not None else 0, n, _vp(par),
         _vp(rb) if rb is not None else None, _vp(out))
    return out


def kat_inter_yuv(yuv, width, height, size, par, mvs, bitdepth=8):
    """thor_hip_kat_inter_yuv: par rows ypos, xpos, sign, enable_bipred, split; mvs [n][4][2]."""
    T = _pix(bitdepth)
    yuv = np.ascontiguousarray(yuv, dtype=T); par = np.ascontiguousarray(par, dtype=np.int32); mvs = np.ascontiguousarray(mvs, dtype=np.int16)
    n = len(par)
    out = np.zeros((n, size * size * 3 // 2), dtype=T)
    _kat('thor_hip_kat_inter_yuv', _vp(yuv), width, height, bitdepth, size, n, _vp(par), _vp(mvs), _vp(out))
    return out


def kat_average(a, b, size, bitdepth=8):
    T = _pix(bitdepth)
    a = np.ascontiguousarray(a, dtype=T); b = np.ascontiguousarray(b, dtype=T)
    out = np.zeros_like(a)
    _kat('thor_hip_kat_average', _vp(a), _vp(b), size, bitdepth, len(a), _vp(out))
    return out


def kat_cfl(y, uv, ry, n_luma, bitdepth=8):
    T = _pix(bitdepth)
    y = np.ascontiguousarray(y, dtype=T); ry = np.ascontiguousarray(ry, dtype=T); uv = np.array(uv, dtype=T, order='C')
    _kat('thor_hip_kat_cfl', _vp(y), _vp(uv), _vp(ry), n_luma, bitdepth, len(y))
    return uv


def kat_cdef_dir(blocks, bitdepth=8):
    T = _pix(bitdepth)
    blocks = np.ascontiguousarray(blocks, dtype=T)
    n = len(blocks)
    d = np.zeros(n, dtype=np.int32); v = np.zeros(n, dtype=np.int32)
    _kat('thor_hip_kat_cdef_dir', _vp(blocks), bitdepth, n, _vp(d), _vp(v))
    return d, v


def kat_cdef_filter(plane, bsize, par, bitdepth=8):
    T = _pix(bitdepth)
    plane = np.ascontiguousarray(plane, dtype=T); par = np.ascontiguousarray(par, dtype=np.int32)
    out = np.zeros((len(par), bsize, bsize), dtype=T)
    _kat('thor_hip_kat_cdef_filter', _vp(plane), plane.shape[1], plane.shape[0], plane.shape[1], bitdepth, bsize, len(par), _vp(par), _vp(out))
    return out


def kat_cdef_frame(rec, org, mode, width, height, qp, speed, cdef_bits, bitdepth=8):
    """thor_hip_kat_cdef_frame: rec / org (S, width * height * 3 / 2) packed planar frames, mode (S, height / 4, width / 4) bytes, qp / speed / cdef_bits (S,).  Returns a dict of per-job arrays:
    dir, var (S, h/8, w/8), fb_compact, fb_sel (S, nfb), mse (S, 2, nfb, 64), nb_bits, sb_count (S,), strengths, uv_strengths (S, 8), out (S, frame)."""
    T = _pix(bitdepth)
    rec = np.ascontiguousarray(rec, dtype=T); org = np.ascontiguousarray(org, dtype=T); mode = np.ascontiguousarray(mode, dtype=np.uint8)
    S = len(rec)
    nfb = ((width + 63) // 64) * ((height + 63) // 64)
    qp, speed, cdef_bits = (np.ascontiguousarray(a, dtype=np.int32) for a in (qp, speed, cdef_bits))
    assert rec.shape == org.shape == (S, width * height * 3 // 2) and mode.shape == (S, height // 4, width // 4) and len(qp) == len(speed) == len(cdef_bits) == S
    d = np.zeros((S, height // 8, width // 8), dtype=np.int8); v = np.zeros((S, height // 8, width // 8), dtype=np.int32)
    fbc = np.zeros((S, nfb), dtype=np.int32); fbs = np.zeros((S, nfb), dtype=np.int32)
    mse = np.zeros((S, 2, nfb, 64), dtype=np.uint64); res = np.zeros((S, 34), dtype=np.int32)
    out = np.zeros_like(rec)
    _kat('thor_hip_kat_cdef_frame', S, _vp(rec), _vp(org), _vp(mode), width, height, bitdepth, _vp(qp), _vp(speed), _vp(cdef_bits), _vp(d), _vp(v), _vp(fbc), _vp(mse), _vp(res), _vp(fbs),
         _vp(out))
    return dict(dir=d, var=v, fb_compact=fbc, fb_sel=fbs, mse=mse, nb_bits=res[:, 0], strengths=res[:, 1:9], uv_strengths=res[:, 9:17], sb_count=res[:, 17], out=out)


def kat_clpf(rec, org, width, height, qp, cells, strength, fb_log2, fb_on, bitdepth=8):
    T = _pix(bitdepth)
    rec = np.ascontiguousarray(rec, dtype=T); org = np.ascontiguousarray(org, dtype=T)
    cells = np.ascontiguousarray(cells, dtype=np.uint8); fb_on = np.ascontiguousarray(fb_on, dtype=np.uint8)
    st = np.ascontiguousarray(strength, dtype=np.int32)
    nblk = (width // 8) * (height // 8) + 2 * (width // 16) * (height // 16)
    stats = np.zeros((nblk, 4), dtype=np.uint32)
    out = np.zeros_like(rec)
    _kat('thor_hip_kat_clpf', _vp(rec), _vp(org), width, height, bitdepth, qp, _vp(cells), _vp(st), fb_log2, _vp(fb_on), _vp(stats), _vp(out))
    return stats, out


def kat_interpolate(yuv0, yuv1, width, height, bitdepth=8):
    T = _pix(bitdepth)
    a = np.ascontiguousarray(yuv0, dtype=T); b = np.ascontiguousarray(yuv1, dtype=T)
    out = np.zeros_like(a)
    _kat('thor_hip_kat_interpolate', _vp(a), _vp(b), width, height, bitdepth, _vp(out))
    return out


def kat_interp_stages(yuv0, yuv1, width, height, bitdepth=8):
    """thor_hip_kat_interp_stages: yuv0 / yuv1 (S, width * height * 3 / 2) packed planar frames, one reference pair per stream, all through one
    make_interp_frames call.  Returns the raw buffers, one row per stream: pyramid planes with padding, nmv[0] / nmv[1] of every level, the padded output
    (layout: include/thor_hip.h)."""
    import math
    T = _pix(bitdepth)
    a = np.ascontiguousarray(yuv0, dtype=T); b = np.ascontiguousarray(yuv1, dtype=T)
    S = len(a)
    assert a.shape == b.shape == (S, width * height * 3 // 2)
    levels = min(4, int(math.log10(min(width, height)) / math.log10(2.0) - 4.0))
    pyr = np.zeros((S, 2 * sum(((height >> l) + 64) * ((width >> l) + 64) for l in range(1, levels))), dtype=T)
    nmv = np.zeros((S, sum(16 * (((width >> l) + 15) // 16) * (((height >> l) + 15) // 16) for l in range(levels))), dtype=np.int16)
    out = np.zeros((S, (height + 320) * (width + 320) + 2 * (height // 2 + 160) * (width // 2 + 160)), dtype=T)
    _kat('thor_hip_kat_interp_stages', S, _vp(a), _vp(b), width, height, bitdepth, levels, _vp(pyr), _vp(nmv), _vp(out))
    return pyr, nmv, out


def kat_motion_estimate(cur, ref, par, lam, cand, bitdepth=8):
    """thor_hip_kat_motion_estimate: the device motion search on len(par) items of one current / reference luma pair; returns (n, 3) mv.x, mv.y, cost."""
    T = _pix(bitdepth)
    cur = np.ascontiguousarray(cur, dtype=T); ref = np.ascontiguousarray(ref, dtype=T)
    par = np.ascontiguousarray(par, dtype=np.int32); lam = np.ascontiguousarray(lam, dtype=np.float64); cand = np.ascontiguousarray(cand, dtype=np.int16).reshape(-1, 2)
    assert cur.shape == ref.shape and par.shape[1] == 17 and len(lam) == len(par)
    out = np.full((len(par), 3), -1, dtype=np.int32)
    _kat('thor_hip_kat_motion_estimate', _vp(cur), _vp(ref), cur.shape[1], cur.shape[0], bitdepth, len(par), _vp(par), _vp(lam), _vp(cand), len(cand), _vp(out))
    return out


def kat_motion_estimate_bi(cur, ref0, ref1, par, lam, cand, bitdepth=8):
    """thor_hip_kat_motion_estimate_bi; cand: (n, 6, 2) list slots.  Returns ((n, 3) mv.x, mv.y, cost, (n, 6, 2) the list afterwards)."""
    T = _pix(bitdepth)
    cur, ref0, ref1 = (np.ascontiguousarray(a, dtype=T) for a in (cur, ref0, ref1))
    par = np.ascontiguousarray(par, dtype=np.int32); lam = np.ascontiguousarray(lam, dtype=np.float64); cand = np.ascontiguousarray(cand, dtype=np.int16)
    assert cur.shape == ref0.shape == ref1.shape and par.shape[1] == 17 and len(lam) == len(par) and cand.size == 12 * len(par)
    out = np.full((len(par), 3), -1, dtype=np.int32)
    lists = np.zeros((len(par), 6, 2), dtype=np.int16)
    _kat('thor_hip_kat_motion_estimate_bi', _vp(cur), _vp(ref0), _vp(ref1), cur.shape[1], cur.shape[0], bitdepth, len(par), _vp(par), _vp(lam), _vp(cand), _vp(out), _vp(lists))
    return out, lists


def kat_early_skip(chroma, org, pred, size, qp, thr, bitdepth=8):
    """thor_hip_kat_early_skip: org / pred (n, 32, 32) blocks; chroma / size / qp / thr per item.  Returns the n decisions (1 = significant)."""
    T = _pix(bitdepth)
    org = np.ascontiguousarray(org, dtype=T); pred = np.ascontiguousarray(pred, dtype=T)
    chroma, size, qp = (np.ascontiguousarray(a, dtype=np.int32) for a in (chroma, size, qp))
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    n = len(org)
    assert org.shape == pred.shape == (n, 32, 32) and len(chroma) == len(size) == len(qp) == len(thr) == n
    out = np.full(n, -1, dtype=np.int32)
    _kat('thor_hip_kat_early_skip', _vp(chroma), _vp(org), _vp(pred), _vp(size), _vp(qp), _vp(thr), bitdepth, n, _vp(out))
    return out


def kat_block_ctx(cells, cell_stride, par):
    """thor_hip_kat_block_ctx: cells (ncells, 16) bytes = thor_hip_cell records in raster order; par (n, 6) ypos, xpos, size, frame width, frame height,
    superblock size.  Returns (n, 23): get_mv_pred, the candidates of get_mv_cands, the contexts with enable 0 / 1, the two availability flags."""
    cells = np.ascontiguousarray(cells, dtype=np.uint8); par = np.ascontiguousarray(par, dtype=np.int32)
    assert cells.ndim == 2 and cells.shape[1] == 16 and par.ndim == 2 and par.shape[1] == 6
    out = np.full((len(par), 23), -77, dtype=np.int32)
    _kat('thor_hip_kat_block_ctx', _vp(cells), C.c_longlong(len(cells)), cell_stride, len(par), _vp(par), _vp(out))
    return out


def kat_lds_block():
    """thor_hip_kat_lds_block: the largest coding-block size the build keeps in LDS."""
    fn = lib().thor_hip_kat_lds_block
    fn.restype = C.c_int
    return fn()


def kat_block_cost(par, lam, org, rec, bitdepth=8):
    """thor_hip_kat_block_cost: par (n, 7) size, bw, bh, nbits, off, skew, stride; lam (n,); org / rec: sample pools holding the compact 4:2:0 blocks at `off`.
    Returns (n, 4) uint64: luma SSD (global-memory instance), luma SSD (LDS instance, all ones for blocks the engine keeps in global memory), rd_cost,
    rd_cost with the luma SSD passed in."""
    T = _pix(bitdepth)
    org = np.ascontiguousarray(org, dtype=T).ravel(); rec = np.ascontiguousarray(rec, dtype=T).ravel()
    par = np.ascontiguousarray(par, dtype=np.int32); lam = np.ascontiguousarray(lam, dtype=np.float64)
    assert par.ndim == 2 and par.shape[1] == 7 and len(lam) == len(par) and len(org) == len(rec)
    out = np.zeros((len(par), 4), dtype=np.uint64)
    _kat('thor_hip_kat_block_cost', len(par), _vp(par), _vp(lam), _vp(org), _vp(rec), C.c_longlong(len(org)), bitdepth, _vp(out))
    return out


def kat_intra_search(par, plane, org, bitdepth=8):
    """thor_hip_kat_intra_search: par (n, 6) ypos, xpos, size, superblock size, num_intra_modes, off; plane (height, width) reconstructed luma; org: pool of
    compact original blocks.  Returns (n, 2): intra mode, SAD."""
    T = _pix(bitdepth)
    plane = np.ascontiguousarray(plane, dtype=T); org = np.ascontiguousarray(org, dtype=T).ravel()
    par = np.ascontiguousarray(par, dtype=np.int32)
    assert plane.ndim == 2 and par.ndim == 2 and par.shape[1] == 6
    out = np.full((len(par), 2), -77, dtype=np.int32)
    _kat('thor_hip_kat_intra_search', len(par), _vp(par), _vp(plane), plane.shape[1], plane.shape[0], _vp(org), C.c_longlong(len(org)), bitdepth, _vp(out))
    return out


def kat_build_org8(par, org, pred, bitdepth=8, fill=0):
    """thor_hip_kat_build_org8: par (n, 4) size, off, skew, stride; org / pred: sample pools.  Returns (out_global, out_lds): pools pre-filled with `fill` holding
    each item's result at `off` (out_lds only for blocks the engine keeps in LDS)."""
    T = _pix(bitdepth)
    org = np.ascontiguousarray(org, dtype=T).ravel(); pred = np.ascontiguousarray(pred, dtype=T).ravel()
    par = np.ascontiguousarray(par, dtype=np.int32)
    assert par.ndim == 2 and par.shape[1] == 4 and len(org) == len(pred)
    og = np.full(len(org), fill, dtype=T); ol = np.full(len(org), fill, dtype=T)
    _kat('thor_hip_kat_build_org8', len(par), _vp(par), _vp(org), _vp(pred), C.c_longlong(len(org)), bitdepth, _vp(og), _vp(ol))
    return og, ol


def kat_coeff_syntax(par, coef, words, buf_single, buf_team):
    """thor_hip_kat_coeff_syntax: par (n, 4) size, type, start bit, capacity; coef (n, 256); buf_* (n, words) uint32, pre-filled.  Returns (out (n, 6),
    buf_single, buf_team) - the buffers as the device left them."""
    par = np.ascontiguousarray(par, dtype=np.int32); coef = np.ascontiguousarray(coef, dtype=np.int16)
    n = len(par)
    b1 = np.ascontiguousarray(buf_single, dtype=np.uint32).copy(); bt = np.ascontiguousarray(buf_team, dtype=np.uint32).copy()
    assert par.shape == (n, 4) and coef.shape == (n, 256) and b1.shape == (n, words) and bt.shape == (n, words)
    out = np.zeros((n, 6), dtype=np.int32)
    _kat('thor_hip_kat_coeff_syntax', n, _vp(par), _vp(coef), words, _vp(b1), _vp(bt), _vp(out))
    return out, b1, bt


def kat_block_syntax(par, pool, words, fill=0):
    """thor_hip_kat_block_syntax: par (n, 57) rows (thor_amd/csrc/tk_kat_bits.h), pool (npool, 256) coefficients.  Returns (out (n, 10), buf_coop, buf_single),
    the buffers (n, words) uint32 pre-filled with `fill`."""
    par = np.ascontiguousarray(par, dtype=np.int32); pool = np.ascontiguousarray(pool, dtype=np.int16)
    n = len(par)
    assert par.shape == (n, 57) and pool.ndim == 2 and pool.shape[1] == 256
    bc = np.full((n, words), fill, dtype=np.uint32); b1 = np.full((n, words), fill, dtype=np.uint32)
    out = np.zeros((n, 10), dtype=np.int32)
    _kat('thor_hip_kat_block_syntax', n, _vp(par), _vp(pool), len(pool), words, _vp(bc), _vp(b1), _vp(out))
    return out, bc, b1


def kat_gather_bits(src, src_off, nbits, dst_bit, dst_words):
    """thor_hip_kat_gather_bits: strings of nbits[i] bits at word src_off[i] of `src` to bit dst_bit[i] of a zeroed destination; returns it (uint32)."""
    src = np.ascontiguousarray(src, dtype=np.uint32); src_off = np.ascontiguousarray(src_off, dtype=np.int32)
    nbits = np.ascontiguousarray(nbits, dtype=np.int32); dst_bit = np.ascontiguousarray(dst_bit, dtype=np.int64)
    dst = np.zeros(dst_words, dtype=np.uint32)
    _kat('thor_hip_kat_gather_bits', len(nbits), _vp(src), len(src), _vp(src_off), _vp(nbits), _vp(dst_bit), _vp(dst), dst_words)
    return dst


def frame_sse(a, b, width, height, bitdepth=8):
    """Per-plane (Y, U, V) sums of squared differences of two planar 4:2:0 frames on the GPU (thor_hip_frame_sse, kernel k_frame_sse)."""
    T = _pix(bitdepth)
    a = np.ascontiguousarray(a, dtype=T).reshape(-1); b = np.ascontiguousarray(b, dtype=T).reshape(-1)
    if a.size != width * height * 3 // 2 or b.size != a.size:
        raise ValueError('frame size does not match width x height 4:2:0')
    out = (C.c_ulonglong * 3)()
    rc = lib().thor_hip_frame_sse(_vp(a), _vp(b), width, height, bitdepth, out)
    if rc:
        raise RuntimeError(f'thor_hip_frame_sse returned {rc}')
    return [int(v) for v in out]


def _depth_frame(a, depth, width, height):
    a = np.ascontiguousarray(a, dtype=_pix(depth)).reshape(-1)
    if a.size != width * height * 3 // 2:
        raise ValueError('frame size does not match width x height 4:2:0')
    return a


def kat_depth_up(frame, width, height, bitdepth, input_bitdepth):
    """thor_hip_kat_depth_up: a planar 4:2:0 frame of input-depth samples widened to `bitdepth` by the kernel that stages frames (uint16)."""
    a = _depth_frame(frame, input_bitdepth, width, height)
    out = np.zeros(a.size, dtype=np.uint16)
    _kat('thor_hip_kat_depth_up', _vp(a), width, height, bitdepth, input_bitdepth, _vp(out))
    return out


def kat_depth_down(frame, width, height, bitdepth, input_bitdepth):
    """thor_hip_kat_depth_down: a uint16 frame at `bitdepth` rounded and saturated to the input depth by the kernel behind Encoder.recon."""
    a = _depth_frame(frame, 16, width, height)
    out = np.zeros(a.size, dtype=_pix(input_bitdepth))
    _kat('thor_hip_kat_depth_down', _vp(a), width, height, bitdepth, input_bitdepth, _vp(out))
    return out


def frame_sse_depth(a, b, width, height, bitdepth, input_bitdepth):
    """thor_hip_frame_sse_depth: per-plane (Y, U, V) sums of squared differences of two frames at `bitdepth`, measured at the input depth."""
    T = 16 if bitdepth > input_bitdepth else bitdepth
    a = _depth_frame(a, T, width, height); b = _depth_frame(b, T, width, height)
    out = (C.c_ulonglong * 3)()
    _kat('thor_hip_frame_sse_depth', _vp(a), _vp(b), width, height, bitdepth, input_bitdepth, out)
    return [int(v) for v in out]


def layout_bytes(layout, width, height, input_bitdepth):
    """thor_hip_layout_bytes_for: bytes a width x height frame in `layout` spans, 0 if the layout is refused.  Needs no encoder and no device."""
    return lib().thor_hip_layout_bytes_for(width, height, input_bitdepth, C.byref(layout))


def kat_layout_in(src, layout, width, height, input_bitdepth, bitdepth):
    """thor_hip_kat_layout_in: a frame in `layout` (a uint8 array of at least layout_bytes; its address decides the kernel's path) through
    k_layout_in -> packed planar 4:2:0 at `bitdepth`."""
    assert src.dtype == np.uint8 and src.flags.c_contiguous and src.size >= layout_bytes(layout, width, height, input_bitdepth) > 0
    out = np.zeros(width * height * 3 // 2, dtype=_pix(bitdepth))
    _kat('thor_hip_kat_layout_in', _vp(src), C.byref(layout), width, height, input_bitdepth, bitdepth, _vp(out))
    return out


def kat_layout_out(planar, layout, width, height, input_bitdepth, bitdepth, dst):
    """thor_hip_kat_layout_out: a packed planar 4:2:0 frame at `bitdepth` through k_layout_out into `dst`, in place: a uint8 array of layout_bytes
    + 64 guard bytes, all of which travel to the device and back."""
    a = _depth_frame(planar, bitdepth, width, height)
    assert dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.size == layout_bytes(layout, width, height, input_bitdepth) + 64 > 64
    _kat('thor_hip_kat_layout_out', _vp(a), C.byref(layout), width, height, input_bitdepth, bitdepth, _vp(dst))
    return dst


def rgb_bytes(fmt, width, height):
    """thor_hip_rgb_bytes_for: bytes a width x height RGB frame in `fmt` spans, 0 if the format is refused.  Needs no encoder and no device."""
    return lib().thor_hip_rgb_bytes_for(width, height, C.byref(fmt))


def kat_rgb_in(src, fmt, width, height, input_bitdepth, bitdepth):
    """thor_hip_kat_rgb_in: an RGB frame (a uint8 array of at least rgb_bytes; its address decides the kernel's path) through k_rgb_in -> packed
    planar 4:2:0 at `bitdepth`."""
    assert src.dtype == np.uint8 and src.flags.c_contiguous and src.size >= rgb_bytes(fmt, width, height) > 0
    out = np.zeros(width * height * 3 // 2, dtype=_pix(bitdepth))
    _kat('thor_hip_kat_rgb_in', _vp(src), C.byref(fmt), width, height, input_bitdepth, bitdepth, _vp(out))
    return out


def kat_rgb_out(planar, fmt, width, height, input_bitdepth, bitdepth, dst):
    """thor_hip_kat_rgb_out: a packed planar 4:2:0 frame at `bitdepth` through k_rgb_out into `dst`, in place: a uint8 array of rgb_bytes + 64 guard
    bytes, all of which travel to the device and back."""
    a = _depth_frame(planar, bitdepth, width, height)
    assert dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.size == rgb_bytes(fmt, width, height) + 64 > 64
    _kat('thor_hip_kat_rgb_out', _vp(a), C.byref(fmt), width, height, input_bitdepth, bitdepth, _vp(dst))
    return dst


def scale_bytes(scale, width, height, input_bitdepth=8, layout=None):
    """thor_hip_scale_bytes_for: bytes the source frame of `scale` spans when it feeds a width x height encoder, 0 if refused.  Needs no device."""
    return lib().thor_hip_scale_bytes_for(width, height, input_bitdepth, C.byref(scale), C.byref(layout) if layout is not None else None)


def scale_taps(S, T, filter, cosited, i):
    """thor_hip_scale_taps: (first source index, [coefficients]) of destination index i on an axis S -> T; None if refused.  Needs no device."""
    first, coef = C.c_int(0), (C.c_short * 33)()
    n = lib().thor_hip_scale_taps(S, T, filter, cosited, i, C.byref(first), coef, 33)
    return (first.value, list(coef[:n])) if n else None


def kat_scale_in(src, scale, width, height, input_bitdepth, bitdepth, layout=None):
    """thor_hip_kat_scale_in: a source frame (a uint8 array of at least scale_bytes; its address decides the kernel's path) through k_scale_in ->
    packed planar 4:2:0 of width x height at `bitdepth`."""
    assert src.dtype == np.uint8 and src.flags.c_contiguous and src.size >= scale_bytes(scale, width, height, input_bitdepth, layout) > 0
    out = np.zeros(width * height * 3 // 2, dtype=_pix(bitdepth))
    _kat('thor_hip_kat_scale_in', _vp(src), C.byref(scale), C.byref(layout) if layout is not None else None, width, height, input_bitdepth, bitdepth, _vp(out))
    return out


def kat_rc_cost(cur, prev, bitdepth):
    """thor_hip_kat_rc_cost: k_rc_cost on the luma plane `cur` (h x w) after `prev` (None: no previous frame), in the engine's launch sequence.
    Returns ([sum_intra, sum_best, n_intra], the half-size plane of cur)."""
    T = _pix(bitdepth)
    cur = np.ascontiguousarray(cur, dtype=T)
    h, w = cur.shape
    if prev is not None:
        prev = np.ascontiguousarray(prev, dtype=T)
        assert prev.shape == cur.shape
    sums = (C.c_ulonglong * 3)()
    half = np.zeros((h // 2, w // 2), dtype=T)
    _kat('thor_hip_kat_rc_cost', _vp(cur), _vp(prev) if prev is not None else None, w, h, bitdepth, sums, _vp(half))
    return [int(v) for v in sums], half


def kat_scene_cost(cur, prev, bitdepth):
    """thor_hip_kat_scene_cost: the instantiation of k_rc_cost behind thor_hip_scene_cost on the luma plane `cur` (h x w) against the ORIGINAL `prev`
    (None: no previous frame).  Returns [sum_intra, sum_best, n_intra]."""
    T = _pix(bitdepth)
    cur = np.ascontiguousarray(cur, dtype=T)
    h, w = cur.shape
    if prev is not None:
        prev = np.ascontiguousarray(prev, dtype=T)
        assert prev.shape == cur.shape
    sums = (C.c_ulonglong * 3)()
    _kat('thor_hip_kat_scene_cost', _vp(cur), _vp(prev) if prev is not None else None, w, h, bitdepth, sums)
    return [int(v) for v in sums]


def kat_temporal_filter(cur, refs, dists, depth, strength):
    """thor_hip_kat_temporal_filter: k_tf_search and k_tf_blend on the frame `cur` = (Y, U, V) against the frames `refs` (up to four such triples, dists 1 or 2
    each), as the engine launches them for one request.  Returns ((Y, U, V) filtered, mv int32 (nrefs, h / 8, w / 8, 2) as (dx, dy), wb int32 (nrefs, h / 8, w / 8))."""
    T = _pix(depth)
    h, w = cur[0].shape
    pack = lambda f: np.concatenate([np.ascontiguousarray(p, dtype=T).ravel() for p in f])
    c = pack(cur)
    r = np.concatenate([pack(f) for f in refs]) if len(refs) else np.zeros(1, dtype=T)
    d = (C.c_int * 4)(*list(dists))
    out = np.zeros(w * h * 3 // 2, dtype=T)
    mv = np.zeros((len(refs), h // 8, w // 8, 2), dtype=np.int32)
    wb = np.zeros((len(refs), h // 8, w // 8), dtype=np.int32)
    _kat('thor_hip_kat_temporal_filter', _vp(c), _vp(r), d, len(refs), w, h, depth, strength, _vp(out), _vp(mv), _vp(wb))
    ny, nc = w * h, (w // 2) * (h // 2)
    return (out[:ny].reshape(h, w), out[ny:ny + nc].reshape(h // 2, w // 2), out[ny + nc:].reshape(h // 2, w // 2)), mv, wb
