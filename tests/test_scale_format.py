"""Staging frames of another size, at the boundary (-m "not gpu"): thor_hip_scale_taps against the restatement of tests/scale_format.py for every
destination index of the size pairs that can go wrong; the host build of resolve_scale and of the pieces k_scale_in is made of
(tests/hostsim/unit_scale.cpp, one lane and 4 x 64 lanes) against the numpy model, exactly, over sizes x depths x layouts x contents; and the
argument checks, which answer without a device."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from util import ROOT
import frame_layout as fl
import scale_format as sf
from test_frame_layout import build_host_program

CFG = os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')
# down by 3; up from a length that is no multiple of 8; by 2; by 1.93; up by 1.31; the ratio limits both ways; a ratio a hair under 2; no change
PAIRS = [(48, 16), (34, 64), (400, 200), (232, 120), (208, 272), (128, 16), (16, 128), (1918, 960), (24, 24)]


# ---- the taps ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cosited', [0, 1], ids=['centre', 'cosited'])
@pytest.mark.parametrize('filt', [0, 1], ids=sf.FILTER_NAMES)
@pytest.mark.parametrize('S,T', PAIRS)
def test_taps_match_the_restatement(S, T, filt, cosited):
    import thor_amd
    for i in range(T):
        got = thor_amd.scale_taps(S, T, filt, cosited, i)
        want = sf.taps(S, T, filt, cosited, i)
        assert got == want, (i, got, want)
        first, c = got
        assert sum(c) == sf.ONE and len(c) <= 33 and sum(abs(x) for x in c) <= sf.MAX_ABS
        if S == T:   # nothing but the sample itself: a scaled call at the coded size is layout staging
            assert [(first + k, x) for k, x in enumerate(c) if x] == [(i, sf.ONE)]


def test_the_quoted_row():
    """48 -> 16, bicubic, centre-aligned, i = 0: the row include/thor_hip.h's rule gives by hand."""
    import thor_amd
    assert thor_amd.scale_taps(48, 16, sf.BICUBIC, 0, 0) == (-4, [-202, -405, 0, 1820, 4248, 5462, 4248, 1820, 0, -405, -202])
    assert thor_amd.scale_taps(24, 24, sf.BILINEAR, 0, 7) == (7, [sf.ONE])


def test_taps_refusals():
    import thor_amd
    T = thor_amd.scale_taps
    assert T(48, 16, 2, 0, 0) is None and T(48, 16, -1, 0, 0) is None and T(48, 16, 1, 2, 0) is None
    assert T(48, 16, 1, 0, 16) is None and T(48, 16, 1, 0, -1) is None
    assert T(129, 16, 1, 0, 0) is None and T(16, 129, 1, 0, 0) is None and T(8194, 4096, 1, 0, 0) is None and T(0, 16, 1, 0, 0) is None
    first, coef = C.c_int(0), (C.c_short * 33)()
    assert thor_amd.lib().thor_hip_scale_taps(48, 16, 1, 0, 0, C.byref(first), coef, 10) == 0      # 11 taps do not fit
    assert thor_amd.lib().thor_hip_scale_taps(48, 16, 1, 0, 0, C.byref(first), coef, 11) == 11


# ---- the passes on the host -----------------------------------------------------------------------------------------------------------------------

def run_unit(exe, g, skew, w, h, n, bd, filt, site, src, tmp_path):
    (tmp_path / 'in').write_bytes(src.tobytes())
    f = g.fields
    subprocess.run([exe, str(g.w), str(g.h), str(w), str(h), str(n), str(bd), str(filt), str(site), str(g.chroma), str(g.msb), str(f['pitch_y']),
                    str(f['pitch_c']), str(skew), str(tmp_path / 'in'), str(tmp_path / 'out')], check=True)
    return np.frombuffer((tmp_path / 'out').read_bytes(), dtype=np.uint16 if bd > 8 else np.uint8)


@pytest.mark.parametrize('bd,n', sf.DEPTHS)
@pytest.mark.parametrize('sw,sh,w,h', sf.SIZES)
def test_host_functions_match_the_model(sw, sh, w, h, bd, n, tmp_path):
    """Both filters and both sitings over every source layout and content: the planes equal the model's; one lane and 4 x 64 lanes agree (checked by
    the program); a constant frame stays that constant."""
    exe = build_host_program('unit_scale')
    for name, g, skew in sf.source_layouts(sw, sh, n):
        for kind in sf.CONTENTS:
            frame = sf.content(kind, sw, sh, n)
            src = fl.pack(frame, g)
            for filt, site in ((sf.BICUBIC, 1), (sf.BILINEAR, 0)) if kind != 'noise' or name != 'planar' else ((1, 1), (1, 0), (0, 1), (0, 0)):
                got = run_unit(exe, g, skew, w, h, n, bd, filt, site, src, tmp_path)
                want = sf.expect_in(src, g, w, h, filt, site, n, bd)
                assert got.dtype == want.dtype and np.array_equal(got, want), (name, kind, filt, site, np.flatnonzero(got != want)[:8])
                if kind == 'constant':
                    top = (1 << n) - 1
                    ny, nc = w * h, (w // 2) * (h // 2)
                    assert np.all(got[:ny] == (top * 3 // 5) << (bd - n)) and np.all(got[ny:ny + nc] == (top // 3) << (bd - n)) and np.all(got[ny + nc:] == top << (bd - n))


def test_model_clamps_are_exercised():
    """The alternating columns drive the horizontal intermediate below zero and above the maximum with bicubic, so both clamps of the vertical pass
    (and the signed intermediate) are on the path the comparisons above take."""
    y = sf.content('columns', 34, 18, 8)[:34 * 18].reshape(18, 34)
    inter = (sf._pass(y, 34, 64, sf.BICUBIC, 0, 1) + (1 << 11)) >> 12
    assert inter.min() < 0 and inter.max() > 255 * 4


# ---- argument checks, without a device -------------------------------------------------------------------------------------------------------------

def test_scale_structure_matches_the_header():
    import thor_amd
    T = thor_amd.Scale
    assert [f[0] for f in T._fields_] == ['size', 'src_width', 'src_height', 'filter', 'chroma_site']
    assert T().size == C.sizeof(T) == 20
    t = T(192, 128)
    assert (t.src_width, t.src_height, t.filter, t.chroma_site) == (192, 128, 1, 1)


def refused(w, h, n):
    """(why, Scale, FrameLayout or None) that a w x h engine of n-bit input refuses."""
    import thor_amd
    S, L = thor_amd.Scale, thor_amd.FrameLayout
    bad_size = S(192, 128)
    bad_size.size -= 4
    B = 2 if n > 8 else 1
    out = [('odd source width', S(191, 128), None), ('odd source height', S(192, 127), None), ('14 x 16', S(14, 16), None), ('16 x 14', S(16, 14), None),
           ('source above 8192', S(8194, 128), None), ('ratio above 8 across', S(w * 8 + 2, h), None), ('ratio above 8 down', S(w, h * 8 + 2), None),
           ('ratio above 8 up', S(16, h), None), ('unknown filter', S(192, 128, filter=2), None),
           ('unknown filter', S(192, 128, filter=-1), None), ('unknown site', S(192, 128, chroma_site=2), None), ('size', bad_size, None),
           ('pitch below the source row', S(192, 128), L(0, 0, 192 * B - B, 0)), ('chroma pitch below the source row', S(192, 128), L.nv12(pitch=192 * B - 2))]
    if n == 8:
        out.append(('msb_aligned with 8-bit input', S(192, 128), L(1, 1, 0, 0)))
    return out


@pytest.mark.parametrize('bd,n', [(8, 8), (10, 8), (12, 10)])
def test_refusals_answer_before_the_device_is_touched(bd, n):
    """scale_bytes is 0, the known-answer entry point - which validates with the function thor_hip_stage_frame_scaled uses and needs no encoder -
    returns 1, and so does the encoder call (a valid call goes on to the device: tests/test_gpu_scale.py)."""
    import thor_amd
    L = thor_amd.lib()
    w, h = 192, 136
    buf = fl.skewed(1 << 20, 0)
    planar = np.zeros(w * h * 3 // 2, dtype=np.uint16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for why, sc, lay in refused(w, h, n):
        lp = C.byref(lay) if lay is not None else None
        assert thor_amd.scale_bytes(sc, w, h, n, lay) == 0, why
        assert L.thor_hip_kat_scale_in(vp(buf), C.byref(sc), lp, w, h, n, bd, vp(planar)) == 1, why
        assert L.thor_hip_stage_frame_scaled(None, 0, 0, vp(buf), C.byref(sc), lp, 0) == 1
    ok = thor_amd.Scale(192, 128)
    assert thor_amd.scale_bytes(ok, w, h, n) == 192 * 128 * 3 // 2 * (2 if n > 8 else 1)
    assert thor_amd.scale_bytes(ok, w, h, n, thor_amd.FrameLayout.nv12(pitch=512)) == 512 * 128 + 512 * 64
    assert thor_amd.scale_bytes(ok, w + 4, h, n) == 0 and thor_amd.scale_bytes(ok, 8, 8, n) == 0 and L.thor_hip_scale_bytes(None, C.byref(ok), None) == 0
    assert L.thor_hip_kat_scale_in(vp(buf), None, None, w, h, n, bd, vp(planar)) == 1
    assert L.thor_hip_kat_scale_in(vp(buf), C.byref(ok), None, w, h, bd + 2, bd, vp(planar)) == 1   # input deeper than the engine
    if n > 8:
        assert L.thor_hip_kat_scale_in(vp(fl.skewed(1 << 20, 1)), C.byref(ok), None, w, h, n, bd, vp(planar)) == 1   # base not sample-aligned


def test_scale_options_are_front_end_options_at_the_parameter_door():
    import thor_amd
    p = thor_amd.load_config(CFG, width=96, height=64)
    before = bytes(p)
    S = thor_amd.lib().thor_hip_params_set
    assert S(C.byref(p), b'-src_width', b'192') == 3 and S(C.byref(p), b'-src_height', b'128') == 3
    assert S(C.byref(p), b'-scale_filter', b'bilinear') == 3 and S(C.byref(p), b'-scale_site', b'centre') == 3
    assert S(C.byref(p), b'-scale_filter', b'lanczos') == 2 and S(C.byref(p), b'-scale_site', b'top') == 2
    assert bytes(p) == before


@pytest.mark.parametrize('binary', ['hostsim_mixed', 'thorenc_hip'])
def test_command_line_refuses_scaling_an_rgb_source(binary):
    exe = build_host_program('hostsim_mixed') if binary == 'hostsim_mixed' else os.path.join(ROOT, 'tools', 'thorenc_hip')
    r = subprocess.run([exe, '-cf', CFG, '-if', os.devnull, '-width', '96', '-height', '64', '-qp', '32', '-n', '1', '-pixfmt', 'bgra', '-src_width', '192',
                        '-src_height', '128'], capture_output=True, text=True)
    assert r.returncode == 2 and 'src_width' in r.stderr, (r.returncode, r.stderr)
