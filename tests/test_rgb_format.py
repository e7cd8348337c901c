"""RGB frames at the boundary (-m "not gpu"): the host build of resolve_rgb, rgb_in_rows and rgb_out_rows (tests/hostsim/unit_rgb.cpp, one lane and
64-lane teams) against the numpy model of tests/rgb_format.py, exactly, for every order x depth x input depth x siting on the shapes that can go
wrong; the anchor conditions of the arithmetic (greys, black, white, rows summing to zero); the bound of one code value against the textbook formula
in float64; and the argument checks, which answer without a device."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
from util import ROOT
import rgb_format as rf
from test_frame_layout import build_host_program

CFG = os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')
# (bitdepth, input_bitdepth): the 8-bit engine, a widened 8-bit input, 10- and 12-bit input
PAIRS = [(8, 8), (10, 8), (12, 10), (12, 12)]


def run_unit(exe, f, skew, n, bd, src, rec, before, tmp_path):
    (tmp_path / 'in').write_bytes(src.tobytes() + rec.tobytes() + before.tobytes())
    subprocess.run([exe, str(f.w), str(f.h), str(n), str(bd), str(f.order), str(f.depth), str(f.msb), str(f.matrix), str(f.full), str(f.site),
                    str(f.fields['pitch']), str(f.fields['plane_stride']), str(skew), str(tmp_path / 'in'), str(tmp_path / 'out')], check=True)
    out = (tmp_path / 'out').read_bytes()
    nb = f.w * f.h * 3 // 2 * rec.itemsize
    assert len(out) == nb + f.bytes + rf.GUARD
    return np.frombuffer(out[:nb], dtype=rec.dtype), np.frombuffer(out[nb:], dtype=np.uint8)


# ---- the row functions on the host --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('site', [0, 1], ids=['centre', 'left'])
@pytest.mark.parametrize('bd,n', PAIRS)
@pytest.mark.parametrize('depth,msb', rf.DEPTHS)
@pytest.mark.parametrize('order', range(7), ids=rf.ORDER_NAMES)
def test_row_functions_match_the_model(order, depth, msb, bd, n, site, tmp_path):
    """rgb_in_rows: the planes equal the model's.  rgb_out_rows: every sample of the picture equals the model's and every other byte - row padding,
    gaps between planes, the guard - is untouched.  Matrix and range rotate with the case so that all six occur for every order."""
    exe = build_host_program('unit_rgb')
    k = order + depth + n + site
    matrix, full = k % 3, (k // 3) % 2
    for shape in rf.shapes(order, depth):
        f, skew = rf.shaped(order, depth, msb, matrix, full, site, shape)
        src = rf.pack(*rf.random_rgb(f, 7 + k), f)
        rec = rf.random_rec(f.w, f.h, bd, 9 + k)
        before = np.full(f.bytes + rf.GUARD, rf.CANARY, dtype=np.uint8)
        want = rf.expect_out(rec, f, n, bd, before.copy())
        planes, dst = run_unit(exe, f, skew, n, bd, src, rec, before, tmp_path)
        assert np.array_equal(planes, rf.expect_in(src, f, n, bd)), (rf.format_id(f), shape)
        assert np.array_equal(dst, want), (rf.format_id(f), shape, np.flatnonzero(dst != want)[:8])


CONVERSIONS = [(m, full, depth, n) for m in range(3) for full in (0, 1) for depth in (8, 10, 12, 16) for n in (8, 10, 12)]


def coefficients_of(exe, f, n):
    out = subprocess.run([exe, 'coefficients', str(f.w), str(f.h), str(n), str(f.order), str(f.depth), str(f.msb), str(f.matrix), str(f.full), str(f.site)],
                         check=True, capture_output=True, text=True).stdout
    return {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}


@pytest.mark.parametrize('matrix,full,depth,n', CONVERSIONS)
def test_anchor_conditions(matrix, full, depth, n, tmp_path):
    """Derived, not measured: the Cb and Cr rows sum to zero, so every grey gives chroma exactly 1 << (n - 1) (= 128 << (n - 8)); black and white
    give the end points of the range; the coefficients equal the model's derivation."""
    exe = build_host_program('unit_rgb')
    f = rf.Format(16, 16, rf.RGBA, depth, 0, matrix, full, 1)
    c = coefficients_of(exe, f, n)
    assert c['ur'] + c['ug'] + c['ub'] == 0 and c['vr'] + c['vg'] + c['vb'] == 0
    want = f.coefficients(n)
    assert {k: c[k] for k in want} == want
    M = f.M
    grey = np.random.default_rng(depth + n).integers(0, M + 1, (16, 16))
    grey[0, :4] = [0, M, 0, M]
    grey[1, :4] = [0, M, M, 0]
    bd = 8 if n == 8 else 12
    rec = rf.random_rec(16, 16, bd, 1)
    before = np.zeros(f.bytes + rf.GUARD, dtype=np.uint8)
    for site in (0, 1):
        f = rf.Format(16, 16, rf.RGBA, depth, 0, matrix, full, site)
        planes, _ = run_unit(exe, f, 0, n, bd, rf.pack(grey, grey, grey, f), rec, before, tmp_path)
        planes = planes.astype(np.int64) >> (bd - n)
        SY, _, OY, OC = f.constants(n)
        assert (OY, OY + SY, OC) == ((16 << (n - 8), 235 << (n - 8), 128 << (n - 8)) if not full else (0, (1 << n) - 1, 1 << (n - 1)))
        assert np.all(planes[256:] == OC), 'a grey input gave chroma off the mid value'
        y = planes[:256].reshape(16, 16)
        assert (y[0, 0], y[0, 1]) == (OY, OY + SY), 'black and white must map to the end points'
        assert np.all(np.diff(y.reshape(-1)[np.argsort(grey.reshape(-1), kind='stable')]) >= 0), 'luma of greys is not monotonic'


@pytest.mark.parametrize('matrix,full,depth,n', CONVERSIONS)
def test_within_one_code_value_of_the_textbook_formula(matrix, full, depth, n):
    """The model (which the row functions equal exactly, above) against float64 rounded to nearest, on random frames, both sitings: at most one code
    value, and that only where the exact value lies next to a rounding step."""
    for site in (0, 1):
        f = rf.Format(40, 24, rf.RGB, depth, 0, matrix, full, site)
        R, G, B = rf.random_rgb(f, 100 + depth + n + site)
        got = rf.to_yuv(R, G, B, f, n).astype(np.int64)
        Y, U, V = rf.textbook_yuv(R, G, B, f, n)
        exact = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)])
        ref = np.clip(np.floor(exact + 0.5), 0, (1 << n) - 1).astype(np.int64)
        diff = np.abs(got - ref)
        assert diff.max() <= 1
        off = diff > 0
        frac = exact[off] + 0.5 - np.floor(exact[off] + 0.5)
        assert np.all(np.minimum(frac, 1 - frac) < 0.02), 'a result differs from float64 away from a rounding step'
        # and back: the inverse of the model's own frame is close to the input where nothing clipped (8 code values of the coarser of the two scales)
        if site == 0 and depth == 8 and n >= 8:
            flat = np.full((24, 40), f.M // 3)
            r, g, b = rf.to_rgb(rf.to_yuv(flat, flat + 7, flat + 20, f, n), f, n)
            assert abs(int(r[4, 4]) - f.M // 3) <= 2 and abs(int(g[4, 4]) - f.M // 3 - 7) <= 2 and abs(int(b[4, 4]) - f.M // 3 - 20) <= 2


def test_model_geometry_and_round_trip():
    """The test's own pack / unpack: inverse of each other, canary elsewhere; BGRA bytes are B G R 255."""
    for order in range(7):
        for depth, msb in rf.DEPTHS:
            for shape in rf.shapes(order, depth):
                f, _ = rf.shaped(order, depth, msb, 1, 0, 1, shape)
                P = rf.random_rgb(f, 3)
                buf = rf.pack(*P, f)
                assert buf.size == f.bytes and all(np.array_equal(a, b) for a, b in zip(rf.unpack(buf, f), P))
    f = rf.Format(16, 16, rf.BGRA)
    R, G, B = rf.random_rgb(f, 1)
    b = rf.pack(R, G, B, f)
    assert (b[0], b[1], b[2], b[3]) == (B[0, 0], G[0, 0], R[0, 0], 255) and f.bytes == 16 * 16 * 4
    f = rf.Format(16, 16, rf.RGBA, 10, 1)
    assert rf.pack(R, G, B, f).view('<u2')[0] == R[0, 0] << 6


# ---- argument checks, without a device -------------------------------------------------------------------------------------------------------------

def test_rgb_format_structure_matches_the_header():
    import thor_amd
    T = thor_amd.RgbFormat
    assert [f[0] for f in T._fields_] == ['size', 'order', 'depth', 'msb_aligned', 'matrix', 'full_range', 'chroma_site', 'pitch', 'plane_stride']
    assert T().size == C.sizeof(T) == 8 * 4 + C.sizeof(C.c_size_t)
    assert [t.order for t in (T.rgba(), T.bgra(), T.rgb24(), T.bgr24(), T.planar())] == [0, 1, 4, 5, 6]
    t = T.bgra(depth=10, matrix=2, full_range=1, chroma_site=0, pitch=512)
    assert (t.depth, t.matrix, t.full_range, t.chroma_site, t.pitch) == (10, 2, 1, 0, 512)
    assert (T.rgba().matrix, T.rgba().full_range, T.rgba().chroma_site) == (1, 0, 1)   # BT.709, limited, left


def test_rgb_bytes_matches_the_model_without_a_device():
    import thor_amd
    T = thor_amd.RgbFormat
    for order in range(7):
        for depth, msb in rf.DEPTHS:
            for shape in rf.shapes(order, depth):
                f, _ = rf.shaped(order, depth, msb, 1, 0, 1, shape)
                assert thor_amd.rgb_bytes(T(**f.fields), f.w, f.h) == f.bytes, (rf.format_id(f), shape)
    assert thor_amd.rgb_bytes(T.bgra(), 80, 48) == 80 * 48 * 4 and thor_amd.rgb_bytes(T.planar(depth=16), 80, 48) == 80 * 48 * 6
    assert thor_amd.lib().thor_hip_rgb_bytes(None, C.byref(T())) == 0


def refused_formats(w, h):
    import thor_amd
    T = thor_amd.RgbFormat
    bad_size = T.bgra()
    bad_size.size -= 4
    return [('size', bad_size), ('order', T(order=7)), ('order', T(order=-1)), ('depth', T.rgba(depth=9)), ('depth', T.rgba(depth=14)),
            ('msb_aligned with depth 8', T.rgba(depth=8, msb_aligned=1)), ('msb_aligned with depth 16', T.rgba(depth=16, msb_aligned=1)),
            ('msb_aligned = 2', T.rgba(depth=10, msb_aligned=2)), ('matrix', T.rgba(matrix=3)), ('matrix', T.rgba(matrix=-1)),
            ('full_range', T.rgba(full_range=2)), ('chroma_site', T.rgba(chroma_site=2)), ('negative pitch', T.rgba(pitch=-512)),
            ('pitch below the row', T.rgba(pitch=w * 4 - 1)), ('pitch below the row', T.rgb24(pitch=w * 3 - 1)),
            ('pitch no multiple of the sample size', T.rgba(depth=16, pitch=w * 8 + 1)), ('plane_stride for a packed order', T(order=0, plane_stride=w * h * 4)),
            ('plane_stride below a plane', T.planar(plane_stride=w * h - 1)), ('plane_stride odd', T.planar(depth=10, plane_stride=w * h * 2 + 1))]


@pytest.mark.parametrize('bd,n', [(8, 8), (10, 8), (12, 10)])
def test_refusals_answer_before_the_device_is_touched(bd, n):
    """rgb_bytes is 0, the known-answer entry points - which validate as thor_hip_stage_frame_rgb / thor_hip_get_recon_rgb do, with the same function,
    and need no encoder - return 1, and so do the encoder calls (a valid call goes on to the device: tests/test_gpu_rgb.py)."""
    import thor_amd
    L = thor_amd.lib()
    w, h = 80, 48
    buf = rf.skewed(w * h * 8 + 64, 0)
    planar = np.zeros(w * h * 3 // 2, dtype=np.uint16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for why, fmt in refused_formats(w, h):
        assert thor_amd.rgb_bytes(fmt, w, h) == 0, why
        assert L.thor_hip_kat_rgb_in(vp(buf), C.byref(fmt), w, h, n, bd, vp(planar)) == 1, why
        assert L.thor_hip_kat_rgb_out(vp(planar), C.byref(fmt), w, h, n, bd, vp(buf)) == 1, why
        assert L.thor_hip_stage_frame_rgb(None, 0, 0, vp(buf), C.byref(fmt), 0) == 1
        assert L.thor_hip_get_recon_rgb(None, 0, vp(buf), C.byref(fmt), 0) == 1
    ok = thor_amd.RgbFormat.bgra()
    assert thor_amd.rgb_bytes(ok, w, h) > 0
    assert thor_amd.rgb_bytes(ok, w + 4, h) == 0 and thor_amd.rgb_bytes(ok, 8, 8) == 0
    assert L.thor_hip_kat_rgb_in(vp(buf), None, w, h, n, bd, vp(planar)) == 1
    assert L.thor_hip_kat_rgb_in(vp(buf), C.byref(ok), w, h, bd + 2, bd, vp(planar)) == 1   # input deeper than the engine
    odd = rf.skewed(w * h * 8 + 64, 1)                                                        # a base pointer that is not sample-aligned
    wide = thor_amd.RgbFormat.bgra(depth=16)
    assert L.thor_hip_kat_rgb_in(vp(odd), C.byref(wide), w, h, n, bd, vp(planar)) == 1
    assert L.thor_hip_kat_rgb_out(vp(planar), C.byref(wide), w, h, n, bd, vp(odd)) == 1


def test_rgb_options_are_front_end_options_at_the_parameter_door():
    import thor_amd
    p = thor_amd.load_config(CFG, width=192, height=128)
    before = bytes(p)
    S = thor_amd.lib().thor_hip_params_set
    assert S(C.byref(p), b'-pixfmt', b'bgra') == 3 and S(C.byref(p), b'-pixfmt', b'rgb24') == 3
    assert S(C.byref(p), b'-rgbmatrix', b'601') == 3 and S(C.byref(p), b'-rgbrange', b'full') == 3 and S(C.byref(p), b'-rgbsite', b'centre') == 3
    assert S(C.byref(p), b'-pixfmt', b'yuy2') == 2 and S(C.byref(p), b'-rgbmatrix', b'240') == 2 and S(C.byref(p), b'-rgbrange', b'pc') == 2
    assert bytes(p) == before
    with pytest.raises(ValueError):
        thor_amd.load_config(CFG, width=192, height=128, pixfmt='bgra')


@pytest.mark.parametrize('binary', ['hostsim_mixed', 'thorenc_hip'])
def test_command_line_refuses_a_bad_rgb_option(binary):
    exe = build_host_program('hostsim_mixed') if binary == 'hostsim_mixed' else os.path.join(ROOT, 'tools', 'thorenc_hip')
    r = subprocess.run([exe, '-cf', CFG, '-if', os.devnull, '-width', '192', '-height', '128', '-qp', '32', '-n', '1', '-pixfmt', 'bgra', '-rgbmatrix', '240'],
                       capture_output=True, text=True)
    assert r.returncode == 2 and 'rgbmatrix' in r.stderr, (r.returncode, r.stderr)
