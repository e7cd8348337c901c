"""Frames in NV12 / NV21 / P010 layouts with a row pitch (-m "not gpu"): the two row functions behind thor_hip_stage_frame_layout and
thor_hip_get_recon_layout run on the host (tests/hostsim/unit_layout.cpp, one lane and 64 lanes) against numpy over the grid of
tests/frame_layout.py; whole encodes through the host simulation with -pixfmt nv12 / p010 reproduce the recorded bitstreams and, converted back
in the test, the recorded reconstructions; the argument checks answer without a device.  Every comparison is exact."""
import ctypes as C
import json
import os
import subprocess
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, golden_clip, md5
import frame_layout as fl

HOSTSIM_DIR = os.path.join(ROOT, 'tests', 'hostsim')
STREAMS = json.load(open(os.path.join(GOLD, 'streams.json')))
MIXED = json.load(open(os.path.join(GOLD, 'streams_mixed.json')))
CFG = os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')
_BUILT = {}


def build_host_program(name):
    """tests/hostsim/<name>.cpp with the flags of util.build_hostsim (1-lane teams)."""
    if name not in _BUILT:
        out, src = os.path.join(HOSTSIM_DIR, name), os.path.join(HOSTSIM_DIR, name + '.cpp')
        csrc = os.path.join(ROOT, 'thor_amd', 'csrc')
        deps = [src, os.path.join(HOSTSIM_DIR, 'hostsim.cpp')] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
            subprocess.check_call(['g++', '-std=c++17', '-O2', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-pthread', '-o', out, src])
        _BUILT[name] = out
    return _BUILT[name]


# ---- the row functions on the host ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout', fl.LAYOUTS, ids=fl.layout_id)
@pytest.mark.parametrize('w,h', fl.SIZES)
def test_row_functions_match_numpy(w, h, layout, tmp_path):
    """layout_in_rows and layout_out_rows, as one work item with one lane and split over 64-lane teams, for every pitch and base offset: the planes
    equal numpy's; in the destination every sample of the picture equals numpy's and every other byte - row padding, gaps, guard - is untouched."""
    exe = build_host_program('unit_layout')
    chroma, msb, inp, bd, _ = layout
    fin, rec = fl.vectors(w, h, inp, bd)
    n = w * h * 3 // 2
    for pitch in fl.PITCHES:
        g = fl.case_geometry(w, h, layout, pitch)
        src = fl.pack(fin, g)
        before = np.full(g.bytes + fl.GUARD, fl.CANARY, dtype=np.uint8)
        want_dst = before.copy()
        fl.pack(fl.expect_out(rec, inp, bd), g, into=want_dst[:g.bytes])
        for skew in fl.SKEWS:
            (tmp_path / 'in').write_bytes(src.tobytes() + rec.tobytes() + before.tobytes())
            f = g.fields
            subprocess.run([exe, str(w), str(h), str(inp), str(bd), str(chroma), str(msb), str(f['pitch_y']), str(f['pitch_c']), str(f['offset_u']),
                            str(f['offset_v']), str(skew * g.B), str(tmp_path / 'in'), str(tmp_path / 'out')], check=True)
            out = (tmp_path / 'out').read_bytes()
            nb = n * rec.itemsize
            assert len(out) == nb + g.bytes + fl.GUARD
            assert np.array_equal(np.frombuffer(out[:nb], dtype=rec.dtype), fl.expect_in(fin, inp, bd)), (pitch, skew)
            assert np.array_equal(np.frombuffer(out[nb:], dtype=np.uint8), want_dst), (pitch, skew)


def test_numpy_restatement_round_trips():
    """The test's own pack / unpack: inverse of each other, canary everywhere else, and NV12 of a tight frame is Y then U0 V0 U1 V1 ..."""
    w, h = 16, 16
    fin, _ = fl.vectors(w, h, 8, 8)
    g = fl.Geometry(w, h, 8, fl.UV)
    b = fl.pack(fin, g)
    y, u, v = fl.planes(fin, w, h)
    assert g.bytes == w * h * 3 // 2 and np.array_equal(b[:w * h], fin[:w * h])
    assert np.array_equal(b[w * h::2], u.reshape(-1)) and np.array_equal(b[w * h + 1::2], v.reshape(-1))
    for layout in fl.LAYOUTS:
        fin, _ = fl.vectors(w, h, layout[2], layout[3])
        for pitch in fl.PITCHES:
            g = fl.case_geometry(w, h, layout, pitch)
            assert np.array_equal(fl.unpack(fl.pack(fin, g), g), fin)
    g = fl.Geometry(w, h, 10, fl.UV, 1)
    f10, _ = fl.vectors(w, h, 10, 10)
    assert np.array_equal(fl.pack(f10, g)[:2 * w * h].view('<u2'), f10[:w * h].astype(np.uint16) << 6)


# ---- whole encodes through the host simulation -----------------------------------------------------------------------------------------------

def hostsim_pixfmt(c, pixfmt, g):
    """hostsim_mixed on case `c` with the clip converted to `pixfmt` here; returns (bits, the -rf file converted back to planar here)."""
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(fl.convert_clip(golden_clip(c['clip']), g, c['n']))
        cmd = [build_host_program('hostsim_mixed'), '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'),
               '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30',
               '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv'), '-pixfmt', pixfmt] + c['extra']
        subprocess.run(cmd, check=True, capture_output=True, text=True)
        rec = open(os.path.join(d, 'o.yuv'), 'rb').read()
        return open(os.path.join(d, 'o.bit'), 'rb').read(), fl.convert_clip(rec, g, c['n'], back=True)


ENCODES = [('208x120_n4_q32', STREAMS, 'nv12', fl.UV, 0, 8), ('192x128_n4_q32_10bit', STREAMS, 'p010', fl.UV, 1, 10),
           ('208x120_n4_q32', STREAMS, 'nv21', fl.VU, 0, 8), ('192x128_n4_q32_in8_bd10', MIXED, 'nv12', fl.UV, 0, 8)]


@pytest.mark.parametrize('name,table,pixfmt,chroma,msb,inp', ENCODES, ids=['%s-%s' % (e[0], e[2]) for e in ENCODES])
def test_host_simulation_with_pixfmt_matches_reference_golden(name, table, pixfmt, chroma, msb, inp):
    c = table[name]
    bits, rec = hostsim_pixfmt(c, pixfmt, fl.Geometry(c['w'], c['h'], inp, chroma, msb))
    assert len(bits) == c['bit_bytes'] and md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@pytest.mark.parametrize('binary', ['hostsim_mixed', 'thorenc_hip'])
def test_command_line_exits_2_for_p010_with_8_bit_input(binary):
    exe = build_host_program('hostsim_mixed') if binary == 'hostsim_mixed' else os.path.join(ROOT, 'tools', 'thorenc_hip')
    r = subprocess.run([exe, '-cf', CFG, '-if', os.devnull, '-width', '192', '-height', '128', '-qp', '32', '-n', '1', '-pixfmt', 'p010'],
                       capture_output=True, text=True)
    assert r.returncode == 2 and 'pixfmt' in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([exe, '-cf', CFG, '-if', os.devnull, '-width', '192', '-height', '128', '-qp', '32', '-n', '1', '-pixfmt', 'yuy2'],
                       capture_output=True, text=True)
    assert r.returncode == 2 and 'pixfmt' in r.stderr, (r.returncode, r.stderr)


# ---- argument checks, without a device ---------------------------------------------------------------------------------------------------------

def test_pixfmt_is_a_front_end_option_at_the_parameter_door():
    import thor_amd
    p = thor_amd.load_config(CFG, width=192, height=128)
    before = bytes(p)
    assert thor_amd.lib().thor_hip_params_set(C.byref(p), b'-pixfmt', b'nv12') == 3
    assert thor_amd.lib().thor_hip_params_set(C.byref(p), b'-pixfmt', b'p010') == 3
    assert bytes(p) == before
    with pytest.raises(ValueError):
        thor_amd.load_config(CFG, width=192, height=128, pixfmt='nv12')


def test_layout_structure_matches_the_header():
    import thor_amd
    T = thor_amd.FrameLayout
    assert [f[0] for f in T._fields_] == ['size', 'chroma', 'msb_aligned', 'pitch_y', 'pitch_c', 'offset_u', 'offset_v']
    assert T().size == C.sizeof(T) == 5 * 4 + 4 + 2 * C.sizeof(C.c_size_t)   # five ints, padding, two size_t
    assert (T.nv12().chroma, T.nv21().chroma, T.p010().chroma, T.planar().chroma) == (1, 2, 1, 0)
    assert (T.nv12().msb_aligned, T.p010().msb_aligned) == (0, 1)
    assert (T.nv12(pitch=256).pitch_y, T.nv12(pitch=256).pitch_c) == (256, 256)


def test_layout_bytes_without_a_device():
    import thor_amd
    T = thor_amd.FrameLayout
    w, h = 208, 120
    nbytes = lambda l, inp=8: thor_amd.layout_bytes(l, w, h, inp)
    assert nbytes(T()) == nbytes(T.nv12()) == nbytes(T.nv21()) == w * h * 3 // 2
    assert nbytes(T.nv12(pitch=256)) == 256 * h * 3 // 2
    assert nbytes(T.p010(), 10) == nbytes(T.planar(), 10) == w * h * 3
    assert nbytes(T.p010(pitch=512), 12) == 512 * h * 3 // 2
    assert nbytes(T.planar(pitch_y=256, pitch_c=128)) == 256 * h + 2 * 128 * (h // 2)
    assert nbytes(T.planar(offset_u=w * h + 32, offset_v=w * h + 32 + w * h // 4 + 48)) == w * h * 3 // 2 + 80
    # YV12: V before U
    assert nbytes(T.planar(offset_u=w * h + w * h // 4, offset_v=w * h)) == w * h * 3 // 2
    # the grid's geometries agree with the test's own arithmetic
    for layout in fl.LAYOUTS:
        for pitch in fl.PITCHES:
            g = fl.case_geometry(w, h, layout, pitch)
            assert thor_amd.layout_bytes(T(**g.fields), w, h, layout[2]) == g.bytes
    assert thor_amd.lib().thor_hip_layout_bytes(None, C.byref(T())) == 0


def refused_layouts(w, inp):
    """(why, FrameLayout) for every refusal include/thor_hip.h lists, against a picture `w` wide with `inp`-bit samples."""
    import thor_amd
    T = thor_amd.FrameLayout
    B = 2 if inp > 8 else 1
    bad_size = T.nv12()
    bad_size.size -= 4
    out = [('size', bad_size), ('chroma', T(chroma=3)), ('chroma', T(chroma=-1)),
           ('luma pitch below the row', T.nv12(pitch=w * B - B)), ('chroma pitch below the row', T(chroma=1, pitch_y=w * B, pitch_c=w * B - B)),
           ('planar chroma pitch below the row', T.planar(pitch_c=w // 2 * B - B)), ('negative pitch', T.planar(pitch_y=-256))]
    if inp > 8:
        out += [('pitch no multiple of the sample size', T.p010(pitch=w * B + 1)), ('offset_u odd', T.planar(offset_u=w * 128 * B + 1)),
                ('offset_v odd', T.planar(offset_v=w * 128 * B * 2 + 1)), ('msb_aligned = 2', T(chroma=1, msb_aligned=2))]
    else:
        out += [('msb_aligned with 8-bit input', T.p010()), ('msb_aligned planar with 8-bit input', T.planar(msb_aligned=1))]
    return out


@pytest.mark.parametrize('inp,bd', [(8, 8), (10, 10), (8, 10)])
def test_refusals_answer_1_before_the_device_is_touched(inp, bd):
    """layout_bytes is 0 and both known-answer entry points - which validate as thor_hip_stage_frame_layout / thor_hip_get_recon_layout do, with
    the same function, and need no encoder - return 1 (a valid call goes on to the device: tests/test_gpu_frame_layout.py)."""
    import thor_amd
    L = thor_amd.lib()
    w, h = 192, 128
    buf = fl.skewed(w * h * 3 * 2 + 64, 0)
    planar = np.zeros(w * h * 3 // 2, dtype=np.uint16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for why, lay in refused_layouts(w, inp):
        assert thor_amd.layout_bytes(lay, w, h, inp) == 0, why
        assert L.thor_hip_kat_layout_in(vp(buf), C.byref(lay), w, h, inp, bd, vp(planar)) == 1, why
        assert L.thor_hip_kat_layout_out(vp(planar), C.byref(lay), w, h, inp, bd, vp(buf)) == 1, why
        assert L.thor_hip_stage_frame_layout(None, 0, 0, vp(buf), C.byref(lay), 0) == 1
        assert L.thor_hip_get_recon_layout(None, 0, vp(buf), C.byref(lay), 0) == 1
    ok = thor_amd.FrameLayout.p010() if inp > 8 else thor_amd.FrameLayout.nv12()
    assert thor_amd.layout_bytes(ok, w, h, inp) > 0
    assert L.thor_hip_kat_layout_in(vp(buf), None, w, h, inp, bd, vp(planar)) == 1
    assert L.thor_hip_kat_layout_in(vp(buf), C.byref(ok), w, h, bd + 2, bd, vp(planar)) == 1   # input deeper than the engine
    assert L.thor_hip_kat_layout_in(vp(buf), C.byref(ok), w + 4, h, inp, bd, vp(planar)) == 1
    if inp > 8:   # a base pointer that is not sample-aligned
        odd = fl.skewed(w * h * 3 + 64, 1)
        assert L.thor_hip_kat_layout_in(vp(odd), C.byref(ok), w, h, inp, bd, vp(planar)) == 1
        assert L.thor_hip_kat_layout_out(vp(planar), C.byref(ok), w, h, inp, bd, vp(odd)) == 1
