"""8- and 10-bit input coded at a higher internal bit depth, -bitdepth 10 / 12 with -input_bitdepth 8, or 12 with 10 (-m "not gpu"): the host
simulation of the engine sources (tests/hostsim/hostsim_mixed.cpp) reproduces the reference encoder's streams, reconstruction files (written at
the input depth) and reports (PSNR on the input-depth scale) recorded by tests/golden/gen_streams_mixed.py / gen_reports_mixed.py; a stand-alone
host program runs the three frame-level row functions on full-range vectors against a numpy restatement of the reference's formulas; and the
parameter doors accept the three new pairs and refuse input_bitdepth above bitdepth.  Where oracle/_ref holds the reference binaries, the live
reference agrees with the recorded hashes and its decoder reproduces the reconstruction of the CDEF-off case.

One case has input of more than 8 bits, 192x128_n5_q32_hdb16_gop4_in10_bd12.  Half of the reference's reconstruction file is uninitialised
memory there (tests/mixed_depth.py explains the reference's row buffer), so that file is compared in the half the reference defines
(rec_defined_md5: the low byte of every sample) and, whole, with what a second run of the reference gives that writes its file correctly
(rec_equal_depth_md5: the clip widened beforehand, equal depths, rounded with the reference's formula); bitstream and report are compared
whole like everywhere else."""
import ctypes as C
import json
import os
import subprocess
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, REF_ENC, REF_DEC, golden_clip, run_encoder, decode, md5
from mixed_depth import defined_rec_bytes, depth_vectors, depth_expected, DEPTH_PAIRS, DEPTH_GEOMETRIES

G = json.load(open(os.path.join(GOLD, 'streams_mixed.json')))
REPORTS = json.load(open(os.path.join(GOLD, 'reports_mixed.json')))
CFG = os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')
CASES = sorted(G)
HOSTSIM_DIR = os.path.join(ROOT, 'tests', 'hostsim')
_BUILT = {}
_RUNS = {}


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


def hostsim_run(name):
    """(bits, recon, stdout) of hostsim_mixed on a case of streams_mixed.json: one run per case, shared by the tests."""
    if name not in _RUNS:
        c = G[name]
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
            cmd = [build_host_program('hostsim_mixed'), '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'),
                   '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30',
                   '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + c['extra']
            out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
            _RUNS[name] = (open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.yuv'), 'rb').read(), out)
    return _RUNS[name]


def check_recon(c, rec):
    """`rec` (a correct file of input-depth samples) against the reference's -rf file as recorded in case `c`."""
    assert len(rec) == c['rec_bytes']
    if 'rec_defined_md5' in c:
        assert md5(defined_rec_bytes(rec, c['w'], c['h'], c['n'], False)) == c['rec_defined_md5'], 'reconstruction differs from the reference'
        assert md5(rec) == c['rec_equal_depth_md5'], 'reconstruction differs from the rounded equal-depth run of the reference'
    else:
        assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


def test_goldens_are_the_cases_they_claim_to_be():
    assert CASES == sorted(['192x128_n4_q32_in8_bd10', '192x128_n3_q32_skip0_in8_bd10', '192x128_n3_q32_skip3_in8_bd10', '208x120_n4_q36_in8_bd12_clpf',
                            '208x120_n4_q36_in8_bd10_nocdef', '128x96_n9_q32_ra_in8_bd10', '192x128_n5_q32_hdb16_gop4_in10_bd12',
                            '208x120_n4_q32_in8_bd10_sb64'])
    assert sorted(REPORTS) == CASES
    equal = json.load(open(os.path.join(GOLD, 'streams.json')))
    for name, c in G.items():
        e = c['extra']
        bd, inp = int(e[e.index('-bitdepth') + 1]), int(e[e.index('-input_bitdepth') + 1])
        assert (bd, inp) in DEPTH_PAIRS and ('in%d_bd%d' % (inp, bd)) in name
        # the -rf file holds input-depth samples (what the issue measured: 110 592 bytes for three 8-bit frames of 192x128)
        assert c['rec_bytes'] == c['w'] * c['h'] * 3 // 2 * c['n'] * (2 if inp > 8 else 1) and len(c['frames']) == c['n']
        assert ('rec_defined_md5' in c) == (inp > 8) == ('rec_equal_depth_md5' in c)
    assert G['192x128_n3_q32_skip0_in8_bd10']['rec_bytes'] == 110592 and G['192x128_n3_q32_skip0_in8_bd10']['bit_bytes'] == 1664
    # neither the 8-bit nor the 10-bit stream of the same command
    assert G['192x128_n3_q32_skip0_in8_bd10']['bit_md5'] not in (equal['192x128_n3_q32']['bit_md5'], equal['192x128_n4_q32_10bit']['bit_md5'])


@pytest.mark.parametrize('name', CASES)
def test_host_simulation_matches_reference_golden(name):
    bits, rec, out = hostsim_run(name)
    c = G[name]
    assert len(bits) == c['bit_bytes']
    assert md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    check_recon(c, rec)
    rep = REPORTS[name]['report']
    assert out == rep, 'report differs from the reference'
    assert [l.split()[:4] for l in rep.splitlines()[1:1 + c['n']]] == c['frames']


def test_report_psnr_is_on_the_input_depth_scale():
    """The same 8-bit clip at (10, 8): were maxsignal taken from the internal depth the PSNRs would sit 12 dB higher (20 log10(1023 / 255))."""
    rep = REPORTS['192x128_n4_q32_in8_bd10']['report']
    y = [float(l.split()[4]) for l in rep.splitlines()[1:5]]
    assert all(30 < v < 40 for v in y), y


@pytest.mark.skipif(not os.path.exists(REF_ENC), reason='oracle/_ref/Thorenc not built')
@pytest.mark.parametrize('name', CASES)
def test_live_reference_agrees_with_recorded_hashes(name):
    c = G[name]
    bits, rec = run_encoder(REF_ENC, golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c['cfg'])
    assert md5(bits) == c['bit_md5'] and len(bits) == c['bit_bytes'] and len(rec) == c['rec_bytes']
    if 'rec_defined_md5' in c:
        assert md5(defined_rec_bytes(rec, c['w'], c['h'], c['n'], True)) == c['rec_defined_md5']
    else:
        assert md5(rec) == c['rec_md5']


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason='oracle/_ref/Thordec not built')
def test_reference_decoder_reproduces_the_reconstruction():
    bits, rec, _ = hostsim_run('208x120_n4_q36_in8_bd10_nocdef')
    assert decode(bits) == rec


@pytest.mark.parametrize('bd,inp', DEPTH_PAIRS)
@pytest.mark.parametrize('w,h', DEPTH_GEOMETRIES)
def test_row_functions_match_the_reference_formulas(w, h, bd, inp, tmp_path):
    """depth_up_rows, depth_down_rows and frame_sse_depth_rows (tests/hostsim/unit_depth.cpp), as one work item and split like a launch."""
    vin, a, b = depth_vectors(w, h, bd, inp)
    (tmp_path / 'in').write_bytes(vin.tobytes() + a.tobytes() + b.tobytes())
    subprocess.run([build_host_program('unit_depth'), str(w), str(h), str(bd), str(inp), str(tmp_path / 'in'), str(tmp_path / 'out')], check=True)
    out = (tmp_path / 'out').read_bytes()
    n = w * h * 3 // 2
    up, down, sse = depth_expected(w, h, bd, inp, vin, a, b)
    assert down.max() == (1 << inp) - 1 and int(a.max() + (1 << (bd - inp - 1))) >> (bd - inp) > down.max(), 'the vectors must reach the clamp'
    assert np.array_equal(np.frombuffer(out[:2 * n], dtype=np.uint16), up)
    nb = n * vin.itemsize
    assert np.array_equal(np.frombuffer(out[2 * n:2 * n + nb], dtype=vin.dtype), down)
    assert list(np.frombuffer(out[2 * n + nb:], dtype=np.uint64)) == sse and all(sse)


def test_row_functions_are_clean_under_the_host_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined (it has its own main: nothing is preloaded): no vector reaches past a
    row or is misaligned, at the geometry whose chroma rows are no multiple of a 16-byte vector and at the smallest one."""
    exe = os.path.join(HOSTSIM_DIR, 'unit_depth_san')
    src = os.path.join(HOSTSIM_DIR, 'unit_depth.cpp')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-o', exe, src])
    for w, h in DEPTH_GEOMETRIES + [(8, 8)]:
        for bd, inp in DEPTH_PAIRS:
            vin, a, b = depth_vectors(w, h, bd, inp)
            (tmp_path / 'in').write_bytes(vin.tobytes() + a.tobytes() + b.tobytes())
            r = subprocess.run([exe, str(w), str(h), str(bd), str(inp), str(tmp_path / 'in'), str(tmp_path / 'out')], capture_output=True, text=True)
            assert r.returncode == 0 and not r.stderr, (w, h, bd, inp, r.stderr[-2000:])


def test_open_without_a_device_returns_null_and_leaves_the_process_alive():
    """A parameter set that is in order cannot be opened on a machine without a device: thor_hip_open says so with NULL (and a message), as it
    does for a device index the node does not have.  With a device the same call opens."""
    import thor_amd
    L = thor_amd.lib()
    p = _params(10, 8)
    h = L.thor_hip_open(C.byref(p), 1, 0)
    if L.thor_hip_device_count() < 1:
        assert not h
    else:
        assert h
        L.thor_hip_close(h)


def _params(bd, inp, **kw):
    import thor_amd
    return thor_amd.load_config(CFG, width=192, height=128, qp=32, f=30, bitdepth=bd, input_bitdepth=inp, **kw)


@pytest.mark.parametrize('bd,inp', [(8, 10), (8, 12), (10, 12), (10, 9), (9, 8)])
def test_open_refuses_the_pair_before_it_touches_the_device(bd, inp):
    """thor_hip_open validates the parameters before it initialises HIP: NULL comes back on a machine without a GPU too.  (The three new pairs
    get past that check and reach the device: tests/test_gpu_mixed_depth.py opens them.)"""
    import thor_amd
    p = _params(bd, inp)
    assert (p.bitdepth, p.input_bitdepth) == (bd, inp)
    assert not thor_amd.lib().thor_hip_open(C.byref(p), 1, 0)


@pytest.mark.parametrize('bd,inp', DEPTH_PAIRS)
def test_load_config_takes_the_new_pairs(bd, inp):
    p = _params(bd, inp)
    assert (p.bitdepth, p.input_bitdepth) == (bd, inp)


def test_frame_bytes_symbol_and_null_handle():
    import thor_amd
    L = thor_amd.lib()
    L.thor_hip_frame_bytes.restype = C.c_size_t
    L.thor_hip_frame_bytes.argtypes = [C.c_void_p]
    assert L.thor_hip_frame_bytes(None) == 0
    for name in ('thor_hip_kat_depth_up', 'thor_hip_kat_depth_down', 'thor_hip_frame_sse_depth'):
        assert hasattr(L, name)
    # bad arguments are refused before the device is touched
    buf = np.zeros(16 * 16 * 3, dtype=np.uint16)
    vp = buf.ctypes.data_as(C.c_void_p)
    assert thor_amd.lib().thor_hip_kat_depth_up(vp, 16, 16, 8, 10, vp) == 1
    assert thor_amd.lib().thor_hip_kat_depth_down(vp, 16, 16, 10, 10, vp) == 1
    assert thor_amd.lib().thor_hip_kat_depth_up(vp, 20, 16, 10, 8, vp) == 1


def test_params_layout_is_unchanged():
    """thor_hip_params keeps its layout: both depth fields existed already."""
    import thor_amd
    T = thor_amd.binding.ThorParams
    names = [f[0] for f in T._fields_]
    assert names[3:5] == ['bitdepth', 'input_bitdepth'] and names[-1] == 'log2_sb_size'
    assert [getattr(T, n).offset for n in names] == [4 * i for i in range(len(names))] and C.sizeof(T) == 4 * len(names)


@pytest.mark.parametrize('binary', ['hostsim_mixed', 'thorenc_hip'])
def test_command_line_exits_2_when_the_input_is_deeper_than_the_encoder(binary):
    exe = build_host_program('hostsim_mixed') if binary == 'hostsim_mixed' else os.path.join(ROOT, 'tools', 'thorenc_hip')
    for bd, inp in ((8, 10), (8, 12), (10, 12)):
        r = subprocess.run([exe, '-cf', CFG, '-if', os.devnull, '-width', '192', '-height', '128', '-qp', '32', '-n', '1',
                            '-bitdepth', str(bd), '-input_bitdepth', str(inp)], capture_output=True, text=True)
        assert r.returncode == 2 and 'input_bitdepth' in r.stderr, (bd, inp, r.returncode, r.stderr)
