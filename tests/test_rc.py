"""Rate control on the host (-m "not gpu"): the analysis functions of thor_amd/csrc/tk_rc.h compiled for the host against the numpy restatement
(tests/rc_model.py) and the doors - the validation without a device, thor_hip_params_set, the host simulation's options (thor_hip_set_rate_control's
refusals need a device and are in test_gpu_rc.py).  Whole encodes: tests/test_rc_streams.py."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest
from util import ROOT, GOLD, build_hostsim
import rc_model as rm
from test_frame_layout import build_host_program

CASES = json.load(open(os.path.join(GOLD, 'rc_streams.json')))


# ---- analysis --------------------------------------------------------------------------------------------------------------------------------

def host_analysis(prog, cur, prev, depth, tmp_path):
    h, w = cur.shape
    fi, fo = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    open(fi, 'wb').write(cur.tobytes() + (prev.tobytes() if prev is not None else b''))
    subprocess.run([prog, str(w), str(h), str(depth), str(int(prev is not None)), fi, fo], check=True)
    raw = open(fo, 'rb').read()
    return [int(v) for v in np.frombuffer(raw[:24], dtype=np.uint64)], np.frombuffer(raw[24:], dtype=cur.dtype).reshape(h // 2, w // 2)


@pytest.mark.parametrize('content', rm.KAT_CONTENTS)
@pytest.mark.parametrize('depth', [8, 10, 12])
@pytest.mark.parametrize('w,h', rm.KAT_SHAPES)
def test_host_analysis_matches_numpy(w, h, depth, content, tmp_path):
    cur, prev = rm.kat_case(w, h, depth, content)
    want, want_half = rm.analyse_luma(cur, prev)
    got, got_half = host_analysis(build_host_program('kat_host_rc'), cur, prev, depth, tmp_path)
    assert np.array_equal(got_half, want_half)
    assert got == want
    if content == 'identical':
        assert got[1] == 0
    if content == 'shift_8_m8' and w > 100:   # the corner of the window is found by the blocks whose displaced block lies inside the plane
        assert got[1] < got[0] // 2
    if content == 'max_stripes' and depth == 12 and (w // 2) % 8 == 0 and (h // 2) % 8 == 0:   # whole blocks: the zero vector's 32 * 2559 beats the intra cost 131040
        assert got[1] == 81888 * (w // 16) * (h // 16) and got[2] == 0
    if content == 'max':   # flat at the maximum against zeros: 64 * 4095 per block in the search, which 16 bits do not hold
        assert got[0] == 0 and got[1] == 0 and got[2] == (w // 2 + 7) // 8 * ((h // 2 + 7) // 8)


def test_host_analysis_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined, once, on the shape with partial blocks and the one with several tiles."""
    out, src = os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_rc_san'), os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_rc.cpp')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-strict-aliasing', '-DTHOR_HOSTSIM',
                           '-ffp-contract=off', '-o', out, src])
    for (w, h), depth, content in (((24, 40), 12, 'max'), ((136, 72), 8, 'shift_8_m8'), ((136, 72), 10, 'random')):
        cur, prev = rm.kat_case(w, h, depth, content)
        assert host_analysis(out, cur, prev, depth, tmp_path)[0] == rm.analyse_luma(cur, prev)[0]


# ---- doors -----------------------------------------------------------------------------------------------------------------------------------

def test_rate_control_validation():
    import thor_amd
    R = thor_amd.RateControl
    assert R(1000).ok() and R(0).ok() and R(1000, 500, 10, 40, 5, 30, 20).ok() and R(1000, min_qp=51, max_qp=51).ok()
    bad = [R(-1), R(1000, buffer_ms=-1), R(1000, min_qp=-1, max_qp=10), R(1000, min_qp=30, max_qp=20), R(1000, min_qp_i=30, max_qp_i=20), R(1000, max_qp=52),
           R(1000, max_qp_i=52), R(1000, initial_qp=52), R(1000, initial_qp=-1)]
    assert not any(r.ok() for r in bad)
    wrong = R(1000)
    wrong.size -= 4
    assert not wrong.ok()
    assert thor_amd.lib().thor_hip_rate_control_check(None) == 0


def test_params_set_calls_the_options_front_end_and_keeps_refusing_bitrate():
    import thor_amd
    p = thor_amd.load_config(None)
    before = bytes(p)
    for k, v in (('-rc_bitrate', '100000'), ('-rc_buffer_ms', '500'), ('-rc_min_qp', '10'), ('-rc_max_qp', '40'), ('-rc_min_qpI', '8'), ('-rc_max_qpI', '30'),
                 ('-rc_initial_qp', '28')):
        assert thor_amd.lib().thor_hip_params_set(C.byref(p), k.encode(), v.encode()) == 3
    assert thor_amd.lib().thor_hip_params_set(C.byref(p), b'-rc_max_qp', b'60') == 2
    assert thor_amd.lib().thor_hip_params_set(C.byref(p), b'-rc_unknown', b'1') == 1
    assert thor_amd.lib().thor_hip_params_set(C.byref(p), b'-bitrate', b'1000') == 2
    assert thor_amd.lib().thor_hip_params_set(C.byref(p), b'-max_delta_qp', b'2') == 2
    assert bytes(p) == before


def test_host_simulation_options(tmp_path):
    c = CASES['ldb_30k']
    base = [build_hostsim(), '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', '/dev/null', '-width', '64', '-height', '64', '-qp', '32', '-n', '1']
    for extra in (['-bitrate', '1000'], ['-rc_min_qp', '30', '-rc_max_qp', '20', '-rc_bitrate', '1000'], ['-rc_bitrate', '-5'], ['-rc_nothing', '1']):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 2 and 'Run-time error' in r.stderr
