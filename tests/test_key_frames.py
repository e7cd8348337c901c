"""Key frames on request and at scene cuts, through the host simulation (-m "not gpu"): -key_frames reproduces the reference's -intra_period streams byte for
byte, a key frame at an arbitrary frame decodes and cuts the references, requests that change nothing and refusals, the scene-cut rule against its Python
restatement (tests/key_model.py), with rate control, and several streams in one engine."""
import ctypes as C
import json
import os
import subprocess
import pytest
from util import ROOT, GOLD, REF_DEC, build_hostsim, decode, golden_clip, md5
import key_model as km
import rc_model as rm

KS = json.load(open(os.path.join(GOLD, 'key_streams.json')))
_RUNS = {}


def clip_of(c):
    return km.cut_clip()[1] if c['clip'] == 'cut' else golden_clip(c['clip'])


def host(c, extra=(), **kw):
    """One host-simulation run per case and variant, shared by the tests of this file."""
    key = json.dumps([c['clip'], c['w'], c['h'], c['n'], c['qp'], list(extra), kw], sort_keys=True)
    if key not in _RUNS:
        _RUNS[key] = km.run(build_hostsim(), clip_of(c), c['w'], c['h'], c['n'] // kw.get('streams', 1), c['qp'], extra, **kw)
    return _RUNS[key]


def frame_rows(report):
    """(type, [frame number of each reference]) per coded frame from the reference-style report: the numbers after the bar."""
    return [(l.split()[1], [int(v) for v in l.split('|')[1].split()]) for l in report.splitlines() if len(l.split()) > 4 and l.split()[1] in 'IPB' and '|' in l]


def frame_chunks(bits):
    out, pos = [], 0
    while pos < len(bits):
        n = int.from_bytes(bits[pos:pos + 4], 'big')
        out.append(bits[pos:pos + 4 + n])
        pos += 4 + n
    return out


# ---- 1. exactness against the reference ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(KS['ref']))
def test_intra_period_reproduces_the_reference(name):
    c = KS['ref'][name]
    r = host(c, c['extra'])
    assert md5(r['bits'][0]) == c['bit_md5'] and md5(r['rec'][0]) == c['rec_md5']


@pytest.mark.parametrize('name', sorted(KS['ref']))
def test_forced_key_frames_reproduce_the_reference_intra_period(name):
    c = KS['ref'][name]
    r = host(c, ['-intra_period', '0', '-key_frames', c['keys']] + c.get('keys_extra', []))
    assert md5(r['bits'][0]) == c['bit_md5'] and md5(r['rec'][0]) == c['rec_md5']


# ---- 2. a key frame at an arbitrary frame ---------------------------------------------------------------------------------------------------------------

BASE = KS['ref']['period4']


def test_key_frame_at_frame_2_cuts_the_references():
    r = host(BASE, ['-cdef', '0', '-key_frames', '2'])
    plain = host(BASE, ['-cdef', '0'])
    rows = km.parse_log(r['key_log'])
    assert [(x['frame_type'], x['reason']) for x in rows] == [(0, 0), (1, 0), (0, 1), (1, 0), (1, 0), (1, 0)]
    a, b = frame_chunks(r['bits'][0]), frame_chunks(plain['bits'][0])
    assert len(a) == len(b) == 6 and a[:2] == b[:2] and a[2] != b[2]
    fsz = 192 * 128 * 3 // 2
    assert r['rec'][0][:2 * fsz] == plain['rec'][0][:2 * fsz]
    assert md5(r['bits'][0]) == KS['host']['key2_nocdef']['bit_md5']


def test_no_later_frame_refers_to_a_frame_before_the_key_frame():
    r = host(BASE, ['-cdef', '0', '-key_frames', '2'])
    rows = frame_rows(r['report'])
    assert [x[0] for x in rows] == ['I', 'P', 'I', 'P', 'P', 'P'] and rows[1][1] == [0] and rows[2][1] == []
    assert all(refs and min(refs) >= 2 for _, refs in rows[3:]), rows


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason='reference decoder not built')
def test_reference_decoder_reproduces_the_reconstruction():
    r = host(BASE, ['-cdef', '0', '-key_frames', '2'])   # with CDEF on the reference's own decoder does not reproduce its encoder (tests/test_sb64.py)
    assert decode(r['bits'][0]) == r['rec'][0]


# ---- 3. requests that change nothing, refusals -------------------------------------------------------------------------------------------------------

def test_requests_that_change_nothing():
    plain = host(BASE, [])
    assert host(BASE, ['-key_frames', '0'])['bits'] == plain['bits']
    p4 = host(BASE, ['-intra_period', '4'])
    again = host(BASE, ['-intra_period', '4', '-key_frames', '4'])
    assert again['bits'] == p4['bits'] and [x['reason'] for x in km.parse_log(again['key_log'])] == [0] * 6


def test_front_end_refusals():
    clip = clip_of(BASE)
    for extra, cfg in ((['-key_frames', '2'], 'ra_high_efficiency.cfg'), (['-key_scenecut', '80'], 'ra_high_efficiency.cfg'), (['-key_scenecut', '101'], 'ldb_high_efficiency.cfg'),
                       (['-key_min_interval', '-1'], 'ldb_high_efficiency.cfg'), (['-key_frames', '1,x'], 'ldb_high_efficiency.cfg'),
                       (['-key_frames', ','.join(map(str, range(km.MAX_REQUESTS + 1)))], 'ldb_high_efficiency.cfg')):
        r = km.run(build_hostsim(), clip, 192, 128, 2, extra=extra, cfg=cfg, check=False)
        assert r['returncode'] == 2 and 'Run-time error' in r['stderr'], extra


def _lib():
    import thor_amd
    thor_amd.lib()   # raises when the library is not built
    return thor_amd


def test_scene_cut_check_needs_no_device():
    t = _lib()
    assert t.SceneCut(0).ok() and t.SceneCut(1).ok() and t.SceneCut(100, 7).ok() and t.lib().thor_hip_scene_cut_check(None) == 0
    assert not t.SceneCut(101).ok() and not t.SceneCut(-1).ok() and not t.SceneCut(50, -1).ok()
    bad = t.SceneCut(50)
    bad.size += 4
    assert not bad.ok()
    assert t.lib().thor_hip_force_key_frame(None, 0, 0) == 1 and t.lib().thor_hip_set_scene_cut(None, 0, None) == 1


def test_layout_of_the_new_structures(tmp_path):
    """The C compiler's layout of thor_hip_scene_cut and thor_hip_frame_key against the ctypes mirrors of thor_amd/binding.py."""
    from thor_amd import binding as b
    src = tmp_path / 'lay.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thor_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(thor_hip_scene_cut), offsetof(thor_hip_scene_cut, size), offsetof(thor_hip_scene_cut, percent), offsetof(thor_hip_scene_cut, min_interval));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(thor_hip_frame_key), offsetof(thor_hip_frame_key, reason), offsetof(thor_hip_frame_key, sum_intra), offsetof(thor_hip_frame_key, sum_best), offsetof(thor_hip_frame_key, n_intra));\n'
                   '  return 0;\n}\n')
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(tmp_path / 'lay'), str(src)])
    got = subprocess.run([str(tmp_path / 'lay')], check=True, capture_output=True, text=True).stdout.split()
    want = [C.sizeof(b.SceneCut)] + [getattr(b.SceneCut, f).offset for f, _ in b.SceneCut._fields_] + \
           [C.sizeof(b.FrameKey)] + [getattr(b.FrameKey, f).offset for f, _ in b.FrameKey._fields_]
    assert list(map(int, got)) == want == [12, 0, 4, 8, 32, 0, 8, 16, 24]


# ---- 4. scene cut ------------------------------------------------------------------------------------------------------------------------------------

CUT = KS['host']['cut']
_MODEL = {}


def model(**kw):
    key = json.dumps(kw, sort_keys=True)
    if key not in _MODEL:
        _MODEL[key] = km.schedule([f[0] for f in km.cut_clip()[0]], **kw)
    return _MODEL[key]


def logged(r, stream=0):
    return [(x['frame_type'], x['reason'], [x['sum_intra'], x['sum_best'], x['n_intra']]) for x in km.parse_log(r['key_log']) if x['stream'] == stream]


def test_recorded_ratios_separate():
    q = KS['ratios']
    cut, within = q['per_frame_from_1'][km.CUT_AT - 1], q['per_frame_from_1'][:km.CUT_AT - 1] + q['per_frame_from_1'][km.CUT_AT:]
    assert q['percent'] == km.PERCENT and max(within) + 10 <= km.PERCENT and cut >= km.PERCENT + 5


def test_scene_cut_matches_the_model():
    r = host(CUT, CUT['extra'])
    want = model(percent=km.PERCENT)
    assert logged(r) == want
    assert [n for n, x in enumerate(want) if x[1] == km.KEY_SCENE_CUT] == [km.CUT_AT] and [x[0] for x in want] == [0, 1, 1, 1, 0, 1, 1, 1]
    assert frame_rows(r['report'])[km.CUT_AT] == ('I', [])


def test_min_interval_above_the_distance_promotes_nothing():
    r = host(CUT, ['-key_scenecut', str(km.PERCENT), '-key_min_interval', '5'])
    assert logged(r) == model(percent=km.PERCENT, min_interval=5) and [x[1] for x in logged(r)] == [0] * 8
    plain = host(CUT, [])
    assert r['bits'] == plain['bits'] and r['rec'] == plain['rec']


def test_forced_frame_counts_for_the_interval():
    """A forced key frame at 2 with min_interval 3: frame 4 is 2 frames after it and stays a P frame."""
    r = host(CUT, ['-key_scenecut', str(km.PERCENT), '-key_min_interval', '3', '-key_frames', '2'])
    assert logged(r) == model(percent=km.PERCENT, min_interval=3, forced=(2,)) and [x[1] for x in logged(r)] == [0, 0, 1, 0, 0, 0, 0, 0]


# ---- 5. with rate control ----------------------------------------------------------------------------------------------------------------------------

def test_rate_control_sees_the_cut_as_class_0():
    c = KS['host']['cut_rc']
    r = host(c, c['extra'])
    rows = rm.parse_log(r['rc_log'])
    assert len(rows) == 8 and rows[km.CUT_AT]['frame_class'] == 0 and [x['frame_class'] for x in rows] == [0, 1, 1, 1, 0, 1, 1, 1]
    p = rm.read_params(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), c['qp'])
    got, _ = rm.replay(rows, p, bitrate=60000)
    assert got == [(x['base_qp'], x['qp'], x['fullness'], x['overflows']) for x in rows]
    assert logged(r) == model(percent=km.PERCENT)
    assert [(x['sum_intra'], x['sum_best'], x['n_intra']) for x in rows] == [tuple(x[2]) for x in logged(r)]


# ---- 6. several streams in one engine ----------------------------------------------------------------------------------------------------------------

def test_two_streams_with_different_requests_match_their_single_stream_runs():
    """THOR_KEY_SHIFT=1: stream 0 (frames 0 .. 3) asks for a key frame at 1, stream 1 (frames 4 .. 7) at 2."""
    two = host(CUT, ['-key_frames', '1'], streams=2, env={'THOR_KEY_SHIFT': '1'})
    for s, key in ((0, '1'), (1, '2')):
        one = km.run(build_hostsim(), clip_of(CUT), CUT['w'], CUT['h'], 4, CUT['qp'], ['-skip', str(4 * s), '-key_frames', key])
        assert one['bits'][0] == two['bits'][s] and one['rec'][0] == two['rec'][s]
        assert [x['reason'] for x in km.parse_log(two['key_log']) if x['stream'] == s] == [int(n == int(key)) for n in range(4)]
    st = host(CUT, ['-key_frames', '1'], streams=2, env={'THOR_KEY_SHIFT': '1', 'THOR_STAGGER': '1'})
    assert st['bits'] == two['bits'] and st['rec'] == two['rec'] and st['key_log'] == two['key_log']
