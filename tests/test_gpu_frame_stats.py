"""Per-frame bits and distortion on the GPU (-m gpu): thorenc_hip prints the reference encoder's report byte for byte
(tests/golden/reports.json, recorded by gen_reports.py), thor_hip_frame_sse (the engine's k_frame_sse) equals numpy - up to a
12-bit 3840x2160 frame whose luma sum needs 47 bits - and the engine's per-frame log of 64 1080p streams, lock step and in two
staggered groups, matches the reference's frame lines and numpy on the downloaded reconstructions."""
import json
import os
import subprocess
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, golden_streams, golden_clip

pytestmark = pytest.mark.gpu
G = golden_streams()
REPORTS = json.load(open(os.path.join(GOLD, 'reports.json')))
BIG = json.load(open(os.path.join(GOLD, 'streams_big.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')


def _sse(a, b, w, h):
    a = a.astype(np.int64); b = b.astype(np.int64)
    d = (a - b) ** 2
    return [int(d[:w * h].sum()), int(d[w * h:w * h * 5 // 4].sum()), int(d[w * h * 5 // 4:].sum())]


@pytest.mark.parametrize('name', sorted(REPORTS))
def test_thorenc_hip_prints_the_reference_report(name):
    r = REPORTS[name]
    c = G[r['case']]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
        sf = os.path.join(d, 'stat.txt')
        cmd = [TOOL, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', str(c['w']), '-height', str(c['h']),
               '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit')] + c['extra'] + r['extra']
        if 'stat' in r:
            cmd += ['-stat', sf]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
        lines = out.splitlines(keepends=True)
        assert lines[-1].startswith('thorenc_hip: 1 stream(s)'), lines[-1]
        assert ''.join(lines[:-1]) == r['report']
        if 'stat' in r:
            assert open(sf).read() == r['stat']


@pytest.mark.parametrize('w,h', [(192, 128), (208, 120)])
@pytest.mark.parametrize('bits', [8, 10, 12])
def test_frame_sse_equals_numpy(w, h, bits):
    import thor_amd
    rng = np.random.default_rng(w + bits)
    T = np.uint16 if bits > 8 else np.uint8
    n = w * h * 3 // 2
    a = rng.integers(0, 1 << bits, n).astype(T)
    b = rng.integers(0, 1 << bits, n).astype(T)
    assert thor_amd.frame_sse(a, b, w, h, bits) == _sse(a, b, w, h)
    assert thor_amd.frame_sse(a, a, w, h, bits) == [0, 0, 0]


def test_frame_sse_needs_64_bit_sums():
    import thor_amd
    w, h = 3840, 2160
    a = np.zeros(w * h * 3 // 2, np.uint16)
    b = np.full_like(a, 4095)
    got = thor_amd.frame_sse(a, b, w, h, 12)
    assert got == [4095 * 4095 * w * h, 4095 * 4095 * w * h // 4, 4095 * 4095 * w * h // 4]
    assert got[0] > 1.39e14


def _big_frames(n):
    raw = np.frombuffer(golden_clip(BIG[n]['clip']), dtype=np.uint8)
    fsz = len(raw) // BIG[n]['n']
    return [raw[f * fsz:(f + 1) * fsz] for f in range(BIG[n]['n'])]


@pytest.mark.parametrize('staggered', [False, True])
def test_64_streams_frame_log_matches_reference_and_numpy(staggered):
    import thor_amd
    names = ['1080p_stream%02d_n6_q32' % s for s in range(64)]
    c = BIG[names[0]]
    w, h = int(c['w']), int(c['h'])
    clips = [_big_frames(n) for n in names]
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', c['cfg']), width=w, height=h, qp=int(c['qp']), f=30)
    with thor_amd.Encoder(p, 64) as enc:
        enc.set_frame_distortion(True)
        _, recs = enc.encode_clips(clips, staggered=staggered)
        for s, n in enumerate(names):
            log = enc.frame_stats(s)
            assert [[str(f['display_index']), f['type'], str(f['qp']), str(f['num_bits'])] for f in log] == BIG[n]['frames'], n
            for f in log:
                i = f['display_index']
                assert f['has_sse'] and f['sse'] == _sse(clips[s][i], recs[s][i].reshape(-1), w, h), (n, i)
            assert enc.report(s).splitlines()[1].split()[:4] == BIG[n]['frames'][0]


def test_distortion_off_keeps_bits_and_begin_sequence_empties_the_log():
    import thor_amd
    c = G['192x128_n3_q32']
    raw = np.frombuffer(golden_clip(c['clip']), dtype=np.uint8)
    fsz = 192 * 128 * 3 // 2
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', c['cfg']), width=192, height=128, qp=32, f=30)
    with thor_amd.Encoder(p, 1) as enc:
        enc.encode_clips([[raw[f * fsz:(f + 1) * fsz] for f in range(3)]])
        log = enc.frame_stats(0)
        assert [[str(f['display_index']), f['type'], str(f['qp']), str(f['num_bits'])] for f in log] == c['frames']
        assert all(f['sse'] == [0, 0, 0] and f['psnr'] == [0.0, 0.0, 0.0] and not f['has_sse'] for f in log)
        assert enc.report(0) == REPORTS['192x128_n3_q32_snrcalc0']['report']
        enc.begin_sequence(0, 3, 3, 6)
        assert enc.frame_stats(0) == []
