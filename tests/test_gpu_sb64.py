"""64x64 superblocks on the GPU (-m gpu): tools/thorenc_hip with -log2_sb_size 6 against the hashes recorded from the reference encoder
(tests/golden/streams_sb64.json, streams_big_sb64.json) - every small case, the 8-bit ones through each of the three builds of the
superblock kernel, four streams side by side in lock step and in two staggered groups, and one 3840x2160 case (a 60x34 grid).
Every encode is a fresh child process under its own time limit; after a child that was killed, timed out or died on a signal no further
child is started.  Sizes 5 and 8 are refused by the parameter functions and by thor_hip_open before anything is launched."""
import ctypes as C
import json
import os
import subprocess
import tempfile
import pytest
from util import ROOT, GOLD, golden_clip, md5

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(GOLD, 'streams_sb64.json')))
BIG = json.load(open(os.path.join(GOLD, 'streams_big_sb64.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')
SMALL = [n for n in sorted(G) if '_skip' not in n]
_DEAD = []   # a child that did not end by itself: nothing more is started on the device


def _kernels(name):
    return ['std'] if '10bit' in name else ['std', 'lat', 'wide']   # 16-bit samples have one kernel


def run_tool(c, clip, limit_s, streams=1, env_extra=None, skip_opts=True):
    """thorenc_hip on case `c` in a child process under `timeout`; returns [(bits, recon)] per stream."""
    if _DEAD:
        pytest.fail('not started: an earlier GPU child process was killed or timed out (%s)' % _DEAD[0])
    extra = list(c['extra'])
    if not skip_opts and '-skip' in extra:
        i = extra.index('-skip')
        del extra[i:i + 2]
    env = dict(os.environ)
    env.update(env_extra or {})
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(clip)
        cmd = ['timeout', '-k', '10', str(limit_s), TOOL, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'),
               '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30',
               '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + extra + (['-streams', str(streams)] if streams > 1 else [])
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=env)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            _DEAD.append('exit status %d' % r.returncode)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        names = [''] if streams == 1 else ['.%d' % s for s in range(streams)]
        return [(open(os.path.join(d, 'o.bit' + s), 'rb').read(), open(os.path.join(d, 'o.yuv' + s), 'rb').read()) for s in names]


def test_sizes_5_and_8_are_refused_before_any_launch():
    import thor_amd
    cfg = os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')
    for bad in (5, 8):
        p = thor_amd.load_config(cfg, width=208, height=120, qp=32, f=30)
        assert thor_amd.lib().thor_hip_params_set(C.byref(p), b'-log2_sb_size', str(bad).encode()) == 2
        p.log2_sb_size = bad
        assert not thor_amd.lib().thor_hip_open(C.byref(p), 1, 0), bad


@pytest.mark.parametrize('name,kernel', [(n, k) for n in SMALL for k in _kernels(n)])
def test_gpu_matches_reference_golden(name, kernel):
    c = G[name]
    (bits, rec), = run_tool(c, golden_clip(c['clip']), 120, env_extra={'THOR_HIP_KERNEL': kernel})
    assert len(bits) == c['bit_bytes']
    assert md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@pytest.mark.parametrize('stagger', ['0', '1'])
def test_four_streams_equal_four_reference_chunks(stagger):
    """Stream s of a four-stream run over the 12-frame 192x128 clip == the reference run with -skip 3*s -n 3, in lock step and with the
    streams in two groups half a frame apart (launches over ranges of anti-diagonals of the 3x2 grid)."""
    chunks = [G['192x128_n3_q32_skip%d_sb64' % (3 * s)] for s in range(4)]
    out = run_tool(chunks[0], golden_clip(chunks[0]['clip']), 120, streams=4, env_extra={'THOR_STAGGER': stagger}, skip_opts=False)
    for s, (bits, rec) in enumerate(out):
        assert md5(bits) == chunks[s]['bit_md5'] and md5(rec) == chunks[s]['rec_md5'], s


def test_3840x2160_matches_reference_golden():
    """60x34 superblocks: grid rows longer than the chip has compute units per stream; the library picks the build itself."""
    c = BIG['4k_ldb_n3_q32_sb64']
    (bits, rec), = run_tool(c, golden_clip(c['clip']), 240)
    assert len(bits) == c['bit_bytes']
    assert md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'
