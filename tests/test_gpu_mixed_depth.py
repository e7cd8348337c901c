"""8- and 10-bit input coded at a higher internal bit depth, on the GPU (-m gpu): tools/thorenc_hip against the reference's streams,
reconstruction files and reports (tests/golden/streams_mixed.json, reports_mixed.json), two streams side by side in lock step and in two
staggered groups, the three frame-level kernels through their known-answer entry points on the vectors of tests/hostsim/unit_depth.cpp, the
Python Encoder staging uint8 frames from host and from device memory, and the reference's own front end over the drop-in seam.
Every encode is a fresh child process under its own time limit; after a child that was killed, timed out or died on a signal no further
child is started.  The case with 10-bit input compares its reconstruction in the half of the file the reference defines, and whole with the rounded
reconstruction of the reference's equal-depth run on the widened clip (tests/mixed_depth.py)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, REF_HIPENC, golden_clip, md5
from mixed_depth import defined_rec_bytes, depth_vectors, depth_expected, DEPTH_PAIRS, DEPTH_GEOMETRIES

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(GOLD, 'streams_mixed.json')))
REPORTS = json.load(open(os.path.join(GOLD, 'reports_mixed.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')
CASES = sorted(G)
_DEAD = []   # a child that did not end by itself: nothing more is started on the device


def run_child(cmd, limit_s, env_extra=None):
    """`cmd` in a child process under `timeout`; returns its stdout."""
    if _DEAD:
        pytest.fail('not started: an earlier GPU child process was killed or timed out (%s)' % _DEAD[0])
    env = dict(os.environ)
    env.update(env_extra or {})
    r = subprocess.run(['timeout', '-k', '10', str(limit_s)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _DEAD.append('exit status %d' % r.returncode)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def run_tool(c, streams=1, env_extra=None, exe=TOOL):
    """A Thorenc-compatible front end on case `c`; returns ([(bits, recon)] per stream, stdout)."""
    extra = list(c['extra'])
    if streams > 1:   # stream s codes frames [s * n, (s + 1) * n): the chunks of the reference's -skip runs
        i = extra.index('-skip')
        del extra[i:i + 2]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
        cmd = [exe, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'),
               '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30',
               '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + extra + (['-streams', str(streams)] if streams > 1 else [])
        out = run_child(cmd, 120, env_extra)
        names = [''] if streams == 1 else ['.%d' % s for s in range(streams)]
        return [(open(os.path.join(d, 'o.bit' + s), 'rb').read(), open(os.path.join(d, 'o.yuv' + s), 'rb').read()) for s in names], out


def check_files(c, bits, rec):
    assert len(bits) == c['bit_bytes'] and len(rec) == c['rec_bytes']
    assert md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    if 'rec_defined_md5' in c:
        assert md5(defined_rec_bytes(rec, c['w'], c['h'], c['n'], False)) == c['rec_defined_md5'], 'reconstruction differs from the reference'
        assert md5(rec) == c['rec_equal_depth_md5'], 'reconstruction differs from the rounded equal-depth run of the reference'
    else:
        assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@pytest.mark.parametrize('name', CASES)
def test_gpu_matches_reference_golden(name):
    """Bitstream, reconstruction at the input depth and report (16-bit samples have the one `std` build of the superblock kernel)."""
    c = G[name]
    ((bits, rec),), out = run_tool(c)
    check_files(c, bits, rec)
    rep = REPORTS[name]['report']
    assert out.startswith(rep) and out[len(rep):].startswith('thorenc_hip: '), 'report differs from the reference'


@pytest.mark.parametrize('stagger', ['0', '1'])
def test_two_streams_equal_two_reference_chunks(stagger):
    chunks = [G['192x128_n3_q32_skip%d_in8_bd10' % (3 * s)] for s in range(2)]
    files, out = run_tool(chunks[0], streams=2, env_extra={'THOR_STAGGER': stagger})
    for s, (bits, rec) in enumerate(files):
        check_files(chunks[s], bits, rec)
    assert out.startswith('stream 0\n' + REPORTS['192x128_n3_q32_skip0_in8_bd10']['report'] + 'stream 1\n' + REPORTS['192x128_n3_q32_skip3_in8_bd10']['report'])


@pytest.mark.parametrize('bd,inp', DEPTH_PAIRS)
@pytest.mark.parametrize('w,h', DEPTH_GEOMETRIES)
def test_kernels_match_the_reference_formulas(w, h, bd, inp):
    """k_depth_up, k_depth_down and k_frame_sse_depth through thor_hip_kat_depth_up / _down / thor_hip_frame_sse_depth, on the vectors the host
    program gets (full range: 0, the maximum, the values that saturate)."""
    import thor_amd
    vin, a, b = depth_vectors(w, h, bd, inp)
    up, down, sse = depth_expected(w, h, bd, inp, vin, a, b)
    assert np.array_equal(thor_amd.kat_depth_up(vin, w, h, bd, inp), up)
    got = thor_amd.kat_depth_down(a, w, h, bd, inp)
    assert got.dtype == vin.dtype and np.array_equal(got, down)
    assert thor_amd.frame_sse_depth(a, b, w, h, bd, inp) == sse


def test_frame_sse_depth_with_equal_depths_is_frame_sse():
    import thor_amd
    _, a, b = depth_vectors(40, 24, 10, 8)
    assert thor_amd.frame_sse_depth(a, b, 40, 24, 10, 10) == thor_amd.frame_sse(a, b, 40, 24, 10)


_ENCODER_CHILD = r'''
import hashlib, json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import thor_amd
from util import golden_clip
c = json.loads(%(case)r)
e = c['extra']
bd, inp = int(e[e.index('-bitdepth') + 1]), int(e[e.index('-input_bitdepth') + 1])
p = thor_amd.load_config(%(cfg)r, width=c['w'], height=c['h'], qp=c['qp'], f=30, bitdepth=bd, input_bitdepth=inp)
clip = np.frombuffer(golden_clip(c['clip']), dtype=np.uint8)
out = {}
for how in ('host', 'device'):
    with thor_amd.Encoder(p, 1) as enc:
        assert enc.dtype == np.uint8 and enc.sample_bytes == 1 and enc.frame_bytes == c['w'] * c['h'] * 3 // 2
        enc.set_frame_distortion(True)
        fsz, rec = enc.frame_bytes, b''
        dev = torch.from_numpy(clip[:c['n'] * fsz].copy()).cuda() if how == 'device' else None
        if dev is not None:
            torch.cuda.synchronize()
        for f in range(c['n']):
            if dev is None:
                enc.stage(0, f, clip[f * fsz:(f + 1) * fsz])
            else:
                enc.stage_device(0, f, dev.data_ptr() + f * fsz)
            enc.encode_staged([f])
            r = enc.recon(0)
            assert r.dtype == np.uint8 and r.size == fsz
            rec += r.tobytes()
        out[how] = {'bit_md5': hashlib.md5(enc.bitstream(0)).hexdigest(), 'rec_md5': hashlib.md5(rec).hexdigest(), 'report': enc.report(0),
                    'psnr': [['%%.4f' %% v for v in s['psnr']] for s in enc.frame_stats(0)]}
print(json.dumps(out))
'''


def test_python_encoder_stages_uint8_frames_from_host_and_device():
    name = '192x128_n4_q32_in8_bd10'
    c = G[name]
    code = _ENCODER_CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'case': json.dumps(c),
                             'cfg': os.path.join(ROOT, 'configs', c['cfg'])}
    out = json.loads(run_child([sys.executable, '-c', code], 180).splitlines()[-1])
    rep = REPORTS[name]['report']
    for how in ('host', 'device'):
        o = out[how]
        assert o['bit_md5'] == c['bit_md5'] and o['rec_md5'] == c['rec_md5'], how
        assert o['report'] == rep, how
        # the PSNR columns of the report's frame lines
        assert o['psnr'] == [l.split()[4:7] for l in rep.splitlines()[1:1 + c['n']]], how
    assert out['host'] == out['device']


@pytest.mark.parametrize('bd,inp', DEPTH_PAIRS)
def test_open_takes_the_new_pairs_and_sizes_frames_at_the_input_depth(bd, inp):
    import thor_amd
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), width=208, height=120, qp=32, f=30, bitdepth=bd, input_bitdepth=inp)
    with thor_amd.Encoder(p, 1) as enc:
        assert enc.frame_bytes == 208 * 120 * 3 // 2 * (2 if inp > 8 else 1) == thor_amd.lib().thor_hip_frame_bytes(enc.h)
        assert enc.dtype == (np.uint16 if inp > 8 else np.uint8)
    for bad in ((8, 10), (10, 12)):
        q = thor_amd.load_config(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), width=208, height=120, bitdepth=bad[0], input_bitdepth=bad[1])
        assert not thor_amd.lib().thor_hip_open(C.byref(q), 1, 0)


@pytest.mark.skipif(not os.path.exists(REF_HIPENC), reason='oracle/_ref/Thorenc_hip not in the snapshot')
def test_dropin_reference_front_end_on_our_library():
    """The reference's main() widens the input, calls encode_frame_hbd (the drop-in seam) with frames at the internal depth, and rounds the
    reconstruction back itself: the files are those of the all-reference encoder."""
    c = G['192x128_n4_q32_in8_bd10']
    ((bits, rec),), _ = run_tool(c, exe=REF_HIPENC)
    check_files(c, bits, rec)
