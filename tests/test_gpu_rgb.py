"""RGB frames on the GPU (-m gpu): k_rgb_in and k_rgb_out through their known-answer entry points against the numpy model of tests/rgb_format.py,
exactly, on the shapes that can go wrong (tails, unaligned rows and bases, the byte path of three-sample pixels, a plane stride larger than a plane;
canaries in every byte the kernel must not write); one encoder with two streams of the RGB clip, one staged from host memory and one from a torch
tensor with a pitch wider than the row, against the reference's recorded bitstream (tests/golden/streams_rgb.json); tools/thorenc_hip -pixfmt bgra;
and a planar and an RGB stream side by side in the three builds of the superblock kernel.
Every encode is a fresh child process under its own time limit; after a child that was killed, timed out or died on a signal no further child
is started."""
import json
import os
import subprocess
import sys
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, golden_clip, md5
import rgb_format as rf

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(GOLD, 'streams_rgb.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')
_DEAD = []   # a child that did not end by itself: nothing more is started on the device


def run_child(cmd, limit_s, env=None):
    """`cmd` in a child process under `timeout`; returns its stdout."""
    if _DEAD:
        pytest.fail('not started: an earlier GPU child process was killed or timed out (%s)' % _DEAD[0])
    r = subprocess.run(['timeout', '-k', '10', str(limit_s)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _DEAD.append('exit status %d' % r.returncode)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


# ---- the kernels --------------------------------------------------------------------------------------------------------------------------------

FORMATS = [(rf.RGBA, 8, 0), (rf.BGRA, 8, 0), (rf.ARGB, 8, 0), (rf.ABGR, 8, 0), (rf.BGR, 8, 0), (rf.RGBA, 10, 1), (rf.RGBA, 16, 0), (rf.PLANAR, 8, 0)]


@pytest.mark.parametrize('bd,n', [(8, 8), (10, 8), (12, 10)])
@pytest.mark.parametrize('order,depth,msb', FORMATS, ids=['%s%d' % (rf.ORDER_NAMES[f[0]], f[1]) for f in FORMATS])
def test_kernels_match_the_model(order, depth, msb, bd, n):
    """In: the planes equal the model's.  Out: every sample of the picture equals the model's and every padding, gap and guard byte is still the
    canary.  Both sitings; matrix and range rotate with the case."""
    import thor_amd
    for site in (0, 1):
        k = order + depth + n + site
        matrix, full = k % 3, (k // 3) % 2
        for shape in rf.shapes(order, depth):
            f, skew = rf.shaped(order, depth, msb, matrix, full, site, shape)
            fmt = thor_amd.RgbFormat(**f.fields)
            src = rf.skewed(f.bytes, skew)
            rf.pack(*rf.random_rgb(f, 7 + k), f, into=src)
            got = thor_amd.kat_rgb_in(src, fmt, f.w, f.h, n, bd)
            want = rf.expect_in(src, f, n, bd)
            assert got.dtype == want.dtype and np.array_equal(got, want), (rf.format_id(f), shape, np.flatnonzero(got != want)[:8])
            rec = rf.random_rec(f.w, f.h, bd, 9 + k)
            dst = rf.skewed(f.bytes + rf.GUARD, skew)
            want_dst = rf.expect_out(rec, f, n, bd, np.full(f.bytes + rf.GUARD, rf.CANARY, dtype=np.uint8))
            thor_amd.kat_rgb_out(rec, fmt, f.w, f.h, n, bd, dst)
            assert np.array_equal(dst, want_dst), (rf.format_id(f), shape, np.flatnonzero(dst != want_dst)[:8])


# ---- whole encodes ------------------------------------------------------------------------------------------------------------------------------

_CHILD = r'''
import hashlib, json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import thor_amd
from util import golden_clip
import rgb_format as rf
c, how = json.loads(%(case)r), %(how)r
e = c['extra']
bd = int(e[e.index('-bitdepth') + 1]) if '-bitdepth' in e else 8
w, h, n = c['w'], c['h'], c['n']
p = thor_amd.load_config(%(cfg)r, width=w, height=h, qp=c['qp'], f=30, bitdepth=bd, input_bitdepth=8)
tight = rf.Format(w, h, rf.BGRA)
wide = rf.Format(w, h, rf.BGRA, pitch=tight.row + 64)          # the device frames: a pitch wider than the row
clip = np.frombuffer(golden_clip(c['clip']), dtype=np.uint8)
frames = [clip[f * tight.bytes:(f + 1) * tight.bytes] for f in range(n)]
out = {}
with thor_amd.Encoder(p, 2) as enc:
    ft, fw = thor_amd.RgbFormat(**tight.fields), thor_amd.RgbFormat(**wide.fields)
    assert enc.rgb_bytes(ft) == tight.bytes and enc.rgb_bytes(fw) == wide.bytes
    if how == 'rgb_and_rgb':   # stream 0 from host memory, stream 1 from a torch tensor in device memory
        dev = torch.from_numpy(np.stack([rf.pack(*rf.unpack(fr, tight), wide) for fr in frames])).cuda()
        back = torch.full((wide.bytes + rf.GUARD,), rf.CANARY, dtype=torch.uint8, device='cuda')
        torch.cuda.synchronize()
    for f in range(n):
        if how == 'rgb_and_rgb':
            enc.stage_rgb(0, f, frames[f], ft)
            enc.stage_rgb_device(1, f, dev[f].data_ptr(), fw)
        else:                  # stream 0 staged as planar Y'CbCr (the model's conversion), stream 1 as RGB
            enc.stage(0, f, rf.to_yuv(*rf.unpack(frames[f], tight), tight, 8))
            enc.stage_rgb(1, f, frames[f], ft)
        enc.encode_staged([f, f])
        if how == 'rgb_and_rgb':
            for s in range(2):
                planar = enc.recon(s)
                want = rf.pack(*rf.to_rgb(planar, tight, 8), tight, into=np.zeros(tight.bytes, dtype=np.uint8))
                assert np.array_equal(enc.recon_rgb(s, ft), want), 'frame %%d stream %%d: recon_rgb is not the inverse of recon()' %% (f, s)
            enc.recon_rgb_device(1, back.data_ptr(), fw)
            want = np.full(wide.bytes + rf.GUARD, rf.CANARY, dtype=np.uint8)     # padding and guard untouched over all frames
            rf.pack(*rf.to_rgb(enc.recon(1), wide, 8), wide, into=want[:wide.bytes])
            assert np.array_equal(back.cpu().numpy(), want), 'frame %%d: recon_rgb_device differs' %% f
    out['bit_md5'] = [hashlib.md5(enc.bitstream(s)).hexdigest() for s in range(2)]
print(json.dumps(out))
'''


def encoder_child(c, how, env=None):
    code = _CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'case': json.dumps(c), 'how': how, 'cfg': os.path.join(ROOT, 'configs', c['cfg'])}
    return json.loads(run_child([sys.executable, '-c', code], 180, env).splitlines()[-1])


@pytest.mark.parametrize('name', sorted(CASES))
def test_two_streams_staged_from_host_and_from_device_memory(name):
    """stage_rgb from host memory and stage_rgb_device from a torch tensor whose pitch is wider than the row: both bitstreams are the reference's;
    recon_rgb and recon_rgb_device are the model's inverse of recon(), row padding and guard untouched."""
    c = CASES[name]
    o = encoder_child(c, 'rgb_and_rgb')
    assert o['bit_md5'] == [c['bit_md5'], c['bit_md5']], 'bitstream differs from the reference'


@pytest.mark.parametrize('build', ['std', 'lat', 'wide'])
def test_planar_and_rgb_streams_agree_in_every_build_of_the_superblock_kernel(build):
    c = CASES['80x48_n4_q32_bgra']
    o = encoder_child(c, 'planar_and_rgb', dict(os.environ, THOR_HIP_KERNEL=build))
    assert o['bit_md5'][0] == o['bit_md5'][1] == c['bit_md5']


def test_command_line_tool_with_pixfmt_bgra():
    c = CASES['80x48_n4_q32_bgra']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.bgra'), 'wb').write(golden_clip(c['clip']))
        run_child([TOOL, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.bgra'), '-width', str(c['w']), '-height', str(c['h']),
                   '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.bgra'),
                   '-pixfmt', 'bgra'] + c['extra'], 120)
        bits, rec = open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.bgra'), 'rb').read()
    assert len(bits) == c['bit_bytes'] and md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_rgb_md5'], 'the RGB -rf file is not the inverse of the reference reconstruction'
