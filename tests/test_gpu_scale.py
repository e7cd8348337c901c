"""Staging frames of another size on the GPU (-m gpu): k_scale_in through its known-answer entry point against the numpy model of
tests/scale_format.py, exactly - the host cases, the two ratio limits (8 down: 33 taps; 8 up: one source sample feeds eight), and destinations
that span several of the kernel's 64 x 32 tiles in both directions with partial last tiles; an encoder fed the 192x128 clip at 96x64 from host and
from device memory against the same encoder fed the model's resampled frames; tools/thorenc_hip with -src_width / -src_height; and the argument
checks of the new entries.  Every encode is a fresh child process under its own time limit; after a child that was killed, timed out or died on a
signal no further child is started."""
import json
import os
import subprocess
import sys
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, golden_clip, md5
import frame_layout as fl
import scale_format as sf

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(GOLD, 'streams_scale.json')))
STREAMS = json.load(open(os.path.join(GOLD, 'streams.json')))
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


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------

# the host cases; 128 -> 16 and 16 -> 128 (ratio 8 both ways); and with tiles of 64 x 32 destination samples: 200x120 is 4 x 4 luma tiles (last 8
# wide, 24 high) and 2 x 2 chroma tiles (last 36 x 28); 272x200 from 176x144 is 5 x 7 luma tiles (last 16 x 8) going up
SIZES = sf.SIZES + [(128, 128, 16, 16), (16, 16, 128, 128), (176, 144, 272, 200)]


def check(sw, sh, w, h, bd, n, g, skew, kind, filt, site):
    import thor_amd
    frame = sf.content(kind, sw, sh, n)
    src = fl.skewed(g.bytes, skew)      # the device copy keeps this offset from a 16-byte boundary
    fl.pack(frame, g, into=src)
    lay = thor_amd.FrameLayout(g.chroma, g.msb, g.fields['pitch_y'], g.fields['pitch_c'], 0, 0)
    got = thor_amd.kat_scale_in(src, thor_amd.Scale(sw, sh, filt, site), w, h, n, bd, lay)
    want = sf.expect_in(src, g, w, h, filt, site, n, bd)
    assert got.dtype == want.dtype and np.array_equal(got, want), ((sw, sh, w, h), kind, filt, site, np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize('bd,n', sf.DEPTHS)
@pytest.mark.parametrize('sw,sh,w,h', SIZES)
def test_kernel_matches_the_model(sw, sh, w, h, bd, n):
    for name, g, skew in sf.source_layouts(sw, sh, n):
        for kind in sf.CONTENTS:
            for filt, site in ((sf.BICUBIC, 1), (sf.BILINEAR, 0)) if kind != 'noise' or name != 'planar' else ((1, 1), (1, 0), (0, 1), (0, 0)):
                check(sw, sh, w, h, bd, n, g, skew, kind, filt, site)


def test_kernel_default_layout_is_packed_planar():
    import thor_amd
    frame = sf.content('noise', 48, 32, 8)
    got = thor_amd.kat_scale_in(np.ascontiguousarray(frame), thor_amd.Scale(48, 32), 16, 16, 8, 8)
    assert np.array_equal(got, sf.scale_frame(frame, 48, 32, 16, 16, sf.BICUBIC, 1, 8))


# ---- whole encodes --------------------------------------------------------------------------------------------------------------------------------

_CHILD = r'''
import ctypes as C, hashlib, json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import thor_amd
from util import golden_clip
import frame_layout as fl
import scale_format as sf
c = json.loads(%(case)r)
sw, sh, w, h, n = c['src_w'], c['src_h'], c['w'], c['h'], c['n']
p = thor_amd.load_config(%(cfg)r, width=w, height=h, qp=c['qp'], f=30)
clip = np.frombuffer(golden_clip(c['clip']), dtype=np.uint8)
fsz = sw * sh * 3 // 2
frames = [clip[f * fsz:(f + 1) * fsz] for f in range(n)]
nv12 = fl.Geometry(sw, sh, 8, fl.UV, 0, sw + 64, sw + 64)        # the device frames: NV12 with a pitch wider than the row
out = {}
with thor_amd.Encoder(p, 3) as enc:
    sc = thor_amd.Scale(sw, sh)
    lay = thor_amd.FrameLayout.nv12(pitch=sw + 64)
    assert enc.scale_bytes(sc) == fsz and enc.scale_bytes(sc, lay) == nv12.bytes
    dev = torch.from_numpy(np.stack([fl.pack(fr, nv12) for fr in frames])).cuda()
    torch.cuda.synchronize()
    rec = [b'', b'', b'']
    for f in range(n):
        enc.stage(0, f, sf.scale_frame(frames[f], sw, sh, w, h, sf.BICUBIC, 1, 8))      # the model's resampling, staged as it is
        enc.stage_scaled(1, f, frames[f], sc)
        enc.stage_scaled_device(2, f, dev[f].data_ptr(), sc, lay)
        if f == 1:   # a refused plan returns 1 and leaves the slot as it was: the encode below still codes the frame staged above
            bad = thor_amd.Scale(sw + 1, sh)
            assert thor_amd.lib().thor_hip_stage_frame_scaled(enc.h, 1, f, frames[f].ctypes.data_as(C.c_void_p), C.byref(bad), None, 0) == 1
            far = thor_amd.Scale(w * 8 + 2, sh)
            assert thor_amd.lib().thor_hip_stage_frame_scaled(enc.h, 2, f, C.c_void_p(dev[f].data_ptr()), C.byref(far), C.byref(lay), 1) == 1
            assert thor_amd.lib().thor_hip_stage_frame_scaled(enc.h, 3, f, frames[f].ctypes.data_as(C.c_void_p), C.byref(sc), None, 0) == 1   # no such stream
            assert thor_amd.lib().thor_hip_stage_frame_scaled(enc.h, 1, f, None, C.byref(sc), None, 0) == 1
        enc.encode_staged([f, f, f])
        for s in range(3):
            rec[s] += enc.recon(s).tobytes()
    out['bit_md5'] = [hashlib.md5(enc.bitstream(s)).hexdigest() for s in range(3)]
    out['rec_md5'] = [hashlib.md5(r).hexdigest() for r in rec]
print(json.dumps(out))
'''


@pytest.mark.parametrize('name', ['192x128_to_96x64_n3_q32'])
def test_scaled_staging_from_host_and_device_memory_equals_staging_the_model(name):
    """Stream 0 stages the numpy-resampled frames with Encoder.stage, stream 1 the 192x128 frames with stage_scaled, stream 2 NV12 frames in device
    memory with stage_scaled_device: the three bitstreams and reconstructions are equal, and equal to the reference's."""
    c = CASES[name]
    code = _CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'case': json.dumps(c), 'cfg': os.path.join(ROOT, 'configs', c['cfg'])}
    o = json.loads(run_child([sys.executable, '-c', code], 180).splitlines()[-1])
    assert o['bit_md5'] == [c['bit_md5']] * 3 and o['rec_md5'] == [c['rec_md5']] * 3


_SAME = r'''
import hashlib, json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import thor_amd
from util import golden_clip
w, h, n = 192, 128, 3
p = thor_amd.load_config(%(cfg)r, width=w, height=h, qp=32, f=30)
clip = np.frombuffer(golden_clip('clip_192x128_6.yuv.gz'), dtype=np.uint8)
fsz = w * h * 3 // 2
with thor_amd.Encoder(p, 2) as enc:
    rec = [b'', b'']
    for f in range(n):
        enc.stage(0, f, clip[f * fsz:(f + 1) * fsz])
        enc.stage_scaled(1, f, clip[f * fsz:(f + 1) * fsz], thor_amd.Scale(w, h, thor_amd.binding.SCALE_BILINEAR if f & 1 else thor_amd.binding.SCALE_BICUBIC, f & 1))
        enc.encode_staged([f, f])
        for s in range(2):
            rec[s] += enc.recon(s).tobytes()
    print(json.dumps({'bit_md5': [hashlib.md5(enc.bitstream(s)).hexdigest() for s in range(2)], 'rec_md5': [hashlib.md5(r).hexdigest() for r in rec]}))
'''


def test_source_size_equal_to_the_coded_size_equals_plain_staging():
    g = STREAMS['192x128_n3_q32']
    code = _SAME % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'cfg': os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')}
    o = json.loads(run_child([sys.executable, '-c', code], 180).splitlines()[-1])
    assert o['bit_md5'] == [g['bit_md5']] * 2 and o['rec_md5'] == [g['rec_md5']] * 2


def test_command_line_tool_with_src_size_and_pixfmt_nv12():
    c = CASES['192x128_to_96x64_n3_q32']
    clip = fl.convert_clip(golden_clip(c['clip']), fl.Geometry(c['src_w'], c['src_h'], 8, fl.UV), c['n'])
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.nv12'), 'wb').write(clip)
        run_child([TOOL, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.nv12'), '-width', str(c['w']), '-height', str(c['h']),
                   '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.nv12'),
                   '-src_width', str(c['src_w']), '-src_height', str(c['src_h']), '-pixfmt', 'nv12'], 120)
        bits, rec = open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.nv12'), 'rb').read()
    rec = fl.convert_clip(rec, fl.Geometry(c['w'], c['h'], 8, fl.UV), c['n'], back=True)
    assert len(bits) == c['bit_bytes'] and md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'
