"""Frames in NV12 / NV21 / P010 layouts with a row pitch, on the GPU (-m gpu): k_layout_in and k_layout_out through their known-answer entry
points against numpy over the grid of tests/frame_layout.py (every pitch, base on and off a 16-byte boundary, canaries in every byte the kernel
must not write); whole encodes staged from a torch tensor that holds NV12 at pitch 256 (P010 at pitch 512) and fetched into one, and through
host-side staging; two streams of one encoder, one staged planar and one NV12; tools/thorenc_hip -pixfmt nv12.  Every comparison is exact.
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
import frame_layout as fl

pytestmark = pytest.mark.gpu
STREAMS = json.load(open(os.path.join(GOLD, 'streams.json')))
MIXED = json.load(open(os.path.join(GOLD, 'streams_mixed.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')
_DEAD = []   # a child that did not end by itself: nothing more is started on the device


def run_child(cmd, limit_s):
    """`cmd` in a child process under `timeout`; returns its stdout."""
    if _DEAD:
        pytest.fail('not started: an earlier GPU child process was killed or timed out (%s)' % _DEAD[0])
    r = subprocess.run(['timeout', '-k', '10', str(limit_s)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _DEAD.append('exit status %d' % r.returncode)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('layout', fl.LAYOUTS, ids=fl.layout_id)
@pytest.mark.parametrize('w,h', fl.SIZES)
def test_kernels_match_numpy(w, h, layout):
    """In: the planes equal numpy's.  Out: every sample of the picture equals numpy's and every padding, gap and guard byte is still the canary."""
    import thor_amd
    chroma, msb, inp, bd, _ = layout
    fin, rec = fl.vectors(w, h, inp, bd)
    want_planes = fl.expect_in(fin, inp, bd)
    for pitch in fl.PITCHES:
        g = fl.case_geometry(w, h, layout, pitch)
        lay = thor_amd.FrameLayout(**g.fields)
        want_dst = np.full(g.bytes + fl.GUARD, fl.CANARY, dtype=np.uint8)
        fl.pack(fl.expect_out(rec, inp, bd), g, into=want_dst[:g.bytes])
        for skew in fl.SKEWS:
            src = fl.skewed(g.bytes, skew * g.B)
            fl.pack(fin, g, into=src)
            got = thor_amd.kat_layout_in(src, lay, w, h, inp, bd)
            assert got.dtype == want_planes.dtype and np.array_equal(got, want_planes), (pitch, skew)
            dst = fl.skewed(g.bytes + fl.GUARD, skew * g.B)
            thor_amd.kat_layout_out(rec, lay, w, h, inp, bd, dst)
            assert np.array_equal(dst, want_dst), (pitch, skew, np.flatnonzero(dst != want_dst)[:8])


# ---- whole encodes ------------------------------------------------------------------------------------------------------------------------------

_CHILD = r'''
import hashlib, json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import thor_amd
from util import golden_clip
import frame_layout as fl
c, how, chroma, msb, pitch = json.loads(%(case)r), %(how)r, %(chroma)d, %(msb)d, %(pitch)d
e = c['extra']
bd = int(e[e.index('-bitdepth') + 1]) if '-bitdepth' in e else 8
inp = int(e[e.index('-input_bitdepth') + 1]) if '-input_bitdepth' in e else 8
w, h, n = c['w'], c['h'], c['n']
p = thor_amd.load_config(%(cfg)r, width=w, height=h, qp=c['qp'], f=30, bitdepth=bd, input_bitdepth=inp)
g = fl.Geometry(w, h, inp, chroma, msb, pitch, pitch)
lay = thor_amd.FrameLayout(**g.fields)
clip = np.frombuffer(golden_clip(c['clip']), dtype=np.uint8)
fsz = w * h * 3 // 2 * g.B
frames = [clip[f * fsz:(f + 1) * fsz] for f in range(n)]
packed = [fl.pack(fr.view(g.dtype), g) for fr in frames]      # numpy: the clip in the layout, 0xA5 in the padding
out = {}
if how == 'two_streams':   # stream 0 through the old planar call, stream 1 through the layout, frame by frame
    with thor_amd.Encoder(p, 2) as enc:
        for f in range(n):
            enc.stage(0, f, frames[f])
            enc.stage(1, f, packed[f], layout=lay)
            enc.encode_staged([f, f])
        out['bit_md5'] = [hashlib.md5(enc.bitstream(s)).hexdigest() for s in range(2)]
else:
    with thor_amd.Encoder(p, 1) as enc:
        assert enc.layout_bytes(lay) == g.bytes
        rec_planar, rec_layout = b'', b''
        if how == 'device':
            dev = torch.from_numpy(np.stack(packed)).cuda()
            back = torch.full((g.bytes + fl.GUARD,), fl.CANARY, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()
        for f in range(n):
            if how == 'device':
                enc.stage_device(0, f, dev[f].data_ptr(), lay)
            else:
                enc.stage(0, f, packed[f], layout=lay)
            enc.encode_staged([f])
            planar = enc.recon(0)
            if how == 'device':
                enc.recon_device(0, back.data_ptr(), lay)
                got = back.cpu().numpy()
                want = np.full(g.bytes + fl.GUARD, fl.CANARY, dtype=np.uint8)   # padding and guard untouched over all frames
                fl.pack(planar.view(g.dtype), g, into=want[:g.bytes])
                assert np.array_equal(got, want), 'frame %%d: recon_device differs from recon()' %% f
                got = got[:g.bytes]
            else:
                got = enc.recon(0, layout=lay)
                want = np.zeros(g.bytes, dtype=np.uint8)
                fl.pack(planar.view(g.dtype), g, into=want)
                assert np.array_equal(got, want), 'frame %%d: recon(layout) differs from recon()' %% f
            rec_planar += planar.tobytes()
            rec_layout += fl.unpack(got, g).tobytes()
        out = {'bit_md5': hashlib.md5(enc.bitstream(0)).hexdigest(), 'rec_md5': hashlib.md5(rec_planar).hexdigest(),
               'rec_layout_md5': hashlib.md5(rec_layout).hexdigest()}
print(json.dumps(out))
'''


def encoder_child(c, how, chroma, msb, pitch):
    code = _CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'case': json.dumps(c), 'how': how, 'chroma': chroma, 'msb': msb,
                     'pitch': pitch, 'cfg': os.path.join(ROOT, 'configs', c['cfg'])}
    return json.loads(run_child([sys.executable, '-c', code], 180).splitlines()[-1])


ENCODES = [('208x120_n4_q32', STREAMS, 'device', fl.UV, 0, 256), ('192x128_n4_q32_10bit', STREAMS, 'device', fl.UV, 1, 512),
           ('192x128_n4_q32_in8_bd10', MIXED, 'host', fl.UV, 0, 256)]


@pytest.mark.parametrize('name,table,how,chroma,msb,pitch', ENCODES, ids=['%s-%s' % (e[0], e[2]) for e in ENCODES])
def test_encoder_stages_and_fetches_frames_in_a_layout(name, table, how, chroma, msb, pitch):
    """stage_device from a torch tensor holding NV12 at pitch 256 (P010 at pitch 512) and recon_device into one - or host-side stage(layout=) and
    recon(layout=): the bitstream is the golden, the fetched reconstruction converted back equals the planar recon() and the recorded digest."""
    c = table[name]
    o = encoder_child(c, how, chroma, msb, pitch)
    assert o['bit_md5'] == c['bit_md5'], 'bitstream differs from the reference'
    assert o['rec_md5'] == c['rec_md5'] and o['rec_layout_md5'] == c['rec_md5'], 'reconstruction differs from the reference'


def test_two_streams_one_planar_one_nv12():
    """Stream 0 staged with the old planar call (input_bitdepth < bitdepth: through the engine's packed staging frame), stream 1 from NV12 through
    the layout staging buffer, same clip, frame by frame: neither path disturbs the other."""
    c = MIXED['192x128_n4_q32_in8_bd10']
    o = encoder_child(c, 'two_streams', fl.UV, 0, 256)
    assert o['bit_md5'] == [c['bit_md5'], c['bit_md5']]


def test_command_line_tool_with_pixfmt_nv12():
    c = STREAMS['208x120_n4_q32']
    g = fl.Geometry(c['w'], c['h'], 8, fl.UV)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(fl.convert_clip(golden_clip(c['clip']), g, c['n']))
        run_child([TOOL, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', str(c['w']), '-height', str(c['h']),
                   '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv'),
                   '-pixfmt', 'nv12'] + c['extra'], 120)
        bits, rec = open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.yuv'), 'rb').read()
    assert len(bits) == c['bit_bytes'] and md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(fl.convert_clip(rec, g, c['n'], back=True)) == c['rec_md5'], 'reconstruction differs from the reference'
