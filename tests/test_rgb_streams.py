"""An RGB clip through the whole encoder on the host (-m "not gpu"): the host simulation reads tests/golden/clip_rgb_80x48_4.bgra.gz with -pixfmt
bgra and must produce the bitstream the reference encoder produced from the numpy model's conversion of that clip (tests/golden/streams_rgb.json,
recorded by gen_streams_rgb.py); its -rf file, which is BGRA, must be the model's inverse of the reference's reconstruction.  Where the reference
binary is built, it runs live as well."""
import json
import os
import subprocess
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, REF_ENC, golden_clip, md5
import rgb_format as rf
from test_frame_layout import build_host_program

CASES = json.load(open(os.path.join(GOLD, 'streams_rgb.json')))


def test_clip_is_the_seeded_generator():
    c = next(iter(CASES.values()))
    clip = golden_clip(c['clip'])
    assert md5(clip) == c['clip_md5'] and clip == rf.make_clip(c['w'], c['h'], c['n'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_simulation_with_pixfmt_bgra_matches_the_reference(name):
    c = CASES[name]
    clip = golden_clip(c['clip'])
    f = rf.Format(c['w'], c['h'], rf.BGRA)
    fsz = c['w'] * c['h'] * 3 // 2
    yuv = b''.join(rf.to_yuv(*rf.unpack(clip[i * f.bytes:(i + 1) * f.bytes], f), f, 8).tobytes() for i in range(c['n']))
    assert md5(yuv) == c['yuv_md5'], 'the model no longer converts the clip as it did when the reference was recorded'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.bgra'), 'wb').write(clip)
        common = ['-cf', os.path.join(ROOT, 'configs', c['cfg']), '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30']
        subprocess.run([build_host_program('hostsim_mixed')] + common + ['-if', os.path.join(d, 'in.bgra'), '-of', os.path.join(d, 'o.bit'),
                       '-rf', os.path.join(d, 'o.bgra'), '-pixfmt', 'bgra'] + c['extra'], check=True, capture_output=True, text=True)
        bits, rec_rgb = open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.bgra'), 'rb').read()
        assert len(bits) == c['bit_bytes'] and md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
        assert len(rec_rgb) == c['n'] * f.bytes and md5(rec_rgb) == c['rec_rgb_md5'], 'the RGB -rf file is not the inverse of the reference reconstruction'
        if os.path.exists(REF_ENC):   # the reference itself, live, on the model's conversion
            open(os.path.join(d, 'in.yuv'), 'wb').write(yuv)
            subprocess.run([REF_ENC] + common + ['-if', os.path.join(d, 'in.yuv'), '-of', os.path.join(d, 'r.bit'), '-rf', os.path.join(d, 'r.yuv')] + c['extra'],
                           check=True, stdout=subprocess.DEVNULL)
            assert open(os.path.join(d, 'r.bit'), 'rb').read() == bits
            rec = np.frombuffer(open(os.path.join(d, 'r.yuv'), 'rb').read(), dtype=np.uint8)
            want = b''.join(rf.pack(*rf.to_rgb(rec[i * fsz:(i + 1) * fsz], f, 8), f).tobytes() for i in range(c['n']))
            assert want == rec_rgb
