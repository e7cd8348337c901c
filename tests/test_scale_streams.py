"""A clip of another size through the whole encoder on the host (-m "not gpu"): the host simulation reads tests/golden/clip_192x128_6.yuv.gz with
-src_width 192 -src_height 128 and codes it at 96x64 (ratio 2) and at 128x88 (ratios 1.5 and 1.4545).  Bitstream and -rf file must be those the
reference encoder makes of the numpy model's resampling of that clip (tests/golden/streams_scale.json, recorded by gen_streams_scale.py; where the
reference binary is built it also runs live).  With the source size equal to the coded size the stream is the clip's existing golden."""
import json
import os
import subprocess
import tempfile
import pytest
from util import ROOT, GOLD, REF_ENC, golden_clip, md5
import scale_format as sf
from test_frame_layout import build_host_program

CASES = json.load(open(os.path.join(GOLD, 'streams_scale.json')))
STREAMS = json.load(open(os.path.join(GOLD, 'streams.json')))


def common(c, w, h):
    return ['-cf', os.path.join(ROOT, 'configs', c['cfg']), '-width', str(w), '-height', str(h), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30']


@pytest.mark.parametrize('pixfmt', ['i420', 'nv12'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_host_simulation_with_src_size_matches_the_reference(name, pixfmt):
    import frame_layout as fl
    c = CASES[name]
    clip = golden_clip(c['clip'])
    yuv = sf.scale_clip(clip, c['src_w'], c['src_h'], c['w'], c['h'], sf.BICUBIC, 1, c['n'])
    assert md5(yuv) == c['yuv_md5'], 'the model no longer resamples the clip as it did when the reference was recorded'
    if pixfmt == 'nv12':
        clip = fl.convert_clip(clip, fl.Geometry(c['src_w'], c['src_h'], 8, fl.UV), c['n'])
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(clip)
        subprocess.run([build_host_program('hostsim_mixed')] + common(c, c['w'], c['h']) + ['-if', os.path.join(d, 'in.yuv'), '-of', os.path.join(d, 'o.bit'),
                       '-rf', os.path.join(d, 'o.yuv'), '-src_width', str(c['src_w']), '-src_height', str(c['src_h']), '-pixfmt', pixfmt],
                       check=True, capture_output=True, text=True)
        bits, rec = open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.yuv'), 'rb').read()
        if pixfmt == 'nv12':   # -rf is in the -pixfmt layout, at the coded size
            rec = fl.convert_clip(rec, fl.Geometry(c['w'], c['h'], 8, fl.UV), c['n'], back=True)
        assert len(bits) == c['bit_bytes'] and md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
        assert len(rec) == c['rec_bytes'] and md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'
        if os.path.exists(REF_ENC):   # the reference itself, live, on the model's resampling
            open(os.path.join(d, 'scaled.yuv'), 'wb').write(yuv)
            subprocess.run([REF_ENC] + common(c, c['w'], c['h']) + ['-if', os.path.join(d, 'scaled.yuv'), '-of', os.path.join(d, 'r.bit'), '-rf', os.path.join(d, 'r.yuv')],
                           check=True, stdout=subprocess.DEVNULL)
            assert open(os.path.join(d, 'r.bit'), 'rb').read() == bits and open(os.path.join(d, 'r.yuv'), 'rb').read() == rec


@pytest.mark.parametrize('filt,site', [('bicubic', 'left'), ('bilinear', 'centre')])
def test_source_size_equal_to_the_coded_size_is_plain_staging(filt, site):
    g = STREAMS['192x128_n3_q32']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip('clip_192x128_6.yuv.gz'))
        subprocess.run([build_host_program('hostsim_mixed'), '-cf', os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), '-width', '192', '-height', '128',
                        '-qp', '32', '-n', '3', '-f', '30', '-if', os.path.join(d, 'in.yuv'), '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv'),
                        '-src_width', '192', '-src_height', '128', '-scale_filter', filt, '-scale_site', site], check=True, capture_output=True, text=True)
        assert md5(open(os.path.join(d, 'o.bit'), 'rb').read()) == g['bit_md5'] and md5(open(os.path.join(d, 'o.yuv'), 'rb').read()) == g['rec_md5']
