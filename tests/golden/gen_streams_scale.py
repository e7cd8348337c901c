#!/usr/bin/env python3
"""Record what the reference encoder (oracle/_ref/Thorenc) makes of a resampled clip: tests/golden/clip_192x128_6.yuv.gz is resampled with the numpy
model of tests/scale_format.py (bicubic, left-sited chroma - the defaults of -src_width / -src_height) to 96x64 and to 128x88 and encoded.  Recorded:
md5 of the resampled input, of the bitstream and of the reconstruction.  tests/test_scale_streams.py and tests/test_gpu_scale.py feed the 192x128 clip
itself to this project and compare.  Run in the build container after `make -C oracle`."""
import gzip, hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G = os.path.join(ROOT, 'tests', 'golden')
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import scale_format as sf  # noqa: E402

CLIP, SW, SH, N, QP = 'clip_192x128_6.yuv.gz', 192, 128, 3, 32
CFG = 'ldb_high_efficiency.cfg'
CASES = {'192x128_to_96x64_n3_q32': (96, 64), '192x128_to_128x88_n3_q32': (128, 88)}

if __name__ == '__main__':
    clip = gzip.open(os.path.join(G, CLIP)).read()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, (w, h) in CASES.items():
            yuv = sf.scale_clip(clip, SW, SH, w, h, sf.BICUBIC, 1, N)
            open(os.path.join(d, 'in.yuv'), 'wb').write(yuv)
            subprocess.run([os.path.join(ROOT, 'oracle/_ref/Thorenc'), '-cf', os.path.join(ROOT, 'configs', CFG), '-if', os.path.join(d, 'in.yuv'),
                            '-width', str(w), '-height', str(h), '-qp', str(QP), '-n', str(N), '-f', '30', '-of', os.path.join(d, 'o.bit'),
                            '-rf', os.path.join(d, 'o.yuv')], check=True, capture_output=True)
            bits, rec = open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.yuv'), 'rb').read()
            out[name] = {'clip': CLIP, 'cfg': CFG, 'src_w': SW, 'src_h': SH, 'w': w, 'h': h, 'n': N, 'qp': QP, 'filter': 'bicubic', 'site': 'left',
                         'yuv_md5': hashlib.md5(yuv).hexdigest(), 'bit_md5': hashlib.md5(bits).hexdigest(), 'rec_md5': hashlib.md5(rec).hexdigest(),
                         'bit_bytes': len(bits), 'rec_bytes': len(rec)}
    json.dump(out, open(os.path.join(G, 'streams_scale.json'), 'w'), indent=1)
    print('wrote', len(out), 'cases')
