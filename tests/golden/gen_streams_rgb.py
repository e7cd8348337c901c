#!/usr/bin/env python3
"""Record what the reference encoder (oracle/_ref/Thorenc) makes of an RGB clip: the seeded synthetic BGRA clip of tests/rgb_format.py (written
to tests/golden/clip_rgb_80x48_4.bgra.gz) is converted to planar 4:2:0 with the numpy model of the same file - BT.709, limited range, left-sited
chroma, the defaults of -pixfmt bgra - and encoded at (bitdepth, input_bitdepth) = (8, 8) and (10, 8).  Recorded: md5 of the bitstream, of the
reconstruction (planar, input-depth samples) and of the model's inverse of that reconstruction (BGRA).  tests/test_rgb_streams.py and tests/test_gpu_rgb.py feed the RGB clip itself to this project and
compare.  Run in the build container after `make -C oracle`."""
import gzip, hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G = os.path.join(ROOT, 'tests', 'golden')
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402
import rgb_format as rf  # noqa: E402

W, H, N, QP = 80, 48, 4, 32
CLIP = 'clip_rgb_80x48_4.bgra.gz'
CFG = 'ldb_high_efficiency.cfg'
CASES = {'80x48_n4_q32_bgra': [], '80x48_n4_q32_bgra_in8_bd10': ['-bitdepth', '10', '-input_bitdepth', '8']}


def clip_to_yuv(clip):
    """The BGRA clip as planar 4:2:0 of 8-bit samples, by the model."""
    f = rf.Format(W, H, rf.BGRA)
    return b''.join(rf.to_yuv(*rf.unpack(clip[i * f.bytes:(i + 1) * f.bytes], f), f, 8).tobytes() for i in range(N))


if __name__ == '__main__':
    clip = rf.make_clip(W, H, N)
    with gzip.GzipFile(os.path.join(G, CLIP), 'wb', mtime=0) as z:
        z.write(clip)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(clip_to_yuv(clip))
        for name, extra in CASES.items():
            subprocess.run([os.path.join(ROOT, 'oracle/_ref/Thorenc'), '-cf', os.path.join(ROOT, 'configs', CFG), '-if', os.path.join(d, 'in.yuv'),
                            '-width', str(W), '-height', str(H), '-qp', str(QP), '-n', str(N), '-f', '30', '-of', os.path.join(d, 'o.bit'),
                            '-rf', os.path.join(d, 'o.yuv')] + extra, check=True, capture_output=True)
            bits, rec = open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.yuv'), 'rb').read()
            # the -rf file of a run with -pixfmt bgra holds RGB: the model's inverse of the reference's reconstruction
            f = rf.Format(W, H, rf.BGRA)
            fsz = W * H * 3 // 2
            rec_rgb = b''.join(rf.pack(*rf.to_rgb(np.frombuffer(rec[i * fsz:(i + 1) * fsz], dtype=np.uint8), f, 8), f).tobytes() for i in range(N))
            out[name] = {'clip': CLIP, 'cfg': CFG, 'w': W, 'h': H, 'n': N, 'qp': QP, 'extra': extra, 'pixfmt': 'bgra',
                         'clip_md5': hashlib.md5(clip).hexdigest(), 'yuv_md5': hashlib.md5(clip_to_yuv(clip)).hexdigest(),
                         'bit_md5': hashlib.md5(bits).hexdigest(), 'rec_md5': hashlib.md5(rec).hexdigest(), 'rec_rgb_md5': hashlib.md5(rec_rgb).hexdigest(),
                         'bit_bytes': len(bits), 'rec_bytes': len(rec)}
    json.dump(out, open(os.path.join(G, 'streams_rgb.json'), 'w'), indent=1)
    print('wrote', len(out), 'cases;', os.path.getsize(os.path.join(G, CLIP)), 'bytes of clip')
