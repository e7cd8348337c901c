#!/usr/bin/env python3
"""Record golden stream / reconstruction hashes from the reference encoder (oracle/_ref/Thorenc) coding 8- and 10-bit input at a higher
internal bit depth (-bitdepth B -input_bitdepth I with B > I): the reference widens the input when it reads it, writes the -rf file
rounded back to the input depth and reports PSNR on the input-depth scale.  Same record format as gen_streams.py.  Run in the build
container after `make -C oracle`; output tests/golden/streams_mixed.json is committed and is what tests/test_mixed_depth.py and
tests/test_gpu_mixed_depth.py compare with."""
import hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G = os.path.join(ROOT, 'tests', 'golden')
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from util import golden_clip  # noqa: E402
from mixed_depth import defined_rec_bytes, round_to_input_depth  # noqa: E402
import numpy as np  # noqa: E402


def depth(bd, inp):
    return ['-bitdepth', str(bd), '-input_bitdepth', str(inp)]


CASES = {
    # 8-bit input at 10 bits: the common use
    '192x128_n4_q32_in8_bd10': ('clip_192x128_6.yuv.gz', 192, 128, 4, 32, depth(10, 8)),
    # two-stream test: stream s of a two-stream run over the 6-frame clip = the reference run with -skip 3*s -n 3
    '192x128_n3_q32_skip0_in8_bd10': ('clip_192x128_6.yuv.gz', 192, 128, 3, 32, depth(10, 8) + ['-skip', '0']),
    '192x128_n3_q32_skip3_in8_bd10': ('clip_192x128_6.yuv.gz', 192, 128, 3, 32, depth(10, 8) + ['-skip', '3']),
    # shift 4, chroma rows of 104 samples, CLPF reads the widened original
    '208x120_n4_q36_in8_bd12_clpf': ('clip_208x120_4.yuv.gz', 208, 120, 4, 36, depth(12, 8) + ['-clpf', '1'], 'ldb_medium_complexity.cfg'),
    # CDEF off: the reference decoder reproduces the reconstruction
    '208x120_n4_q36_in8_bd10_nocdef': ('clip_208x120_4.yuv.gz', 208, 120, 4, 36, depth(10, 8) + ['-cdef', '0']),
    # B frames, interpolated references
    '128x96_n9_q32_ra_in8_bd10': ('clip_128x96_9.yuv.gz', 128, 96, 9, 32, depth(10, 8), 'ra_high_efficiency.cfg'),
    # two-byte input, shift 2, reordered pictures
    '192x128_n5_q32_hdb16_gop4_in10_bd12': ('clip10_192x128_5.yuv.gz', 192, 128, 5, 32, depth(12, 10) + ['-num_reorder_pics', '3'], 'hdb16_high_efficiency.cfg'),
    # 64x64 superblocks
    '208x120_n4_q32_in8_bd10_sb64': ('clip_208x120_4.yuv.gz', 208, 120, 4, 32, depth(10, 8) + ['-log2_sb_size', '6']),
}


def record(case, d):
    clip, w, h, n, qp, extra = case[:6]
    cfg = case[6] if len(case) > 6 else 'ldb_high_efficiency.cfg'
    open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(clip))
    log = subprocess.run([os.path.join(ROOT, 'oracle/_ref/Thorenc'), '-cf', os.path.join(ROOT, 'configs', cfg),
                          '-if', os.path.join(d, 'in.yuv'), '-width', str(w), '-height', str(h), '-qp', str(qp), '-n', str(n),
                          '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + extra,
                         check=True, capture_output=True, text=True).stdout
    frames = [l.split()[:4] for l in log.splitlines() if len(l.split()) > 4 and l.split()[1] in 'IPB']
    rec = open(os.path.join(d, 'o.yuv'), 'rb').read()
    more = {}
    if extra[extra.index('-input_bitdepth') + 1] != '8':
        # two-byte samples rounded down from a higher depth: half of the reference's file is uninitialised memory (tests/mixed_depth.py), so its
        # md5 (rec_md5, recorded all the same) is not reproducible; rec_defined_md5 covers the half that is defined
        more = {'rec_defined_md5': hashlib.md5(defined_rec_bytes(rec, w, h, n, True)).hexdigest()}
        # the whole file, from a run of the reference that writes it correctly: the clip widened beforehand, input_bitdepth == bitdepth (the
        # encoder sees the same samples and reconstructs the same frames), rounded back with write_yuv_frame's formula
        bd, inp = int(extra[extra.index('-bitdepth') + 1]), int(extra[extra.index('-input_bitdepth') + 1])
        wide = (np.frombuffer(golden_clip(clip), dtype=np.uint16) << (bd - inp)).tobytes()
        open(os.path.join(d, 'wide.yuv'), 'wb').write(wide)
        eq = list(extra)
        eq[eq.index('-input_bitdepth') + 1] = str(bd)
        subprocess.run([os.path.join(ROOT, 'oracle/_ref/Thorenc'), '-cf', os.path.join(ROOT, 'configs', cfg),
                        '-if', os.path.join(d, 'wide.yuv'), '-width', str(w), '-height', str(h), '-qp', str(qp), '-n', str(n),
                        '-f', '30', '-of', os.path.join(d, 'e.bit'), '-rf', os.path.join(d, 'e.yuv')] + eq, check=True, capture_output=True)
        full = round_to_input_depth(np.frombuffer(open(os.path.join(d, 'e.yuv'), 'rb').read(), dtype=np.uint16), bd, inp).tobytes()
        assert defined_rec_bytes(full, w, h, n, False) == defined_rec_bytes(rec, w, h, n, True), 'the two runs of the reference disagree'
        more['rec_equal_depth_md5'] = hashlib.md5(full).hexdigest()
    return {**more, 'clip': clip, 'cfg': cfg, 'w': w, 'h': h, 'n': n, 'qp': qp, 'extra': extra,
            'bit_md5': hashlib.md5(open(os.path.join(d, 'o.bit'), 'rb').read()).hexdigest(),
            'rec_md5': hashlib.md5(open(os.path.join(d, 'o.yuv'), 'rb').read()).hexdigest(),
            'bit_bytes': os.path.getsize(os.path.join(d, 'o.bit')), 'rec_bytes': os.path.getsize(os.path.join(d, 'o.yuv')), 'frames': frames}


if __name__ == '__main__':
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, case in CASES.items():
            out[name] = record(case, d)
    json.dump(out, open(os.path.join(G, 'streams_mixed.json'), 'w'), indent=1)
    print('wrote', len(out), 'cases')
