#!/usr/bin/env python3
"""Record golden stream / reconstruction hashes from the reference encoder (oracle/_ref/Thorenc) with 64x64 superblocks
(-log2_sb_size 6): the small cases at which the finer superblock grid can go wrong, and the four 3-frame chunks the multi-stream test
codes side by side.  Same record format as gen_streams.py.  Run in the build container after `make -C oracle`; output
tests/golden/streams_sb64.json is committed and is what tests/test_sb64.py and tests/test_gpu_sb64.py compare with."""
import hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G = os.path.join(ROOT, 'tests', 'golden')
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from util import golden_clip  # noqa: E402
SB = ['-log2_sb_size', '6']
HBD = ['-bitdepth', '10', '-input_bitdepth', '10']
CASES = {
    # 4x2 grid; last column 16 wide, last row 56 high: rectangular blocks and the last-column "up" dependency
    '208x120_n4_q32_sb64': ('clip_208x120_4.yuv.gz', 208, 120, 4, 32, SB),
    # CDEF off: the reference decoder reproduces the reconstruction (tests/test_reference_golden.py on tiny frames with CDEF)
    '208x120_n4_q36_nocdef_sb64': ('clip_208x120_4.yuv.gz', 208, 120, 4, 36, SB + ['-cdef', '0']),
    # 3x2 grid of whole superblocks, P frames with up to four references
    '192x128_n6_q32_sb64': ('clip_192x128_6.yuv.gz', 192, 128, 6, 32, SB),
    # 4x3 grid (three rows: down-left successors of a middle row); last column 8 wide = one minimum block
    '200x184_n4_q30_sb64': ('gen:200,184,4,21,2.0', 200, 184, 4, 30, SB),
    '200x184_n4_q30_nocdef_sb64': ('gen:200,184,4,21,2.0', 200, 184, 4, 30, SB + ['-cdef', '0']),
    # B frames, interpolated references, 2x2 grid with a 32-high row
    '128x96_n9_q32_ra_sb64': ('clip_128x96_9.yuv.gz', 128, 96, 9, 32, SB, 'ra_high_efficiency.cfg'),
    # 16-bit engine
    '192x128_n4_q32_10bit_sb64': ('clip10_192x128_5.yuv.gz', 192, 128, 4, 32, HBD + SB),
    # encoder_speed 2: the early-skip threshold of a block of superblock size (enc/encode_block.c:2256)
    '192x128_n6_q32_ldb_low_sb64': ('clip_192x128_6.yuv.gz', 192, 128, 6, 32, SB, 'ldb_low_complexity.cfg'),
    # encoder_speed 1: top-down split
    '208x120_n4_q30_ldb_medium_sb64': ('clip_208x120_4.yuv.gz', 208, 120, 4, 30, SB, 'ldb_medium_complexity.cfg'),
}
# multi-stream test: stream s of a four-stream run over a 12-frame 192x128 clip = the reference run with -skip 3*s -n 3
MULTI_CLIP = 'gen:192,128,12,7,2.0'
for s in range(4):
    CASES['192x128_n3_q32_skip%d_sb64' % (3 * s)] = (MULTI_CLIP, 192, 128, 3, 32, SB + ['-skip', str(3 * s)])


def record(case, d):
    clip, w, h, n, qp, extra = case[:6]
    cfg = case[6] if len(case) > 6 else 'ldb_high_efficiency.cfg'
    open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(clip))
    log = subprocess.run([os.path.join(ROOT, 'oracle/_ref/Thorenc'), '-cf', os.path.join(ROOT, 'configs', cfg),
                          '-if', os.path.join(d, 'in.yuv'), '-width', str(w), '-height', str(h), '-qp', str(qp), '-n', str(n),
                          '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + extra,
                         check=True, capture_output=True, text=True).stdout
    frames = [l.split()[:4] for l in log.splitlines() if len(l.split()) > 4 and l.split()[1] in 'IPB']
    return {'clip': clip, 'cfg': cfg, 'w': w, 'h': h, 'n': n, 'qp': qp, 'extra': extra,
            'bit_md5': hashlib.md5(open(os.path.join(d, 'o.bit'), 'rb').read()).hexdigest(),
            'rec_md5': hashlib.md5(open(os.path.join(d, 'o.yuv'), 'rb').read()).hexdigest(),
            'bit_bytes': os.path.getsize(os.path.join(d, 'o.bit')), 'frames': frames}


if __name__ == '__main__':
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, case in CASES.items():
            out[name] = record(case, d)
    json.dump(out, open(os.path.join(G, 'streams_sb64.json'), 'w'), indent=1)
    print('wrote', len(out), 'cases')
