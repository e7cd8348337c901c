#!/usr/bin/env python3
"""Record golden stream / reconstruction hashes from the reference encoder (oracle/_ref/Thorenc) at the two CDEF search speeds no other golden uses:
-cdef 1 (search speed 0: 64 strengths, a 64x64 table of candidate pairs) and -cdef 3 (speed 2: 16 strengths); every other golden runs the default -cdef 2
or -cdef 0.  Same record format as gen_streams.py.  Run in the build container after `make -C oracle`; output tests/golden/streams_cdef.json is committed
and is what tests/test_cdef_streams.py and tests/test_gpu_cdef.py compare with."""
import hashlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G = os.path.join(ROOT, 'tests', 'golden')
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from util import golden_clip  # noqa: E402
HBD = ['-bitdepth', '10', '-input_bitdepth', '10']
CASES = {
    # 4x2 filter blocks, the last column 16 wide (one chroma column), the last row 56 high (3 chroma rows against 7 luma rows)
    '208x120_n4_q32_cdef1': ('clip_208x120_4.yuv.gz', 208, 120, 4, 32, ['-cdef', '1']),
    '208x120_n4_q32_cdef3': ('clip_208x120_4.yuv.gz', 208, 120, 4, 32, ['-cdef', '3']),
    # 16-bit samples: the v_dot2 half of the packed sums with all 64 strengths
    '192x128_n4_q32_10bit_cdef1': ('clip10_192x128_5.yuv.gz', 192, 128, 4, 32, HBD + ['-cdef', '1']),
    # filter blocks 8 wide and 8 high: no chroma block in that direction
    '200x136_n4_q30_cdef3': ('gen:200,136,4,31,2.0', 200, 136, 4, 30, ['-cdef', '3']),
    # B frames and interpolated references
    '128x96_n9_q32_ra_cdef1': ('clip_128x96_9.yuv.gz', 128, 96, 9, 32, ['-cdef', '1'], 'ra_high_efficiency.cfg'),
    # qp 44: the P frames take cdef_bits == 0 (fixed strengths from the frame qp, enc/encode_frame.c:686) beside an I frame that searches
    '208x120_n4_q44_cdef1': ('clip_208x120_4.yuv.gz', 208, 120, 4, 44, ['-cdef', '1']),
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
    return {'clip': clip, 'cfg': cfg, 'w': w, 'h': h, 'n': n, 'qp': qp, 'extra': extra,
            'bit_md5': hashlib.md5(open(os.path.join(d, 'o.bit'), 'rb').read()).hexdigest(),
            'rec_md5': hashlib.md5(open(os.path.join(d, 'o.yuv'), 'rb').read()).hexdigest(),
            'bit_bytes': os.path.getsize(os.path.join(d, 'o.bit')), 'frames': frames}


if __name__ == '__main__':
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, case in CASES.items():
            out[name] = record(case, d)
    json.dump(out, open(os.path.join(G, 'streams_cdef.json'), 'w'), indent=1)
    print('wrote', len(out), 'cases')
