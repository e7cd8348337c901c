#!/usr/bin/env python3
"""Record the full-size 64x64-superblock golden from the reference encoder (oracle/_ref/Thorenc): 3840x2160, I + 2 P, LDB high
efficiency at qp 32 with -log2_sb_size 6, on the generated content gen_streams_big.py uses (a 60x34 superblock grid: the only case
where a grid row is longer than the chip has compute units per stream).  The reference needs minutes of CPU for it, so it is recorded
once here (build container, `make -C oracle` first); output tests/golden/streams_big_sb64.json is committed."""
import json, os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_streams_sb64 import G, SB, record  # noqa: E402
CASES = {'4k_ldb_n3_q32_sb64': ('gen:3840,2160,3,4,2.0', 3840, 2160, 3, 32, SB)}

if __name__ == '__main__':
    with tempfile.TemporaryDirectory() as d:
        out = {name: record(case, d) for name, case in CASES.items()}
    json.dump(out, open(os.path.join(G, 'streams_big_sb64.json'), 'w'), indent=1, sort_keys=True)
    print('wrote', len(out), 'cases')
