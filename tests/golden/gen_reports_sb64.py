#!/usr/bin/env python3
"""Record the reference encoder's stdout report (oracle/_ref/Thorenc) for one 64x64-superblock case of streams_sb64.json, with that
case's exact command (the report's layout does not depend on the superblock size; its bit counts and PSNRs do).  Same record format
as gen_reports.py.  Run after `make -C oracle`; output tests/golden/reports_sb64.json is committed (tests/test_sb64.py)."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from util import golden_clip  # noqa: E402
CASES = ['208x120_n4_q32_sb64']

if __name__ == '__main__':
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'streams_sb64.json')))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in CASES:
            c = gold[name]
            open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
            cmd = [os.path.join(ROOT, 'oracle', '_ref', 'Thorenc'), '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'),
                   '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30',
                   '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + c['extra']
            out[name] = {'case': name, 'extra': [], 'report': subprocess.run(cmd, check=True, capture_output=True, text=True).stdout}
    json.dump(out, open(os.path.join(ROOT, 'tests', 'golden', 'reports_sb64.json'), 'w'), indent=1)
    print('wrote', len(out), 'reports')
