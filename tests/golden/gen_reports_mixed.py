#!/usr/bin/env python3
"""Record the reference encoder's stdout report (oracle/_ref/Thorenc) for every mixed-depth case of streams_mixed.json, with that
case's exact command: the PSNR columns are on the input-depth scale (common/snr.c:39-61).  Same record format as gen_reports.py.
Run after `make -C oracle` and gen_streams_mixed.py; output tests/golden/reports_mixed.json is committed (tests/test_mixed_depth.py,
tests/test_gpu_mixed_depth.py)."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from util import golden_clip  # noqa: E402

if __name__ == '__main__':
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'streams_mixed.json')))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, c in gold.items():
            open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
            cmd = [os.path.join(ROOT, 'oracle', '_ref', 'Thorenc'), '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'),
                   '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30',
                   '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + c['extra']
            out[name] = {'case': name, 'extra': [], 'report': subprocess.run(cmd, check=True, capture_output=True, text=True).stdout}
    json.dump(out, open(os.path.join(ROOT, 'tests', 'golden', 'reports_mixed.json'), 'w'), indent=1)
    print('wrote', len(out), 'reports')
