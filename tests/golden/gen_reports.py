#!/usr/bin/env python3
"""Record the reference encoder's stdout report (oracle/_ref/Thorenc: the "SH:" line, one line per coded frame with bits and PSNR,
the average block) for every case of streams.json, with that case's exact command, plus a -snrcalc 0 case and the line a -stat
file receives.  Run after `make -C oracle`; output tests/golden/reports.json is committed and is what test_frame_report.py /
test_gpu_frame_stats.py compare with."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from util import golden_clip, golden_streams  # noqa: E402

REF = os.path.join(ROOT, 'oracle', '_ref', 'Thorenc')
# extra cases: (name, streams.json case, extra options, -stat file wanted)
EXTRA = [('192x128_n3_q32_snrcalc0', '192x128_n3_q32', ['-snrcalc', '0'], False),
         ('208x120_n4_q32_stat', '208x120_n4_q32', [], True),
         ('192x128_n4_q32_12bit_stat', '192x128_n4_q32_12bit', [], True)]


def command(c, d, extra=()):
    return [REF, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', str(c['w']), '-height', str(c['h']),
            '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + c['extra'] + list(extra)


def main():
    gold = golden_streams()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        jobs = [(name, name, [], False) for name in gold] + EXTRA
        for name, base, extra, stat in jobs:
            c = gold[base]
            open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
            sf = os.path.join(d, 'stat.txt')
            if os.path.exists(sf):
                os.remove(sf)
            cmd = command(c, d, extra + (['-stat', sf] if stat else []))
            rep = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
            e = {'case': base, 'extra': extra, 'report': rep}
            if stat:
                e['stat'] = open(sf).read()
            out[name] = e
    json.dump(out, open(os.path.join(ROOT, 'tests', 'golden', 'reports.json'), 'w'), indent=1)
    print('wrote', len(out), 'reports')


if __name__ == '__main__':
    main()
