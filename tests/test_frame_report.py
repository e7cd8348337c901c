"""The encoder report (-m "not gpu"): the reference's stdout - "SH:" line, one line per coded frame with bits and PSNR, the average
block - and its -stat line, recorded from oracle/_ref/Thorenc for every case of streams.json (tests/golden/gen_reports.py ->
reports.json).  The host simulation of the engine (tests/hostsim: the engine sources, SSE rows included) must print it byte for
byte; unit cases of the formatter (thor_amd/csrc/tk_report.h) through tests/hostsim/unit_report.cpp."""
import json
import math
import os
import subprocess
import tempfile
import pytest
from util import ROOT, GOLD, REF_ENC, golden_streams, golden_clip, build_hostsim

G = golden_streams()
REPORTS = json.load(open(os.path.join(GOLD, 'reports.json')))


def run_report(binary, name, env=None):
    """Run a Thorenc-compatible CLI on the case `name` of reports.json; returns (stdout, -stat file contents or None)."""
    r = REPORTS[name]
    c = G[r['case']]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
        sf = os.path.join(d, 'stat.txt')
        cmd = [binary, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', str(c['w']), '-height', str(c['h']),
               '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + c['extra'] + r['extra']
        if 'stat' in r:
            cmd += ['-stat', sf]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env).stdout
        return out, (open(sf).read() if 'stat' in r else None)


def test_reports_cover_every_golden_stream():
    assert set(G) <= set(REPORTS)
    for name, r in REPORTS.items():
        c = G[r['case']]
        lines = r['report'].splitlines()
        assert lines[0].startswith('SH:') and len(lines) == 1 + len(c['frames']) + 6
        if not r['extra']:   # the bits column is what streams.json recorded
            assert [l.split()[:4] for l in lines[1:1 + len(c['frames'])]] == c['frames']


@pytest.mark.skipif(not os.path.exists(REF_ENC), reason='oracle/_ref/Thorenc not built')
@pytest.mark.parametrize('name', ['192x128_n3_q32_skip3', '128x96_n9_q32_ra', '192x128_n3_q32_snrcalc0', '208x120_n4_q32_stat'])
def test_live_reference_reproduces_recorded_report(name):
    out, stat = run_report(REF_ENC, name)
    assert out == REPORTS[name]['report']
    assert stat == REPORTS[name].get('stat')


HOSTSIM_CASES = ['192x128_n3_q32', '192x128_n3_q32_skip3', '128x96_n9_q32_ra', '192x128_n6_q30_ra_gop4', '192x128_n5_q32_hdb16_gop4_10bit',
                 '192x128_n4_q32_12bit', '208x120_n4_q38_ldb_medium_clpf', '208x120_n4_q36_nocdef', '192x128_n3_q32_snrcalc0', '208x120_n4_q32_stat',
                 '192x128_n4_q32_12bit_stat']


@pytest.mark.parametrize('name', HOSTSIM_CASES)
def test_host_simulation_prints_the_reference_report(name):
    out, stat = run_report(build_hostsim(), name)
    assert out == REPORTS[name]['report']
    assert stat == REPORTS[name].get('stat')


def test_host_simulation_streams_print_one_report_each():
    """-streams 2: stream 1 is the -skip 3 chunk; each report follows a line "stream <s>", one -stat line per stream."""
    c = G['192x128_n3_q32']
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
        sf = os.path.join(d, 'stat.txt')
        out = subprocess.run([build_hostsim(), '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', '192',
                              '-height', '128', '-qp', '32', '-n', '3', '-f', '30', '-streams', '2', '-stat', sf],
                             check=True, capture_output=True, text=True).stdout
        stat = open(sf).read().splitlines()
    assert out == 'stream 0\n' + REPORTS['192x128_n3_q32']['report'] + 'stream 1\n' + REPORTS['192x128_n3_q32_skip3']['report']
    assert len(stat) == 3 and stat[0] == ' NFR     kbps     PSNRY  PSNRU  PSNRV'


def _psnr(sse, bits, w, h):
    m = float((1 << bits) - 1)
    return -10 * math.log10(sse / (m * m * h * w)) if sse else math.inf


def test_formatter_inf_snrcalc0_and_reference_list_padding(tmp_path):
    exe = str(tmp_path / 'unit_report')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-o', exe, os.path.join(ROOT, 'tests', 'hostsim', 'unit_report.cpp')])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    p1 = [_psnr(1234567, 8, 64, 32), _psnr(89, 8, 32, 16), _psnr(1, 8, 32, 16)]
    acc = [math.inf + p1[0], math.inf + p1[1], math.inf + p1[2]]
    kbps = 0.001 * 30.0 * (58 + 1000 + 200 + 50) / 3
    want = ('SH:    58 bits\n'
            '%4d I %4d %10d %10.4f %8.4f %8.4f ' % (0, 30, 1000, math.inf, math.inf, math.inf) + '   ' * 4 + ' | \n'
            '%4d P %4d %10d %10.4f %8.4f %8.4f ' % (4, 32, 200, *p1) + '  0' + '   ' * 3 + ' |   0\n'
            '%4d B %4d %10d %10.4f %8.4f %8.4f ' % (2, 36, 50, 0, 0, 0) + 'I(1,0)   1  0' + '   ' + ' | I(0,4)  0  4\n'
            '------------------- Average data for all frames ------------------------------\n'
            'kbps            : %12.3f\nPSNR Y          : %12.3f\nPSNR U          : %12.3f\nPSNR V          : %12.3f\n' % (kbps, acc[0] / 3, acc[1] / 3, acc[2] / 3) +
            '------------------------------------------------------------------------------\n'
            '%4d %12.3f %6.3f %6.3f %6.3f\n' % (3, kbps, acc[0] / 3, acc[1] / 3, acc[2] / 3))
    assert out.startswith(want), out
    rest = out[len(want):].splitlines()
    assert rest[0] == 'SH:    60 bits'
    assert rest[1] == '%4d I %4d %10d %10.4f %8.4f %8.4f ' % (0, 0, 0, _psnr(4095 * 4095 * 64 * 32, 12, 64, 32), _psnr(1, 12, 32, 16), _psnr(2, 12, 32, 16)) + '   ' + ' | '
    assert ' inf ' in out.splitlines()[1] and '0.0000   0.0000   0.0000 I(1,0)' in out
