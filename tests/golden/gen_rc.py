"""Records tests/golden/rc_streams.json from the host simulation (tests/hostsim/hostsim with the -rc_ options): per case the hashes of stream, reconstruction
and report and the controller's log.  The GPU tests compare the device against these; the CPU tests run the host simulation live.
  python tests/golden/gen_rc.py            writes the file
  python tests/golden/gen_rc.py --fit      prints the initial bits-per-cost factors of thor_amd/csrc/tk_rc.h and the fit's residual"""
import json
import math
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import rc_model as rm
from util import ROOT, build_hostsim, golden_clip, md5

CASES = {
    'ldb_30k': dict(cfg='ldb_high_efficiency.cfg', clip='gen:64,64,16,7,3.0', w=64, h=64, n=16, qp=32, rc=dict(bitrate=30000)),
    'ldb_60k': dict(cfg='ldb_high_efficiency.cfg', clip='gen:64,64,16,7,3.0', w=64, h=64, n=16, qp=32, rc=dict(bitrate=60000)),
    'ldb_30k_nocdef': dict(cfg='ldb_high_efficiency.cfg', clip='gen:64,64,16,7,3.0', w=64, h=64, n=16, qp=32, rc=dict(bitrate=30000), extra=['-cdef', '0']),
    'ldb_60k_nocdef': dict(cfg='ldb_high_efficiency.cfg', clip='gen:64,64,16,7,3.0', w=64, h=64, n=16, qp=32, rc=dict(bitrate=60000), extra=['-cdef', '0']),
    'ra_40k_nocdef': dict(cfg='ra_high_efficiency.cfg', clip='gen:64,64,17,5,3.0', w=64, h=64, n=17, qp=32, rc=dict(bitrate=40000, buffer_ms=2000), extra=['-cdef', '0']),
    'ldb_30k_n8': dict(cfg='ldb_high_efficiency.cfg', clip='gen:64,64,16,7,3.0', w=64, h=64, n=8, qp=32, rc=dict(bitrate=30000)),
    'ldb_60k_n8': dict(cfg='ldb_high_efficiency.cfg', clip='gen:64,64,16,7,3.0', w=64, h=64, n=8, qp=32, rc=dict(bitrate=60000)),
    'ldb_fixed_n8': dict(cfg='ldb_high_efficiency.cfg', clip='gen:64,64,16,7,3.0', w=64, h=64, n=8, qp=32, rc={}),
    'ra_40k': dict(cfg='ra_high_efficiency.cfg', clip='gen:64,64,17,5,3.0', w=64, h=64, n=17, qp=32, rc=dict(bitrate=40000, buffer_ms=2000)),
}
OPT = {'bitrate': '-rc_bitrate', 'buffer_ms': '-rc_buffer_ms', 'min_qp': '-rc_min_qp', 'max_qp': '-rc_max_qp', 'min_qp_i': '-rc_min_qpI', 'max_qp_i': '-rc_max_qpI',
       'initial_qp': '-rc_initial_qp'}


def rc_args(rc):
    return [x for k, v in rc.items() for x in (OPT[k], str(v))]


def run(binary, c, extra=(), env=None, streams=1):
    """One run of a Thorenc-compatible front end on a case: dict(bits=[...], rec=[...], report=str, log=str) per stream."""
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
        e = dict(os.environ, THOR_RC_LOG=os.path.join(d, 'rc.log'), **(env or {}))
        cmd = [binary, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']),
               '-n', str(c['n'] // streams), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv'), '-streams', str(streams)] + rc_args(c['rc']) + list(c.get('extra', [])) + list(extra)
        rep = subprocess.run(cmd, check=True, capture_output=True, text=True, env=e).stdout
        names = [''] if streams == 1 else ['.%d' % s for s in range(streams)]
        log = open(os.path.join(d, 'rc.log')).read() if os.path.exists(os.path.join(d, 'rc.log')) else ''
        return dict(bits=[open(os.path.join(d, 'o.bit' + s), 'rb').read() for s in names], rec=[open(os.path.join(d, 'o.yuv' + s), 'rb').read() for s in names],
                    report=rep, log=log)


def fit():
    obs = {c: [] for c in range(6)}
    for cfg, clip, w, h, n in (('ldb_high_efficiency.cfg', 'gen:64,64,12,7,3.0', 64, 64, 12), ('ldb_high_efficiency.cfg', 'gen:96,64,10,11,6.0', 96, 64, 10),
                               ('ra_high_efficiency.cfg', 'gen:64,64,17,5,3.0', 64, 64, 17)):
        for q in (22, 32, 42):
            r = run(build_hostsim(), dict(cfg=cfg, clip=clip, w=w, h=h, n=n, qp=q, rc=dict(bitrate=100000, min_qp=q, max_qp=q)))
            for row in rm.parse_log(r['log']):
                cost = row['sum_intra'] if row['frame_class'] == 0 else row['sum_best']
                obs[row['frame_class']].append(row['bits'] * rm.STEP_Q16[row['qp']] / max(cost, 1))
    for c, v in obs.items():
        if v:
            lg = [math.log2(x) for x in v]
            m = sum(lg) / len(lg)
            print('class %d: %d frames, factor (geometric mean) %d, rms residual %.3f in log2(bits)' % (c, len(v), round(2 ** m), (sum((x - m) ** 2 for x in lg) / len(lg)) ** .5))


if __name__ == '__main__':
    if '--fit' in sys.argv:
        fit()
    else:
        out = {}
        for name, c in CASES.items():
            r = run(build_hostsim(), c)
            out[name] = dict(c, bit_md5=md5(r['bits'][0]), bit_bytes=len(r['bits'][0]), rec_md5=md5(r['rec'][0]), report_md5=md5(r['report'].encode()), log=r['log'].splitlines())
        json.dump(out, open(os.path.join(HERE, 'rc_streams.json'), 'w'), indent=1)
