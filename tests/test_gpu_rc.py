"""Rate control on the device (-m gpu): k_rc_cost against the numpy restatement, the C front end with -rc_bitrate against the hashes recorded from the host
simulation (tests/golden/rc_streams.json), three streams with different targets in one engine (lock step and thor_hip_encode_staged_run), and a run
through Python with frames staged from device memory."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
from util import ROOT, GOLD, REF_DEC, golden_clip, decode, md5
import rc_model as rm

sys.path.insert(0, GOLD)
import gen_rc

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(GOLD, 'rc_streams.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')
_WANT = {}


def want(w, h, depth, content):
    k = (w, h, depth, content)
    if k not in _WANT:
        cur, prev = rm.kat_case(w, h, depth, content)
        _WANT[k] = (cur, prev) + rm.analyse_luma(cur, prev)
    return _WANT[k]


@pytest.mark.parametrize('content', rm.KAT_CONTENTS)
@pytest.mark.parametrize('depth', [8, 10, 12])
@pytest.mark.parametrize('w,h', rm.KAT_SHAPES)
def test_kernel_matches_numpy(w, h, depth, content):
    import thor_amd
    cur, prev, sums, half = want(w, h, depth, content)
    got, got_half = thor_amd.kat_rc_cost(cur, prev, depth)
    assert np.array_equal(got_half, half)
    assert got == sums


_TOOL_RUNS = {}


def tool_run(name):
    if name not in _TOOL_RUNS:
        _TOOL_RUNS[name] = gen_rc.run(TOOL, CASES[name])
    return _TOOL_RUNS[name]


NOCDEF = ['ldb_30k_nocdef', 'ldb_60k_nocdef', 'ra_40k_nocdef']


@pytest.mark.parametrize('name', ['ldb_30k', 'ldb_60k', 'ra_40k'] + NOCDEF)
def test_front_end_matches_the_host_simulation(name):
    c = CASES[name]
    r = tool_run(name)
    report = r['report'][:r['report'].rindex('thorenc_hip:')]   # the throughput line follows the report
    assert md5(r['bits'][0]) == c['bit_md5'] and md5(r['rec'][0]) == c['rec_md5'] and md5(report.encode()) == c['report_md5']


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason='reference decoder not built')
@pytest.mark.parametrize('name', NOCDEF)
def test_reference_decoder_reproduces_the_device_reconstruction(name):
    """Both targets of the low-delay clip and the hierarchical-B clip; with CDEF on the reference's own decoder does not reproduce its encoder (tests/test_sb64.py)."""
    r = tool_run(name)
    assert decode(r['bits'][0]) == r['rec'][0]


def encoder(S):
    import thor_amd
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), width=64, height=64, qp=32, f=30)
    return thor_amd.Encoder(p, S)


def frames(n=8):
    clip = np.frombuffer(golden_clip('gen:64,64,16,7,3.0'), dtype=np.uint8)
    fsz = 64 * 64 * 3 // 2
    return [clip[i * fsz:(i + 1) * fsz] for i in range(n)]


def test_three_streams_two_targets_one_without():
    import thor_amd
    names = ['ldb_30k_n8', 'ldb_60k_n8', 'ldb_fixed_n8']
    fr = frames()
    outs = []
    for run in (False, True):
        with encoder(3) as enc:
            assert thor_amd.lib().thor_hip_set_rate_control(enc.h, 3, None) == 1
            enc.set_rate_control(0, thor_amd.RateControl(30000))
            enc.set_rate_control(1, thor_amd.RateControl(60000))
            enc.set_rate_control(2, None)
            rec = [b'', b'', b'']
            for s in range(3):
                for i, f in enumerate(fr):
                    enc.stage(s, i, f)
            if run:
                def done(user, first, count):
                    for s in range(first, first + count):
                        rec[s] += enc.recon(s).tobytes()
                cb = thor_amd.binding.FRAMES_DONE_FN(done)
                assert thor_amd.lib().thor_hip_encode_staged_run(enc.h, len(fr), cb, None) == 0
            else:
                for i in range(len(fr)):
                    enc.encode_staged([i, i, i])
                    for s in range(3):
                        rec[s] += enc.recon(s).tobytes()
                with pytest.raises(ValueError):   # in the middle of a sequence
                    enc.set_rate_control(0, thor_amd.RateControl(10000))
            for s, name in enumerate(names):
                c = CASES[name]
                assert md5(enc.bitstream(s)) == c['bit_md5'] and md5(rec[s]) == c['rec_md5']
                log = enc.frame_rc(s)
                rows = rm.parse_log('\n'.join(c['log']))
                assert [(x['base_qp'], x['sum_intra'], x['sum_best'], x['n_intra'], x['fullness']) for x in log] == \
                       [(x['base_qp'], x['sum_intra'], x['sum_best'], x['n_intra'], x['fullness']) for x in rows]
                assert [x['qp'] for x in enc.frame_stats(s)] == ([x['qp'] for x in rows] if rows else [30] + [38] * 7)
            outs.append([enc.bitstream(s) for s in range(3)])
    assert outs[0] == outs[1]


_CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import thor_amd
from util import golden_clip
p = thor_amd.load_config(%(cfg)r, width=64, height=64, qp=32, f=30)
clip = np.frombuffer(golden_clip('gen:64,64,16,7,3.0'), dtype=np.uint8)
fsz = 64 * 64 * 3 // 2
out = {}
with thor_amd.Encoder(p, 1) as enc:
    try:
        enc.set_rate_control(0, thor_amd.RateControl(30000, min_qp=40, max_qp=30))
        out['refused'] = False
    except ValueError:
        out['refused'] = True
    enc.set_rate_control(0, thor_amd.RateControl(30000))
    dev = torch.from_numpy(clip[:8 * fsz].copy()).cuda()
    torch.cuda.synchronize()
    rec = b''
    for i in range(8):
        enc.stage_device(0, i, dev.data_ptr() + i * fsz)
        enc.encode_staged([i])
        rec += enc.recon(0).tobytes()
    out['bit_md5'] = hashlib.md5(enc.bitstream(0)).hexdigest()
    out['rec_md5'] = hashlib.md5(rec).hexdigest()
    out['log'] = enc.frame_rc(0)
print(json.dumps(out))
"""


def test_python_run_with_frames_staged_on_the_device():
    """Encoder.set_rate_control and frame_rc with frames that live in device memory (a torch tensor), in a process of its own: torch comes first there."""
    from test_gpu_rgb import run_child
    c = CASES['ldb_30k_n8']
    code = _CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests'), 'cfg': os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')}
    o = json.loads(run_child([sys.executable, '-c', code], 180).splitlines()[-1])
    assert o['refused'] and o['bit_md5'] == c['bit_md5'] and o['rec_md5'] == c['rec_md5']
    log, rows = o['log'], rm.parse_log('\n'.join(c['log']))
    assert [(x['base_qp'], x['sum_best'], x['fullness']) for x in log] == [(x['base_qp'], x['sum_best'], x['fullness']) for x in rows]
    assert log[-1]['overflows'] == 0 and log[0]['target_bits'] == 1000 and log[0]['buffer_bits'] == 30000
