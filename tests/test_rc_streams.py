"""Rate-controlled encodes through the host simulation (-m "not gpu"): the controller's Python restatement (tests/rc_model.py) fed with the analysis sums
and bit counts of a run yields the QP and fullness sequence the run logged - low delay, dyadic hierarchical B, two streams with different targets in one
engine, lock step and staggered - and the properties a rate-controlled stream must have: the reference decoder reproduces the reconstruction, a higher
target gives more bytes at a lower QP, the buffer stays within its bounds, and a pinned base QP is the fixed-QP encode."""
import json
import os
import sys
import pytest
from util import ROOT, GOLD, REF_DEC, build_hostsim, decode, md5
import rc_model as rm

sys.path.insert(0, GOLD)
import gen_rc

CASES = json.load(open(os.path.join(GOLD, 'rc_streams.json')))
_RUNS = {}


def hostsim_run(name, **kw):
    """One host-simulation run per case and variant, shared by the tests of this file."""
    key = (name, json.dumps(kw, sort_keys=True))
    if key not in _RUNS:
        c = dict(CASES[name])
        c['rc'] = dict(c['rc'], **kw.pop('rc', {}))
        _RUNS[key] = gen_rc.run(build_hostsim(), c, **kw)
    return _RUNS[key]


# ---- controller ------------------------------------------------------------------------------------------------------------------------------

def check_replay(rows, c, rc):
    p = rm.read_params(os.path.join(ROOT, 'configs', c['cfg']), c['qp'])
    got, ctl = rm.replay(rows, p, **rc)
    assert got == [(r['base_qp'], r['qp'], r['fullness'], r['overflows']) for r in rows]
    return ctl


@pytest.mark.parametrize('name', ['ldb_30k', 'ra_40k'])
def test_controller_restatement_yields_the_logged_decisions(name):
    c = CASES[name]
    r = hostsim_run(name)
    rows = rm.parse_log(r['log'])
    assert len(rows) == c['n']
    check_replay(rows, c, c['rc'])
    assert r['log'].splitlines() == c['log'] and md5(r['bits'][0]) == c['bit_md5'] and md5(r['rec'][0]) == c['rec_md5'] and md5(r['report'].encode()) == c['report_md5']


def test_two_streams_with_different_targets_in_one_engine():
    c = CASES['ldb_30k']
    r = hostsim_run('ldb_30k', streams=2, env={'THOR_RC_SCALE': '1'})   # stream 1 aims at twice stream 0's bitrate
    rows = rm.parse_log(r['log'])
    for s in (0, 1):
        mine = [x for x in rows if x['stream'] == s]
        assert len(mine) == c['n'] // 2
        check_replay(mine, c, dict(c['rc'], bitrate=c['rc']['bitrate'] * (1 + s)))
    st = hostsim_run('ldb_30k', streams=2, env={'THOR_RC_SCALE': '1', 'THOR_STAGGER': '1'})   # the two groups half a frame apart
    assert st['bits'] == r['bits'] and st['rec'] == r['rec'] and st['log'] == r['log']


# ---- properties ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(REF_DEC), reason='reference decoder not built')
@pytest.mark.parametrize('name', ['ldb_30k', 'ra_40k'])
def test_reference_decoder_reproduces_the_reconstruction(name):
    r = hostsim_run(name, extra=['-cdef', '0'])   # with CDEF on the reference's own decoder does not reproduce its encoder (tests/test_sb64.py)
    assert decode(r['bits'][0]) == r['rec'][0]


def test_higher_target_gives_more_bytes_and_lower_qp():
    lo, hi = hostsim_run('ldb_30k'), hostsim_run('ldb_60k')
    qlo, qhi = [x['qp'] for x in rm.parse_log(lo['log'])], [x['qp'] for x in rm.parse_log(hi['log'])]
    assert len(hi['bits'][0]) > len(lo['bits'][0]) and sum(qhi) / len(qhi) < sum(qlo) / len(qlo)


@pytest.mark.parametrize('name', ['ldb_30k', 'ldb_60k', 'ra_40k'])
def test_buffer_stays_within_bounds_without_reaching_a_qp_limit(name):
    K = 2
    c = CASES[name]
    rows = rm.parse_log(hostsim_run(name)['log'])
    B = c['rc']['bitrate'] * c['rc'].get('buffer_ms', 1000) // 1000
    assert all(abs(x['fullness']) <= B for x in rows[K:]) and rows[-1]['overflows'] == 0
    assert all(0 < x['base_qp'] < 51 for x in rows)


def test_pinned_qp_equals_the_fixed_qp_run():
    q = 30
    c = dict(CASES['ldb_30k'], qp=q)
    pinned = gen_rc.run(build_hostsim(), dict(c, rc=dict(bitrate=30000, min_qp=q, max_qp=q)))
    fixed = gen_rc.run(build_hostsim(), dict(c, rc={}))
    assert pinned['bits'] == fixed['bits'] and pinned['rec'] == fixed['rec'] and pinned['report'] == fixed['report']
    assert fixed['log'] == ''
