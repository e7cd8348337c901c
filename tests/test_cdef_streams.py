"""Whole encodes at the two CDEF search speeds no other golden uses (-m "not gpu"): -cdef 1 (speed 0, 64 strengths) and -cdef 3 (speed 2, 16 strengths),
tests/golden/gen_streams_cdef.py -> streams_cdef.json.  The reference built by oracle/Makefile reproduces the recorded hashes (pins the golden), and the
host simulation of the engine sources (tests/hostsim) reproduces the reference's streams and reconstructions.  tests/test_gpu_cdef.py runs the same cases
on the device; tests/test_kat_host_cdef.py pins the passes themselves."""
import json
import os
import pytest
from util import GOLD, REF_ENC, golden_clip, build_hostsim, run_encoder, md5

G = json.load(open(os.path.join(GOLD, 'streams_cdef.json')))
NAMES = sorted(G)


def test_goldens_are_the_cases_they_claim_to_be():
    assert len(NAMES) == 6
    speeds = [c['extra'][c['extra'].index('-cdef') + 1] for c in G.values()]
    assert sorted(set(speeds)) == ['1', '3'] and all(len(c['frames']) == c['n'] for c in G.values())
    # the searches decide differently from the default -cdef 2: the streams differ from the goldens of the same command without the option
    g2 = json.load(open(os.path.join(GOLD, 'streams.json')))
    for name, base in (('208x120_n4_q32_cdef1', '208x120_n4_q32'), ('208x120_n4_q32_cdef3', '208x120_n4_q32'), ('128x96_n9_q32_ra_cdef1', '128x96_n9_q32_ra'),
                       ('192x128_n4_q32_10bit_cdef1', '192x128_n4_q32_10bit')):
        assert G[name]['bit_md5'] != g2[base]['bit_md5'], name
    # qp 44: the P frames are coded at a frame qp of 44 or more, where the guess is cdef_bits == 0 (3 - (qp + 4) / 16)
    q44 = G['208x120_n4_q44_cdef1']['frames']
    assert q44[0][1] == 'I' and all(f[1] == 'P' and int(f[2]) >= 44 for f in q44[1:]), q44


@pytest.mark.skipif(not os.path.exists(REF_ENC), reason='oracle/_ref/Thorenc not built')
@pytest.mark.parametrize('name', NAMES)
def test_live_reference_agrees_with_recorded_hashes(name):
    c = G[name]
    bits, rec = run_encoder(REF_ENC, golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c['cfg'])
    assert md5(bits) == c['bit_md5'] and md5(rec) == c['rec_md5'] and len(bits) == c['bit_bytes']


@pytest.mark.parametrize('name', NAMES)
def test_host_simulation_matches_reference_golden(name):
    c = G[name]
    bits, rec = run_encoder(build_hostsim(), golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c['cfg'])
    assert len(bits) == c['bit_bytes']
    assert md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'
