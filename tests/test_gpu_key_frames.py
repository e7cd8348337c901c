"""Key frames on the device (-m gpu): the instantiation of k_rc_cost that halves the previous original itself against the numpy restatement and against the
stored-plane instantiation, the C front end with the -key_ options against the reference's -intra_period hashes and the host simulation's bytes and logs
(tests/golden/key_streams.json), and three streams in one engine - one forced, one with scene cuts, one plain - in lock step and staggered."""
import json
import os
import numpy as np
import pytest
from util import ROOT, GOLD, golden_clip, md5
import key_model as km
import rc_model as rm
from test_gpu_rc import want

pytestmark = pytest.mark.gpu
KS = json.load(open(os.path.join(GOLD, 'key_streams.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')


@pytest.mark.parametrize('content', rm.KAT_CONTENTS)
@pytest.mark.parametrize('depth', [8, 10, 12])
@pytest.mark.parametrize('w,h', rm.KAT_SHAPES)
def test_kernel_variant_matches_numpy_and_the_stored_plane_path(w, h, depth, content):
    import thor_amd
    cur, prev, sums, _ = want(w, h, depth, content)
    got = thor_amd.kat_scene_cost(cur, prev, depth)
    assert got == sums
    assert got == thor_amd.kat_rc_cost(cur, prev, depth)[0]


def clip_of(c):
    return km.cut_clip()[1] if c['clip'] == 'cut' else golden_clip(c['clip'])


@pytest.mark.parametrize('name', sorted(KS['ref']))
def test_front_end_reproduces_the_reference_intra_period(name):
    c = KS['ref'][name]
    r = km.run(TOOL, clip_of(c), c['w'], c['h'], c['n'], c['qp'], ['-intra_period', '0', '-key_frames', c['keys']] + c.get('keys_extra', []))
    assert md5(r['bits'][0]) == c['bit_md5'] and md5(r['rec'][0]) == c['rec_md5']


@pytest.mark.parametrize('name', ['key2_nocdef', 'cut', 'cut_rc'])
def test_front_end_matches_the_host_simulation(name):
    c = KS['host'][name]
    r = km.run(TOOL, clip_of(c), c['w'], c['h'], c['n'], c['qp'], c['extra'])
    assert md5(r['bits'][0]) == c['bit_md5'] and md5(r['rec'][0]) == c['rec_md5'] and r['key_log'].splitlines() == c['key_log']


def test_front_end_refuses_a_b_frame_configuration():
    c = KS['host']['key2_nocdef']
    r = km.run(TOOL, clip_of(c), c['w'], c['h'], 2, c['qp'], ['-key_frames', '1'], cfg='ra_high_efficiency.cfg', check=False)
    assert r['returncode'] == 2 and 'Run-time error' in r['stderr']


def test_three_streams_forced_scene_cut_and_plain():
    import thor_amd
    names = ['key5_cut_clip', 'cut', 'plain_cut_clip']
    fr = [np.concatenate([p.ravel() for p in f]) for f in km.cut_clip()[0]]
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), width=km.CUT_W, height=km.CUT_H, qp=32, f=30)
    outs = []
    for run in (False, True):
        with thor_amd.Encoder(p, 3) as enc:
            for s in range(3):
                enc.begin_sequence(s, 0, len(fr), len(fr))
                for i, f in enumerate(fr):
                    enc.stage(s, i, f)
            enc.force_key_frame(0, 5)
            enc.force_key_frame(0, 5)   # asked for twice, held once
            enc.set_scene_cut(1, thor_amd.SceneCut(km.PERCENT))
            with pytest.raises(ValueError):
                enc.force_key_frame(0, len(fr))
            with pytest.raises(ValueError):
                enc.set_scene_cut(3, thor_amd.SceneCut(km.PERCENT))
            rec = [b'', b'', b'']
            if run:
                def done(first, count):
                    for s in range(first, first + count):
                        rec[s] += enc.recon(s).tobytes()
                enc.encode_run(len(fr), done)
            else:
                for i in range(len(fr)):
                    enc.encode_staged([i, i, i])
                    for s in range(3):
                        rec[s] += enc.recon(s).tobytes()
                with pytest.raises(ValueError):   # frame 2 is coded; the stream is in the middle of a sequence
                    enc.force_key_frame(0, 2)
                with pytest.raises(ValueError):
                    enc.set_scene_cut(1, None)
            for s, name in enumerate(names):
                c = KS['host'][name]
                assert md5(enc.bitstream(s)) == c['bit_md5'] and md5(rec[s]) == c['rec_md5']
                rows = km.parse_log('\n'.join(c['key_log']))
                assert [(x['reason'], x['sum_intra'], x['sum_best'], x['n_intra']) for x in enc.frame_key(s)] == \
                       [(x['reason'], x['sum_intra'], x['sum_best'], x['n_intra']) for x in rows]
                assert [x['type'] for x in enc.frame_stats(s)] == ['IPB'[x['frame_type']] for x in rows]
            assert all(x['ref_frame_num'] and min(x['ref_frame_num']) >= 5 for x in enc.frame_stats(0)[6:])
            logged = enc.frame_key(1)
            for i in range(len(fr)):   # the call of its own on the staged slots, after the run: it touches nothing of the stream
                assert enc.scene_cost(1, i, i - 1) == [logged[i]['sum_intra'], logged[i]['sum_best'], logged[i]['n_intra']]
            outs.append([enc.bitstream(s) for s in range(3)])
    assert outs[0] == outs[1]


def test_hierarchical_b_engine_refuses_every_entry_point():
    import thor_amd
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', 'ra_high_efficiency.cfg'), width=64, height=64, qp=32, f=30)
    with thor_amd.Encoder(p, 1) as enc:
        L = thor_amd.lib()
        sums = (thor_amd.binding.C.c_ulonglong * 3)()
        sc = thor_amd.SceneCut(50)
        assert L.thor_hip_force_key_frame(enc.h, 0, 1) == 2 and L.thor_hip_set_scene_cut(enc.h, 0, sc) == 2 and L.thor_hip_scene_cost(enc.h, 0, 0, -1, sums) == 2


def test_more_requests_than_the_cap_are_refused():
    import thor_amd
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), width=64, height=64, qp=32, f=30)
    with thor_amd.Encoder(p, 1) as enc:
        enc.begin_sequence(0, 0, 200, 200)
        for i in range(km.MAX_REQUESTS):
            enc.force_key_frame(0, 2 * i + 1)
        with pytest.raises(ValueError):
            enc.force_key_frame(0, 199)
        enc.begin_sequence(0, 0, 200, 200)   # empties the set
        enc.force_key_frame(0, 199)
