"""The temporal noise filter without a GPU (-m "not gpu"): the host twin tf_filter_frame against its numpy restatement (tests/tf_model.py), the model's effect
on a noisy clip, exactness of the front end's -tf_ options through the host simulation, and the argument checks."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest
from util import ROOT, GOLD, build_hostsim, golden_clip, md5
import key_model as km
import tf_model as tm

TS = json.load(open(os.path.join(GOLD, 'tf_streams.json')))
HOSTSIM_DIR = os.path.join(ROOT, 'tests', 'hostsim')
_BUILT = {}


def build_host_program(name):
    """tests/hostsim/<name>.cpp with the flags of util.build_hostsim (1-lane teams)."""
    if name not in _BUILT:
        out, src = os.path.join(HOSTSIM_DIR, name), os.path.join(HOSTSIM_DIR, name + '.cpp')
        csrc = os.path.join(ROOT, 'thor_amd', 'csrc')
        deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc)]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
            subprocess.check_call(['g++', '-std=c++17', '-O2', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-pthread', '-o', out, src])
        _BUILT[name] = out
    return _BUILT[name]


# ---- 1. the host twin against the model ---------------------------------------------------------------------------------------------------------------

def host_filter(cur, refs, dists, depth, strength, tmp_path):
    """tests/hostsim/unit_tf.cpp: (planes, mv, wb) like tf_model.filter_frame."""
    h, w = cur[0].shape
    fin, fout = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    open(fin, 'wb').write(tm.join_frames([cur] + list(refs)))
    subprocess.check_call([build_host_program('unit_tf'), 'filter', str(w), str(h), str(depth), str(strength), str(len(refs))] + [str(d) for d in dists] + [fin, fout])
    raw = open(fout, 'rb').read()
    fsz = w * h * 3 // 2 * (1 if depth == 8 else 2)
    planes = tm.split_frames(raw[:fsz], w, h, 1, depth)[0]
    rec = np.frombuffer(raw[fsz:], dtype=np.int32).reshape(len(refs), h // 8, w // 8, 3)
    return planes, rec[..., :2], rec[..., 2]


def check_case(got, want, cur, content):
    """Vectors first, then wb, then samples: a mismatch names its stage.  Then what the content promises."""
    (gp, gmv, gwb), (wp, wmv, wwb) = got, want
    assert np.array_equal(gmv, wmv), 'vectors'
    assert np.array_equal(gwb, wwb), 'wb'
    for p in range(3):
        assert np.array_equal(gp[p], wp[p]), 'plane %d' % p
    if content in ('identical', 'max'):
        assert (wmv == 0).all() and (wwb[:2] == 192).all() and all(np.array_equal(wp[p], cur[p]) for p in range(3))
    if content == 'unrelated':
        assert (wwb == 0).all() and all(np.array_equal(wp[p], cur[p]) for p in range(3))
    if content == 'flat':
        assert (wmv == 0).all()
    if content == 'pan_8_m8' and cur[0].shape[1] > 100:   # found by the blocks whose displaced block lies inside the plane
        assert ((wmv[1, 1:, :-1, 0] == 8) & (wmv[1, 1:, :-1, 1] == -8)).all() and (wwb[1, 1:, :-1] > 0).all()   # neighbour 1 shows the scene moved by (-8, 8)
        assert ((wmv[0, :-1, 1:, 0] == -8) & (wmv[0, :-1, 1:, 1] == 8)).all() and (wwb[0, :-1, 1:] > 0).all()
    if content == 'edge_ties':   # rows of equal SADs: the rank decides, and the zero vector wins every tie it is part of
        assert (wmv[..., 1] <= 0).all()


@pytest.mark.parametrize('w,h,depth,content,nrefs', list(tm.kat_cases()))
def test_host_twin_matches_the_model(w, h, depth, content, nrefs, tmp_path):
    cur, refs, dists = tm.kat_case(w, h, depth, content, nrefs)
    want = tm.filter_frame(cur, refs, dists, depth, tm.STRENGTH)
    check_case(host_filter(cur, refs, dists, depth, tm.STRENGTH, tmp_path), want, cur, content)


def test_pan_out_of_range_is_not_followed():
    """A pan of 9 lies outside [-8, 8]: no block reports it, and the blocks of the textured interior find no neighbour worth a weight above the one of a miss."""
    cur, refs, dists = tm.kat_case(136, 72, 8, 'pan_9')
    _, mv, _ = tm.filter_frame(cur, refs, dists, 8, tm.STRENGTH)
    assert np.abs(mv).max() <= 8


# ---- 2. the model does its job ---------------------------------------------------------------------------------------------------------------------------

def test_model_reduces_noise_on_a_panning_clip():
    from thor_amd import synth
    w, h, n = 96, 64, 7
    clean = synth.make_clip(w, h, n, 5, 0.0)
    rng = np.random.default_rng(17)
    noisy = [tuple(np.clip(np.rint(p + rng.normal(0.0, 6.0, size=p.shape)), 0, 255).astype(np.uint8) for p in f) for f in clean]
    filt = tm.filter_clip(noisy, 8, 6, 2, 2)
    sse = lambda a, b: int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    for f in range(2, n - 2):   # the interior frames have all four neighbours
        before, after = sse(noisy[f][0], clean[f][0]), sse(filt[f][0], clean[f][0])
        print('frame', f, 'luma SSE against the clean frame: noisy', before, 'filtered', after)
        assert after < before


# ---- 3. exactness through the encoder (host simulation) --------------------------------------------------------------------------------------------------

def tf_run(binary, name, filtered_by_model, env=None):
    c = TS[name]
    clip = golden_clip(c['clip'])
    extra = list(c.get('extra', []))
    if filtered_by_model:
        clip = tm.join_frames(tm.filter_clip(tm.split_frames(clip, c['w'], c['h'], c['n'], c['depth']), c['depth'], c['strength'], c['past'], c['future']))
    else:
        extra += ['-tf_strength', str(c['strength']), '-tf_past', str(c['past']), '-tf_future', str(c['future'])]
    return km.run(binary, clip, c['w'], c['h'], c['n'], c['qp'], extra, cfg=c['cfg'], env=env)


@pytest.mark.parametrize('name', sorted(TS))
def test_tool_with_the_filter_codes_the_model_filtered_clip(name):
    a, b = tf_run(build_hostsim(), name, False), tf_run(build_hostsim(), name, True)
    assert a['bits'][0] == b['bits'][0] and a['rec'][0] == b['rec'][0]
    assert md5(a['bits'][0]) == TS[name]['bit_md5'] and md5(a['rec'][0]) == TS[name]['rec_md5']
    plain = km.run(build_hostsim(), golden_clip(TS[name]['clip']), TS[name]['w'], TS[name]['h'], TS[name]['n'], TS[name]['qp'], TS[name].get('extra', []), cfg=TS[name]['cfg'])
    assert plain['bits'][0] != a['bits'][0]


def test_front_end_refusals():
    c = TS['ldb_8bit']
    for extra in (['-tf_strength', '17'], ['-tf_strength', '-1'], ['-tf_strength', '6', '-tf_past', '3'], ['-tf_strength', '6', '-tf_future', '-1']):
        r = km.run(build_hostsim(), golden_clip(c['clip']), c['w'], c['h'], 2, extra=extra, check=False)
        assert r['returncode'] == 2 and 'Run-time error' in r['stderr'], extra


# ---- 4. argument checks, without a device -------------------------------------------------------------------------------------------------------------------

def requests_ok(reqs, streams=2, staged=6):
    """tk::tf_requests_ok, the check thor_hip_filter_staged makes before it touches the device, with slots 0 .. staged - 1 of every stream staged."""
    flat = []
    for (stream, dst, slot, refs, dists) in reqs:
        flat += [stream, dst, slot, len(refs)] + (list(refs) + [0] * 4)[:4] + (list(dists) + [0] * 4)[:4]
    out = subprocess.run([build_host_program('unit_tf'), 'requests', str(streams), str(staged), str(len(reqs))] + [str(v) for v in flat], check=True, capture_output=True, text=True)
    return int(out.stdout) == 0


def test_request_checks():
    good = (0, 8, 2, [1, 0, 3, 4], [1, 2, 1, 2])
    assert requests_ok([good]) and requests_ok([good, (1, 8, 2, [], [])]) and requests_ok([good, (0, 9, 3, [2, 4], [1, 1])])
    assert requests_ok([(0, 9, 2, [1], [1]), (0, 10, 1, [2], [1])])              # a neighbour that is another request's source
    assert not requests_ok([(0, 2, 2, [1], [1])])                                # destination equals its source
    assert not requests_ok([(0, 1, 2, [1], [1])])                                # destination equals a neighbour
    assert not requests_ok([good, (0, 9, 3, [8], [1])])                          # a neighbour is another request's destination (and not staged)
    assert not requests_ok([(0, 3, 2, [1], [1]), (0, 9, 3, [2], [1])])           # destination is a source of another request of the call
    assert not requests_ok([good, (0, 8, 3, [], [])])                            # duplicate destinations
    assert requests_ok([good, (1, 8, 3, [], [])])                                # ... in different streams are different slots
    assert not requests_ok([(0, 8, 6, [], [])]) and not requests_ok([(0, 8, 2, [6], [1])]) and not requests_ok([(0, 8, -1, [], [])])   # an unstaged slot
    assert not requests_ok([(0, 8, 2, [1], [0])]) and not requests_ok([(0, 8, 2, [1], [3])])   # ref_dist 0 or 3
    assert not requests_ok([(0, 8, 2, [1, 0, 3, 4, 5], [1, 2, 1, 2, 1])])         # nrefs 5
    assert not requests_ok([(2, 8, 2, [], [])]) and not requests_ok([(0, -1, 2, [], [])]) and not requests_ok([])


def test_temporal_filter_check_needs_no_device():
    import thor_amd
    T = thor_amd.TemporalFilter
    assert T(1).ok() and T(6).ok() and T(16).ok()
    assert not T(0).ok() and not T(17).ok() and not T(-3).ok() and thor_amd.lib().thor_hip_temporal_filter_check(None) == 1
    bad = T(6)
    bad.size += 4
    assert not bad.ok()
    req = (thor_amd.binding.TfRequest * 1)()
    assert thor_amd.lib().thor_hip_filter_staged(None, req, 1, C.byref(T(6))) == 1


def test_layout_of_the_new_structures(tmp_path):
    """The C compiler's layout of thor_hip_temporal_filter and thor_hip_tf_request against the ctypes mirrors of thor_amd/binding.py."""
    from thor_amd import binding as b
    src = tmp_path / 'lay.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thor_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(thor_hip_temporal_filter), offsetof(thor_hip_temporal_filter, size), offsetof(thor_hip_temporal_filter, strength));\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(thor_hip_tf_request), offsetof(thor_hip_tf_request, stream), offsetof(thor_hip_tf_request, dst_slot), offsetof(thor_hip_tf_request, slot), offsetof(thor_hip_tf_request, nrefs), offsetof(thor_hip_tf_request, ref_slot), offsetof(thor_hip_tf_request, ref_dist));\n'
                   '  return 0;\n}\n')
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(tmp_path / 'lay'), str(src)])
    got = subprocess.run([str(tmp_path / 'lay')], check=True, capture_output=True, text=True).stdout.split()
    want = [C.sizeof(b.TemporalFilter)] + [getattr(b.TemporalFilter, f).offset for f, _ in b.TemporalFilter._fields_] + \
           [C.sizeof(b.TfRequest)] + [getattr(b.TfRequest, f).offset for f, _ in b.TfRequest._fields_]
    assert list(map(int, got)) == want == [8, 0, 4, 48, 0, 4, 8, 12, 16, 32]
