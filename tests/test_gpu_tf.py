"""The temporal noise filter on the device (-m gpu): k_tf_search / k_tf_blend against the numpy model (tests/tf_model.py) on the cases of the host twin, one
call with the requests of several streams against the same requests one by one, the command-line tool against the recorded hashes, frames staged from NV12
in device memory, and a refused call.  Every comparison is exact."""
import json
import os
import subprocess
import sys
import tempfile
import numpy as np
import pytest
from util import ROOT, GOLD, golden_clip, md5
import frame_layout as fl
import tf_model as tm

pytestmark = pytest.mark.gpu
TS = json.load(open(os.path.join(GOLD, 'tf_streams.json')))
TOOL = os.path.join(ROOT, 'tools', 'thorenc_hip')
W, H, N = 72, 40, 5   # more than one tile per axis, no multiple of the tile


@pytest.mark.parametrize('w,h,depth,content,nrefs', list(tm.kat_cases()))
def test_device_matches_the_model(w, h, depth, content, nrefs):
    import thor_amd
    cur, refs, dists = tm.kat_case(w, h, depth, content, nrefs)
    wp, wmv, wwb = tm.filter_frame(cur, refs, dists, depth, tm.STRENGTH)
    gp, gmv, gwb = thor_amd.kat_temporal_filter(cur, refs, dists, depth, tm.STRENGTH)
    assert np.array_equal(gmv, wmv), 'vectors'
    assert np.array_equal(gwb, wwb), 'wb'
    for p in range(3):
        assert np.array_equal(gp[p], wp[p]), 'plane %d' % p


def clip_frames(seed, depth=8):
    return tm.split_frames(golden_clip('gen:%d,%d,%d,%d,6.0%s' % (W, H, N, seed, ',%d' % depth if depth > 8 else '')), W, H, N, depth)


def flat(frame):
    return np.concatenate([np.ascontiguousarray(p).ravel() for p in frame])


def params(depth=8):
    import thor_amd
    return thor_amd.load_config(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), width=W, height=H, qp=32, f=30, bitdepth=depth, input_bitdepth=depth)


# requests: (stream, dst_slot, slot, [(ref_slot, ref_dist)]): three streams, two frames of stream 0, and stream 0's second request has the first one's source
# as a neighbour (and the other way round)
REQUESTS = [(0, 8, 2, [(1, 1), (0, 2), (3, 1), (4, 2)]), (0, 9, 3, [(2, 1), (4, 1)]), (1, 8, 0, [(1, 1), (2, 2)]), (2, 5, 4, [])]


def test_one_call_equals_the_requests_one_by_one():
    import thor_amd
    clips = [clip_frames(31 + s) for s in range(3)]
    got = []
    for batched in (True, False):
        with thor_amd.Encoder(params(), 3) as enc:
            for s in range(3):
                for f in range(N):
                    enc.stage(s, f, flat(clips[s][f]))
            if batched:
                enc.filter_staged(REQUESTS, thor_amd.TemporalFilter(6))
            else:
                for r in REQUESTS:
                    enc.filter_staged([r], thor_amd.TemporalFilter(6))
            got.append([enc.staged(r[0], r[1]) for r in REQUESTS])
    for (s, _, slot, refs), a, b in zip(REQUESTS, got[0], got[1]):
        assert np.array_equal(a, b)
        want = tm.filter_frame(clips[s][slot], [clips[s][k] for k, _ in refs], [d for _, d in refs], 8, 6)[0]
        assert np.array_equal(a, flat(want))
    assert np.array_equal(got[0][3], flat(clips[2][4]))   # nrefs = 0 copies the frame


def run_tool(name, env=None):
    c = TS[name]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
        cmd = [TOOL, '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', str(c['w']), '-height', str(c['h']), '-qp', str(c['qp']),
               '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv'), '-tf_strength', str(c['strength']),
               '-tf_past', str(c['past']), '-tf_future', str(c['future'])] + c['extra']
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=120, env=dict(os.environ, **(env or {})))
        return open(os.path.join(d, 'o.bit'), 'rb').read(), open(os.path.join(d, 'o.yuv'), 'rb').read()


@pytest.mark.parametrize('name,kernel', [('ldb_8bit', 'std'), ('ldb_8bit', 'wide'), ('ra_10bit', None)])
def test_tool_reproduces_the_recorded_hashes(name, kernel):
    bits, rec = run_tool(name, {'THOR_HIP_KERNEL': kernel} if kernel else None)
    assert len(bits) == TS[name]['bit_bytes'] and md5(bits) == TS[name]['bit_md5'] and md5(rec) == TS[name]['rec_md5']


_NV12_CHILD = r'''
import sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import thor_amd
import frame_layout as fl
import tf_model as tm
import test_gpu_tf as t
frames = t.clip_frames(41)
g = fl.Geometry(t.W, t.H, 8, fl.UV, 0, 256, 256)
lay = thor_amd.FrameLayout(**g.fields)
dev = torch.from_numpy(np.stack([fl.pack(t.flat(f), g) for f in frames])).cuda()
torch.cuda.synchronize()
with thor_amd.Encoder(t.params(), 1) as enc:
    for f in range(t.N):
        enc.stage_device(0, f, dev[f].data_ptr(), lay)
    enc.filter_staged([(0, t.N, 2, [(1, 1), (0, 2), (3, 1), (4, 2)])], thor_amd.TemporalFilter(6))
    got = enc.staged(0, t.N)
want = tm.filter_frame(frames[2], [frames[1], frames[0], frames[3], frames[4]], [1, 2, 1, 2], 8, 6)[0]
assert np.array_equal(got, t.flat(want)), 'filtered NV12-staged frame differs from the model on the planar frames'
print('equal')
'''


def test_frames_staged_from_nv12_in_device_memory():
    """In a process of its own: the tensor's runtime has to start before the library's."""
    code = _NV12_CHILD % {'root': ROOT, 'tests': os.path.join(ROOT, 'tests')}
    r = subprocess.run(['timeout', '-k', '10', '120', sys.executable, '-c', code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.split()[-1:] == ['equal'], (r.returncode, r.stderr[-2000:])


def test_refused_call_leaves_the_destination_as_it_was():
    import thor_amd
    frames = clip_frames(43, 10)
    with thor_amd.Encoder(params(10), 1) as enc:
        for f in range(3):
            enc.stage(0, f, flat(frames[f]))
        before = enc.staged(0, 2).copy()
        T = thor_amd.TemporalFilter
        for reqs, tf in (([(0, 2, 1, [(0, 1)]), (0, 2, 0, [])], T(6)),        # two requests with one destination
                         ([(0, 2, 1, [(2, 1)])], T(6)),                       # the destination is a neighbour
                         ([(0, 2, 1, [(0, 3)])], T(6)),                       # ref_dist 3
                         ([(0, 2, 1, [(7, 1)])], T(6)),                       # a neighbour that is not staged
                         ([(0, 2, 1, [(0, 1)])], T(17))):                     # a refused strength
            with pytest.raises(ValueError):
                enc.filter_staged(reqs, tf)
            assert np.array_equal(enc.staged(0, 2), before)
        with pytest.raises(ValueError):
            enc.filter_staged([(0, 9, 1, [(0, 3)])], T(6))
        with pytest.raises(ValueError):
            enc.staged(0, 9)                                                  # a refused call allocates no slot either
        enc.filter_staged([(0, 2, 1, [(0, 1)])], T(6))
        assert not np.array_equal(enc.staged(0, 2), before)
