"""CDEF on the device (-m gpu).  (1) The strength search and frame filter as the encoder launches them - thor_hip_kat_cdef_frame fills CdefJobs like
Engine::finish_frames and calls backend::run_cdef once: copy, flags, direction / variance, k_cdef_mse (wavefront form: LDS row pitch, packed dot products,
four wavefronts per workgroup), k_cdef_select (1024 threads) and the apply pass - bit-exact against the reference's cdef_search + cdef_frame
(tests/golden/gen_kat10.py -> kat10.npz), all cases of one (size, bitdepth) group as the jobs of ONE launch sequence (blockIdx.y).  The same fixture runs
against the host build in tests/test_kat_host_cdef.py: a source error fails both, a device-only error fails only here.  (2) Whole encodes at -cdef 1 and
-cdef 3 through the C ABI against tests/golden/streams_cdef.json, the 8-bit ones through all three builds of the superblock kernel.
Measured on the MI355X: see tests/README.md."""
import json
import os
import numpy as np
import pytest
import kat_cdef
from util import ROOT, GOLD, golden_clip, md5

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(GOLD, 'streams_cdef.json')))


def _device(rec, org, mode, width, height, qp, speed, cdef_bits, bitdepth):
    import thor_amd
    return thor_amd.binding.kat_cdef_frame(rec, org, mode, width, height, qp, speed, cdef_bits, bitdepth)


@pytest.mark.parametrize('bd', [8, 10, 12])
def test_cdef_search_and_frame_match_reference_kat(bd):
    """dir / var of the live filter blocks, every mse entry below the speed's number of strengths, nb_bits, sb_count, the header strengths, each filter
    block's preset through the pair it selects, and every sample of the filtered frame: 200x136 (filter blocks 8 wide and 8 tall: no chroma block there; at
    8 bit two jobs of equal speed and bits with different content and skip maps), 208x120 (16 wide: one chroma column; 56 tall: 3 chroma rows), 72x72,
    128x64; speeds 0 / 1 / 2 (64 / 32 / 16 strengths) with 3 / 2 / 1 bits; fixed strengths at qp 20 / 30 / 44; about 30 % skipped blocks, everything
    skipped (sb_count 0), only the partial corner filter block live; textured, flat (ties, variance 0), checkerboard and - 8 and 12 bit - saturated content."""
    kat_cdef.assert_fixture_not_trivial(bd)
    bad = []
    for g in kat_cdef.groups(bd):
        bad += kat_cdef.check(bd, g, _device)
    assert not bad, (len(bad), bad[:8])


def test_cdef_frame_entry_refuses_bad_arguments():
    import thor_amd
    w, h, rec, org, mode, case = kat_cdef.group(8, 2)
    ok = dict(rec=rec[:1], org=org[:1], mode=mode[:1], width=w, height=h, qp=[32], speed=[1], cdef_bits=[3], bitdepth=8)
    for k, v in (('speed', [3]), ('speed', [-1]), ('cdef_bits', [4]), ('cdef_bits', [-1]), ('qp', [52]), ('qp', [-1]), ('bitdepth', 13)):
        with pytest.raises(RuntimeError, match='rc=1'):
            thor_amd.binding.kat_cdef_frame(**dict(ok, **{k: v}))
    L = thor_amd.lib()
    z = np.zeros(64, dtype=np.int32)
    P = lambda a: a.ctypes.data_as(__import__('ctypes').c_void_p)
    for bw, bh in ((4, 8), (8, 0), (12, 8), (8, 20)):   # not multiples of 8, or smaller than one block: refused before anything is read
        assert L.thor_hip_kat_cdef_frame(1, P(z), P(z), P(z), bw, bh, 8, P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(z)) == 1, (bw, bh)


def encode_gpu(clip, w, h, n, qp, cfg, **over):
    import thor_amd
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', cfg), width=w, height=h, qp=qp, f=30, **over)
    fsz = w * h * 3 // 2 * (2 if int(over.get('bitdepth', 8)) > 8 else 1)
    a = np.frombuffer(clip, dtype=np.uint8)
    with thor_amd.Encoder(p, 1) as enc:
        bits, recs = enc.encode_clips([[a[f * fsz:(f + 1) * fsz] for f in range(n)]], skips=[0], file_frames=len(a) // fsz, staggered=False)
        return bits[0], b''.join(r.tobytes() for r in recs[0] if r is not None)


@pytest.mark.parametrize('name,kernel', [(n, k) for n in sorted(G) for k in (['std'] if '10bit' in n else ['std', 'lat', 'wide'])])
def test_gpu_matches_reference_golden_at_cdef_1_and_3(name, kernel, monkeypatch):
    """-cdef 1 (all 64 lanes of the lanes-as-strengths half live, the 64x64 pair table) and -cdef 3 (16 strengths) through the C ABI: bitstream and
    reconstruction hashes of the reference; 16-bit samples have one kernel."""
    monkeypatch.setenv('THOR_HIP_KERNEL', kernel)
    c = G[name]
    ex = list(c['extra'])
    over = {ex[i][1:]: ex[i + 1] for i in range(0, len(ex), 2)}
    bits, rec = encode_gpu(golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['cfg'], **over)
    assert len(bits) == c['bit_bytes']
    assert md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'
