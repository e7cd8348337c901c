"""The CDEF strength search and frame filter (thor_amd/csrc/tk_cdef.h) in the 1-lane HOST build against the reference's cdef_search + cdef_frame
(tests/golden/kat10.npz, recorded by tests/golden/gen_kat10.py) - the CPU twin of tests/test_gpu_cdef.py: with the same fixture a source error fails both, a
device-only error (packed dot-product builtins, LDS row pitch, four wavefronts per workgroup, the 1024-thread barrier) only the GPU test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kat_cdef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('kat_host_cdef') / 'kat_host_cdef.so')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-shared', '-fPIC', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_cdef.cpp')])
    H = C.CDLL(so)
    H.h_cdef_frame.restype = C.c_int

    def run(rec, org, mode, width, height, qp, speed, cdef_bits, bitdepth):
        T = np.uint8 if bitdepth == 8 else np.uint16
        rec = np.ascontiguousarray(rec, dtype=T); org = np.ascontiguousarray(org, dtype=T); mode = np.ascontiguousarray(mode, dtype=np.uint8)
        qp, speed, cdef_bits = (np.ascontiguousarray(a, dtype=np.int32) for a in (qp, speed, cdef_bits))
        S, nfb = len(rec), ((width + 63) // 64) * ((height + 63) // 64)
        d = np.zeros((S, height // 8, width // 8), dtype=np.int8); v = np.zeros((S, height // 8, width // 8), dtype=np.int32)
        fbc = np.zeros((S, nfb), dtype=np.int32); fbs = np.zeros((S, nfb), dtype=np.int32)
        mse = np.zeros((S, 2, nfb, 64), dtype=np.uint64); res = np.zeros((S, 34), dtype=np.int32)
        out = np.zeros_like(rec)
        rc = H.h_cdef_frame(S, P(rec), P(org), P(mode), width, height, bitdepth, P(qp), P(speed), P(cdef_bits), P(d), P(v), P(fbc), P(mse), P(res), P(fbs), P(out))
        assert rc == 0, rc
        return dict(dir=d, var=v, fb_compact=fbc, fb_sel=fbs, mse=mse, nb_bits=res[:, 0], strengths=res[:, 1:9], uv_strengths=res[:, 9:17], sb_count=res[:, 17], out=out)
    return run


@pytest.mark.parametrize('bd', [8, 10, 12])
def test_cdef_search_and_frame_host_build_match_reference_kat(host, bd):
    """Flags, direction / variance, the wavefront form of the distortion pass (lanes as a loop), the joint strength selection with a one-thread team and the
    apply pass against the reference, every case of kat10.npz: 200x136 / 208x120 / 72x72 / 128x64 (filter blocks 8 wide or tall without chroma, 16 wide / 56
    tall, exact), speeds 0 / 1 / 2 with 3 / 2 / 1 bits, the fixed strengths of qp 20 / 30 / 44, random / all / all-but-the-corner skip maps, textured / flat /
    checkerboard / saturated content."""
    kat_cdef.assert_fixture_not_trivial(bd)
    bad = []
    for g in kat_cdef.groups(bd):
        bad += kat_cdef.check(bd, g, host)
    assert not bad, (len(bad), bad[:8])
