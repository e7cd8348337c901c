"""The temporally interpolated reference (thor_amd/csrc/tk_interp_dev.h) in the 1-lane HOST build against the reference's common/temporal_interp.c, stage by
stage (tests/golden/kat12*.npz, recorded by tests/golden/gen_kat12.py through oracle/interp_shim.c) - the CPU twin of tests/test_gpu_interp.py: with the same
fixture a source error fails both, a device-only error (team_sum over 64 lanes, the row pipeline of k_interp_estimate, launch geometry, the streams of one
launch) only the GPU test.  Everything is compared bit-exactly, in the order the stages run, and the first message names the stage that broke."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kat_interp as KI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('kat_host_interp') / 'kat_host_interp.so')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-pthread', '-shared', '-fPIC', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_interp.cpp')])
    H = C.CDLL(so)
    H.h_interp_stages.restype = C.c_int

    def run(yuv0, yuv1, width, height, bitdepth):
        T = KI.pix(bitdepth)
        a = np.ascontiguousarray(yuv0, dtype=T); b = np.ascontiguousarray(yuv1, dtype=T)
        S = len(a)
        levels, n_pyr, n_mv, n_out = KI.stage_sizes(width, height)
        pyr = np.zeros((S, n_pyr), dtype=T); nmv = np.zeros((S, n_mv), dtype=np.int16); out = np.zeros((S, n_out), dtype=T)
        rc = H.h_interp_stages(S, P(a), P(b), width, height, bitdepth, levels, P(pyr), P(nmv), P(out))
        assert rc == 0, rc
        return pyr, nmv, out
    return run


@pytest.mark.parametrize('bd', [8, 10, 12])
def test_interp_stages_host_build_match_reference_kat(host, bd):
    """Pyramid planes with their padding, nmv[0] / nmv[1] of every level, the picture and the borders of the padded output, every case of this bit depth:
    A 200x136 (3 levels, last unit column and row outside the picture, a rectangle moving over a panning background: occlusion, different vectors next to each
    other), B 264x256 (4 levels, top level 33x32, a pan of (40, 24): all four branches of mot_comp_block in luma and chroma), C 512x64 (2 levels, 32 blocks per
    row, motion changing along and across the rows), D 64x64 (2 levels; identical frames: every block skips; flat at the maximum: ties everywhere; independent
    noise: the full search budget), E 128x64 (a flat area under a moving band: the last-minimum rule of the skip vector)."""
    KI.assert_fixture_not_trivial(bd)
    bad = []
    for case, pair in KI.pairs_of(bd):
        bad += KI.check(bd, [(case, pair)], host)
    assert not bad, (len(bad), bad[:6])


def test_interp_stages_host_build_streams_of_one_call(host):
    """The three D pairs as the streams of one call, each against its own answer, and A twice as streams 0 and 1: the jobs of one run_interp share nothing."""
    bad = KI.check(8, [('D', 'same'), ('D', 'flat'), ('D', 'noise')], host)
    bad += KI.check(8, [('A', 'scene'), ('A', 'scene')], host)
    assert not bad, (len(bad), bad[:6])
