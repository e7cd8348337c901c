"""The temporally interpolated reference on the device (-m gpu), stage by stage: thor_hip_kat_interp_stages opens an engine, uploads one reference pair per
stream and calls Engine::make_interp_frames once - k_interp_clear, k_interp_down per level, then per level from the top k_interp_estimate (one wavefront per
16x16-block row, kept two blocks behind the row above by a ticket dispenser and progress counters), k_interp_merge, k_interp_upscale, and at level 0
k_interp_mc and k_interp_pad - and copies back what the stages left in the engine's memory.  Bit-exact against the reference's common/temporal_interp.c,
recorded stage by stage (tests/golden/gen_kat12.py -> kat12*.npz).  The same fixture runs against the host build in tests/test_kat_host_interp.py: a source
error fails both, a device-only error (team_sum over 64 lanes, the row pipeline, launch geometry, blockIdx.y as the stream) fails only here.  The first
message of a failure names the first stage that differs, the level, the unit and the got / want vectors."""
import numpy as np
import pytest

import kat_interp as KI

pytestmark = pytest.mark.gpu


def _device(yuv0, yuv1, width, height, bitdepth):
    import thor_amd
    return thor_amd.binding.kat_interp_stages(yuv0, yuv1, width, height, bitdepth)


@pytest.mark.parametrize('case,bd', [(c, bd) for c in KI.CASES for bd in KI.CASES[c][3]])
def test_interp_stages_match_reference_kat(case, bd):
    """Pyramid planes with their padding of 32, nmv[0] / nmv[1] of every level, the picture area of Y, U and V and the borders of the padded output (the
    encoder searches in them); one launch sequence per pair.
    A 200x136, 3 levels: both dimensions 16 n + 8 (the last unit column and row lie outside the picture: searched with clamped coordinates, written into the
      padding before k_interp_pad overwrites it); a rectangle moving over a background that pans differently in bands - occlusion, neighbours with different
      vectors, the merge pass changes more than a tenth of the units.
    B 264x256, 4 levels, top level 33x32; a pan of (40, 24): blocks at the edges are more than the margin outside, all four branches of mot_comp_block in
      luma and chroma (both inside, only block 1, only block 0 with its row pitch, clamped).
    C 512x64, 2 levels: 32 blocks per row and 4 rows, the motion changes along and across the rows, so most blocks read an up-right neighbour that holds
      another vector than their own.  If a row of k_interp_estimate ran ahead of the two-block distance it would read a vector that is not written yet, and
      that shows here as a stage-2 difference - WHEN the timing lets it happen: this case makes such a slip visible, it cannot force it, and it is run once.
    D 64x64, 2 levels (the smallest legal size): identical frames (every block skips), flat at the maximum (every SAD ties), independent noise (the search
      runs its full budget, all units in the clamped branch).
    E 128x64: a flat area under a moving band, where the last-minimum rule of the skip vector decides (see kat_interp.CASES)."""
    KI.assert_fixture_not_trivial(bd)
    bad = []
    for pair in KI.CASES[case][4]:
        bad += KI.check(bd, [(case, pair)], _device)
    assert not bad, (len(bad), bad[:6])


def test_interp_stages_streams_of_one_launch():
    """More than one stream per launch (blockIdx.y; every stream has its own row dispenser and progress counters): the three D pairs as streams 0..2 of one
    call, each against its own recorded answer, and A at 8 bit as streams 0 and 1 of one call, both against the recorded answer."""
    bad = KI.check(8, [('D', 'same'), ('D', 'flat'), ('D', 'noise')], _device)
    bad += KI.check(8, [('A', 'scene'), ('A', 'scene')], _device)
    assert not bad, (len(bad), bad[:6])


def test_interp_stages_entry_refuses_bad_arguments():
    import ctypes as C
    import thor_amd
    L = thor_amd.lib()
    z = np.zeros(64 * 64 * 3, dtype=np.uint16)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = dict(S=1, w=64, h=64, bd=8, levels=2)
    # streams 0 / 5, sizes that are no multiple of 8 or below 64, a bit depth out of range, no levels: refused before anything is read
    for k, v in (('S', 0), ('S', 5), ('w', 60), ('h', 68), ('w', 56), ('h', 32), ('bd', 7), ('bd', 13), ('levels', 0), ('levels', 5)):
        a = dict(ok, **{k: v})
        assert L.thor_hip_kat_interp_stages(a['S'], P(z), P(z), a['w'], a['h'], a['bd'], a['levels'], P(z), P(z), P(z)) == 1, (k, v)
    assert L.thor_hip_kat_interp_stages(1, None, P(z), 64, 64, 8, 2, P(z), P(z), P(z)) == 1
    # a level count that is not the engine's for this size (64x64 has 2): refused after the engine is opened, before anything is written
    assert L.thor_hip_kat_interp_stages(1, P(z), P(z), 64, 64, 8, 3, P(z), P(z), P(z)) == 2
