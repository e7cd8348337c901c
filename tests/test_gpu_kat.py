"""Kernel-level entry points of the C ABI vs. the oracle's C restatement and the recorded KATs (-m gpu)."""
import ctypes as C
import os
import numpy as np
import pytest
from util import GOLD, build_oracle_c, vp

pytestmark = pytest.mark.gpu
K = np.load(os.path.join(GOLD, 'kat.npz'))


def test_sad_batch_matches_reference_kat():
    import thor_amd
    plane = K['sad_plane']
    for i in range(7):
        org, cand, want = K[f'sad_org{i}'], K[f'sad_cand{i}'], K[f'sad_out{i}']
        got = thor_amd.sad_batch(org, plane, 12, 12, cand)
        assert (got == want).all(), i


def test_sad_batch_random_vs_oracle_c():
    import thor_amd
    O = build_oracle_c()
    rng = np.random.default_rng(5)
    plane = rng.integers(0, 256, size=(200, 256), dtype=np.uint8)
    for (w, h) in ((4, 8), (8, 4), (16, 16), (64, 32), (128, 128)):
        org = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        cand = rng.integers(-30, 31, size=(400, 2)).astype(np.int32)
        got = thor_amd.sad_batch(org, plane, 32, 32, cand)
        want = [O.orc_sad(vp(org), w, C.c_void_p(int(plane.ctypes.data) + (32 + int(dy)) * 256 + 32 + int(dx)), 256, w, h) for dx, dy in cand]
        assert (got == np.array(want, dtype=np.uint32)).all()


def test_interp_luma_matches_reference_kat():
    import thor_amd
    ref = K['ip_ref']
    k = 0
    while f'ip_geo{k}' in K:
        w, h, bx, by, bip = [int(v) for v in K[f'ip_geo{k}']]
        got = thor_amd.interp_luma(ref, 16, 64, 48, bx, by, w, h, K[f'ip_mv{k}'], bip)
        assert (got == K[f'ip_out{k}']).all(), k
        k += 1


def test_code_tu_matches_reference_kat():
    import thor_amd
    k = 0
    while f'tu_par{k}' in K:
        size, qp, ctype, fast = [int(v) for v in K[f'tu_par{k}']]
        coefq, rec, cbp = thor_amd.code_tu_batch(K[f'tu_org{k}'], K[f'tu_pred{k}'], qp, ctype, fast)
        assert (cbp == K[f'tu_cbp{k}']).all(), k
        assert (coefq == K[f'tu_coefq{k}']).all(), k
        assert (rec == K[f'tu_rec{k}']).all(), k
        k += 1
    assert k == 24


def test_code_tu_random_edge_cases_vs_oracle_c():
    """Extreme residuals (+-255 everywhere, checkerboards, empty) - the wave-parallel quantiser and
    transforms against the serial C restatement."""
    import thor_amd
    O = build_oracle_c()
    rng = np.random.default_rng(9)
    for size in (4, 8, 16, 32, 64):
        n = 8
        org = rng.integers(0, 256, size=(n, size, size), dtype=np.uint8)
        pred = rng.integers(0, 256, size=(n, size, size), dtype=np.uint8)
        org[0] = 255; pred[0] = 0
        org[1] = 0; pred[1] = 255
        org[2] = pred[2]
        org[3] = (np.indices((size, size)).sum(0) % 2 * 255).astype(np.uint8); pred[3] = 255 - org[3]
        for qp, ctype in ((8, 0), (30, 2), (51, 1)):
            coefq, rec, cbp = thor_amd.code_tu_batch(org, pred, qp, ctype, 0)
            q = min(size, 16)
            for i in range(n):
                cq = np.zeros((q, q), dtype=np.int16); rc = np.zeros((size, size), dtype=np.uint8)
                c = O.orc_code_tu(vp(np.ascontiguousarray(org[i])), vp(np.ascontiguousarray(pred[i])), size, qp, ctype, 0, vp(cq), vp(rc))
                assert c == cbp[i] and (cq == coefq[i]).all() and (rc == rec[i]).all(), (size, qp, i)


def test_deblock_frame_matches_reference_kat():
    """thor_hip_deblock_frame (the four k_deblock passes) against deblock_frame_y_lbd / deblock_frame_uv_lbd of the reference
    (common/common_frame.c:47,354) on recorded random frames / block data (tests/golden/gen_kat3.py)."""
    import thor_amd
    K3 = np.load(os.path.join(GOLD, 'kat3.npz'))
    k = 0
    while f'db_par{k}' in K3:
        w, h, qp = [int(v) for v in K3[f'db_par{k}']]
        got = thor_amd.deblock_frame(K3[f'db_in{k}'], w, h, qp, K3[f'db_cells{k}'])
        assert (got == K3[f'db_out{k}']).all(), (k, int((got != K3[f'db_out{k}']).sum()))
        assert (got != K3[f'db_in{k}']).sum() > 100  # the filter did something
        k += 1
    assert k == 5


# ---- 16-bit samples: the _hbd entry points against vectors recorded from the reference's _hbd functions (kat4.npz, bitdepth 10)
K4S = {10: np.load(os.path.join(GOLD, 'kat4.npz')), 12: np.load(os.path.join(GOLD, 'kat4_12.npz'))}   # round 6: the same families at bitdepth 12
K4 = K4S[10]


@pytest.mark.parametrize('bd', [10, 12])
def test_sad_batch_hbd_matches_reference_kat(bd):
    K4 = K4S[bd]
    import thor_amd
    plane = K4['sad_plane']
    for i in range(6):
        org, cand, want = K4[f'sad_org{i}'], K4[f'sad_cand{i}'], K4[f'sad_out{i}']
        got = thor_amd.sad_batch(org, plane, 12, 12, cand, bitdepth=bd)
        assert (got == want).all(), i


def test_sad_batch_hbd_random_vs_oracle_c():
    import thor_amd
    O = build_oracle_c()
    rng = np.random.default_rng(6)
    plane = rng.integers(0, 1024, size=(200, 256), dtype=np.uint16)
    for (w, h) in ((4, 8), (8, 4), (16, 16), (64, 32), (128, 128)):
        org = rng.integers(0, 1024, size=(h, w), dtype=np.uint16)
        cand = rng.integers(-30, 31, size=(200, 2)).astype(np.int32)
        got = thor_amd.sad_batch(org, plane, 32, 32, cand, bitdepth=10)
        want = [O.orc_sad16(vp(org), w, C.c_void_p(int(plane.ctypes.data) + 2 * ((32 + int(dy)) * 256 + 32 + int(dx))), 256, w, h) for dx, dy in cand]
        assert (got == np.array(want, dtype=np.uint32)).all()


@pytest.mark.parametrize('bd', [10, 12])
def test_interp_luma_hbd_matches_reference_kat(bd):
    K4 = K4S[bd]
    import thor_amd
    ref = K4['ip_ref']
    k = 0
    while f'ip_geo{k}' in K4:
        w, h, bx, by, bip = [int(v) for v in K4[f'ip_geo{k}']]
        got = thor_amd.interp_luma(ref, 16, 64, 48, bx, by, w, h, K4[f'ip_mv{k}'], bip, bitdepth=bd)
        assert (got == K4[f'ip_out{k}']).all(), k
        k += 1
    assert k == 8


@pytest.mark.parametrize('bd', [10, 12])
def test_code_tu_hbd_matches_reference_kat(bd):
    K4 = K4S[bd]
    import thor_amd
    k = 0
    while f'tu_par{k}' in K4:
        size, qp, ctype, fast = [int(v) for v in K4[f'tu_par{k}']]
        coefq, rec, cbp = thor_amd.code_tu_batch(K4[f'tu_org{k}'], K4[f'tu_pred{k}'], qp, ctype, fast, bitdepth=bd)
        assert (cbp == K4[f'tu_cbp{k}']).all(), k
        assert (coefq == K4[f'tu_coefq{k}']).all(), k
        assert (rec == K4[f'tu_rec{k}']).all(), k
        k += 1
    assert k == 24


@pytest.mark.parametrize('bd', [10, 12])
def test_code_tu_hbd_edge_cases_vs_oracle_c(bd):
    """The extremes of test_code_tu_random_edge_cases_vs_oracle_c on 16-bit samples: residuals of +-(2^bd - 1) everywhere, checkerboards between 0 and the
    maximum, empty blocks and random ones - the wave-parallel transforms and quantiser against orc_code_tu16 (pinned to the reference in tests/test_oracle_c.py)."""
    import thor_amd
    O = build_oracle_c()
    rng = np.random.default_rng(900 + bd)
    peak = (1 << bd) - 1
    for size in (4, 8, 16, 32, 64):
        n = 8
        org = rng.integers(0, peak + 1, size=(n, size, size), dtype=np.uint16)
        pred = rng.integers(0, peak + 1, size=(n, size, size), dtype=np.uint16)
        org[0] = peak; pred[0] = 0
        org[1] = 0; pred[1] = peak
        org[2] = pred[2]
        org[3] = (np.indices((size, size)).sum(0) % 2 * peak).astype(np.uint16); pred[3] = peak - org[3]
        for qp, ctype in ((8, 0), (30, 2), (51, 1)):
            coefq, rec, cbp = thor_amd.code_tu_batch(org, pred, qp, ctype, 0, bitdepth=bd)
            q = min(size, 16)
            for i in range(n):
                cq = np.zeros((q, q), dtype=np.int16); rc = np.zeros((size, size), dtype=np.uint16)
                c = O.orc_code_tu16(vp(np.ascontiguousarray(org[i])), vp(np.ascontiguousarray(pred[i])), size, qp, ctype, 0, vp(cq), vp(rc), bd)
                assert c == cbp[i] and (cq == coefq[i]).all() and (rc == rec[i]).all(), (bd, size, qp, i)


@pytest.mark.parametrize('bd', [10, 12])
def test_deblock_frame_hbd_matches_reference_kat(bd):
    K4 = K4S[bd]
    import thor_amd
    k = 0
    while f'db_par{k}' in K4:
        w, h, qp = [int(v) for v in K4[f'db_par{k}']]
        got = thor_amd.deblock_frame(K4[f'db_in{k}'], w, h, qp, K4[f'db_cells{k}'], bitdepth=bd)
        assert (got == K4[f'db_out{k}']).all(), (k, int((got != K4[f'db_out{k}']).sum()))
        assert (got != K4[f'db_in{k}']).sum() > 100
        k += 1
    assert k == 3


# ---- round 6: the sample kernels that were only covered by whole-stream hashes, against vectors recorded from the reference functions
# (tests/golden/gen_kat5.py -> kat5.npz; bitdepth 8 = the _lbd instances, 10 / 12 = _hbd) ------------------------------------------------
K5 = np.load(os.path.join(GOLD, 'kat5.npz'))
BDS = [8, 10, 12]


@pytest.mark.parametrize('bd', BDS)
def test_intra_prediction_matches_reference_kat(bd):
    """make_top_and_left + get_intra_prediction (common/intra_prediction.c:57-183, :403-428): every mode, blocks of 4..32 at the frame corner / top row /
    left column / interior with and without up-right / down-left samples, and the four transform units of split blocks (edges from the block-local
    reconstruction)."""
    import thor_amd
    plane = K5[f'in{bd}_plane']
    k = 0
    while f'in{bd}_geo{k}' in K5:
        size, tb = [int(v) for v in K5[f'in{bd}_geo{k}']]
        got = thor_amd.binding.kat_intra(plane, size, K5[f'in{bd}_par{k}'], bd, K5[f'in{bd}_rb{k}'] if tb else None)
        want = K5[f'in{bd}_out{k}']
        bad = [i for i in range(len(want)) if (got[i] != want[i]).any()]
        assert not bad, (k, size, tb, [K5[f'in{bd}_par{k}'][i].tolist() for i in bad[:4]])
        k += 1
    assert k == 7


@pytest.mark.parametrize('bd', BDS)
def test_inter_prediction_yuv_matches_reference_kat(bd):
    """get_inter_prediction_yuv (common/inter_prediction.c:185-226): clip_mv, quarter-pel luma, eighth-pel chroma (the `sic` clamp of :78), one PU and
    four quadrant PUs, vectors far outside the frame."""
    import thor_amd
    W, H = [int(v) for v in K5[f'ip{bd}_geo']]
    k = 0
    while f'ip{bd}_size{k}' in K5:
        size = int(K5[f'ip{bd}_size{k}'][0])
        got = thor_amd.binding.kat_inter_yuv(K5[f'ip{bd}_yuv'], W, H, size, K5[f'ip{bd}_par{k}'], K5[f'ip{bd}_mv{k}'], bd)
        want = K5[f'ip{bd}_out{k}']
        bad = [i for i in range(len(want)) if (got[i] != want[i]).any()]
        assert not bad, (k, size, [(K5[f'ip{bd}_par{k}'][i].tolist(), K5[f'ip{bd}_mv{k}'][i].tolist()) for i in bad[:3]])
        k += 1
    assert k == 4


@pytest.mark.parametrize('bd', BDS)
def test_average_blocks_matches_reference_kat(bd):
    import thor_amd
    for k, size in enumerate((8, 32)):
        got = thor_amd.binding.kat_average(K5[f'av{bd}_a{k}'], K5[f'av{bd}_b{k}'], size, bd)
        assert (got == K5[f'av{bd}_out{k}']).all(), k


@pytest.mark.parametrize('bd', BDS)
def test_chroma_from_luma_matches_reference_kat(bd):
    """improve_uv_prediction (common/common_block.c:347-428): items with a good luma prediction (untouched), correlated and uncorrelated chroma."""
    import thor_amd
    k = 0
    while f'cf{bd}_n{k}' in K5:
        n = int(K5[f'cf{bd}_n{k}'][0])
        got = thor_amd.binding.kat_cfl(K5[f'cf{bd}_y{k}'], K5[f'cf{bd}_uv{k}'], K5[f'cf{bd}_ry{k}'], n, bd)
        assert (got == K5[f'cf{bd}_out{k}']).all(), (k, n)
        assert (K5[f'cf{bd}_out{k}'] != K5[f'cf{bd}_uv{k}']).any()
        k += 1
    assert k == 4


@pytest.mark.parametrize('bd', BDS)
def test_cdef_direction_and_filter_match_reference_kat(bd):
    """cdef_find_dir (common/common_block.c:94-162) and cdef_filter_block (:224-279; recorded from the SIMD kernel the binary executes): 8x8 luma and 4x4
    chroma blocks, frame corners (CDEF_VERY_LARGE taps), every direction, primary / secondary strengths and dampings."""
    import thor_amd
    d, v = thor_amd.binding.kat_cdef_dir(K5[f'cd{bd}_blocks'], bd)
    assert (d == K5[f'cd{bd}_dir']).all() and (v == K5[f'cd{bd}_var']).all()
    assert len(set(d.tolist())) == 8
    for k, bsize in enumerate((8, 4)):
        got = thor_amd.binding.kat_cdef_filter(K5[f'cd{bd}_plane'], bsize, K5[f'cd{bd}_fpar{k}'], bd)
        want = K5[f'cd{bd}_fout{k}']
        bad = [i for i in range(len(want)) if (got[i] != want[i]).any()]
        assert not bad, (bsize, [K5[f'cd{bd}_fpar{k}'][i].tolist() for i in bad[:4]])


@pytest.mark.parametrize('bd', BDS)
def test_clpf_statistics_and_filter_match_reference_kat(bd):
    """CLPF: the per-block squared errors of detect_multi_clpf and the frame filtered by clpf_block under clpf_frame's skip / filter-block / boundary rules."""
    import thor_amd
    W, H, qp, fb_log2, s0, s1, s2 = [int(v) for v in K5[f'cl{bd}_par']]
    stats, out = thor_amd.binding.kat_clpf(K5[f'cl{bd}_rec'], K5[f'cl{bd}_org'], W, H, qp, K5[f'cl{bd}_cells'], [s0, s1, s2], fb_log2, K5[f'cl{bd}_fb_on'], bd)
    assert (stats == K5[f'cl{bd}_stats']).all(), np.argwhere(stats != K5[f'cl{bd}_stats'])[:4].tolist()
    assert (out == K5[f'cl{bd}_out']).all(), int((out != K5[f'cl{bd}_out']).sum())
    assert (out != K5[f'cl{bd}_rec']).sum() > 500


@pytest.mark.parametrize('bd', [8, 10])
def test_interpolate_frames_matches_reference_kat(bd):
    """interpolate_frames(new, ref0, ref1, 2, 1) (common/temporal_interp.c:909) on a panned 192x128 pair: the device pyramid / block motion estimation /
    merge / motion-compensated average against the reference's frame, luma and chroma."""
    import thor_amd
    W, H = [int(v) for v in K5[f'it{bd}_geo']]
    got = thor_amd.binding.kat_interpolate(K5[f'it{bd}_a'], K5[f'it{bd}_b'], W, H, bd)
    want = K5[f'it{bd}_out']
    assert (got == want).all(), int((got != want).sum())


# ---- the motion search and the early-skip sub-block tests on the device (throughput build; the latency and the eight-wave build of the superblock kernel stay
# covered by the stream goldens): known answers of the reference's motion_estimate / motion_estimate_bi (tests/golden/gen_kat8.py -> kat8.npz) and of its
# check_early_skip_sub_block / _sub_blockC (gen_kat7.py -> kat7.npz) ----------------------------------------------------------------------------------------
K8 = np.load(os.path.join(GOLD, 'kat8.npz'))
ME_PAR = 'cb_x cb_y cb pu_dx pu_dy pw ph mvc.x mvc.y mvp.x mvp.y sign bipred speed ncand cand_off stage'.split()


def me_failures(got, want, par, lam, lgot=None, lwant=None):
    """The first failing items with their parameters plus got / want vector and cost."""
    bad = np.flatnonzero((got != want).any(axis=1) | (False if lgot is None else (lgot != lwant).any(axis=(1, 2))))
    rows = [f'{len(bad)} of {len(want)} items differ']
    for i in bad[:6]:
        rows.append(f'item {i}: ' + ' '.join(f'{k}={int(v)}' for k, v in zip(ME_PAR, par[i])) + f' lambda={lam[i]} got mv ({got[i][0]}, {got[i][1]}) cost {got[i][2]} want mv ({want[i][0]}, {want[i][1]}) '
                    f'cost {want[i][2]}' + ('' if lgot is None or (lgot[i] == lwant[i]).all() else f' list got {lgot[i].tolist()} want {lwant[i].tolist()}'))
    return len(bad), '\n'.join(rows)


@pytest.mark.parametrize('bd', [8, 10])
def test_motion_estimate_matches_reference_kat(bd):
    """motion_estimate on the device (one launch, one wavefront per item, the superblock kernel's workspace and LDS search window): the LDS window per PU and
    per CB (me_stage_cb_window), the lane-per-candidate evaluators me_cand_fullpel / me_cand8_subpel / me_cand16_subpel, the 64-lane row-segment evaluator
    (PUs of 64 and 128 samples), eval_wide, grid and list de-duplication, the hexagon, the half- and quarter-pel passes and the encoder_speed 1 / 2
    approximations against the reference's vector and cost, every item, bit-exact.  The speed-1 16x16 telescope items and the 16x16 list items pin eval_wide
    against the reference's widesad_calc, ties included."""
    import thor_amd
    par, lam, want = K8[f'me{bd}_par'], K8[f'me{bd}_lam'], K8[f'me{bd}_out']
    wide = (par[:, 2] == 16) & ((par[:, 14] > 0) | ((par[:, 13] == 1) & (par[:, 12] == 1)))
    assert wide.sum() >= 100 and len(par) >= 600
    got = thor_amd.binding.kat_motion_estimate(K8[f'f{bd}_cur'], K8[f'f{bd}_ref'], par, lam, K8[f'me{bd}_cand'], bd)
    nbad, rep = me_failures(got, want, par, lam)
    assert nbad == 0, rep


@pytest.mark.parametrize('bd', [8, 10])
def test_motion_estimate_bi_matches_reference_kat(bd):
    """motion_estimate_bi on the device: vector, cost and the candidate list as the call leaves it (slots num..3 zero-filled, 4 and 5 overwritten), CBs 8 .. 64,
    both signs, blocks whose vector the second clip changes."""
    import thor_amd
    par, lam, want, lwant = K8[f'bi{bd}_par'], K8[f'bi{bd}_lam'], K8[f'bi{bd}_out'], K8[f'bi{bd}_list']
    assert len(par) >= 100
    got, lgot = thor_amd.binding.kat_motion_estimate_bi(K8[f'f{bd}_cur'], K8[f'f{bd}_ref'], K8[f'f{bd}_ref1'], par, lam, K8[f'bi{bd}_cand'], bd)
    nbad, rep = me_failures(got, want, par, lam, lgot, lwant)
    assert nbad == 0, rep


def test_early_skip_sub_block_tests_match_reference_kat():
    """early_skip_sub / early_skip_subC (tk_block.h) on the device against the 288 answers of kat7.npz (luma 8 / 16 / 32, chroma 4 / 8 / 16, three qp, two
    thresholds, residuals around the decision boundary)."""
    import thor_amd
    K7 = np.load(os.path.join(GOLD, 'kat7.npz'))
    arg, want = K7['es_arg'], K7['es_out']
    assert len(want) == 288
    got = thor_amd.binding.kat_early_skip(arg[:, 0], K7['es_org'], K7['es_pred'], arg[:, 1], arg[:, 2], arg[:, 3] / 10.0, 8)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), [(int(i), arg[i].tolist(), int(got[i]), int(want[i])) for i in bad[:6]])


# ---- the block syntax writer and its bit counter on the device (thor_amd/csrc/tk_bits.h through thor_hip_kat_coeff_syntax / thor_hip_kat_block_syntax, one launch
# per test) against the reference's bit strings (tests/golden/gen_kat9.py -> kat9.npz), and k_gather_bits ---------------------------------------------------------
def test_coeff_syntax_matches_reference_kat():
    """write_coeff, every coefficient item of kat9.npz: coeff_bits_team<SP_LDS> and <SP_GLOBAL> (the 64-lane ballot automaton with its carries across rounds)
    equal the reference length; bs_coeff on one lane and bs_coeff_team on 64 lanes (the readlane form that only exists on the device) write the reference
    string at start offsets 0, 1, 31, 32, 33, 63, 17 and leave the bits before the offset as they were."""
    import thor_amd
    import kat_bits as B
    want = B.strings('co')
    n = len(want)
    assert n >= 2000
    par = np.zeros((n, 4), dtype=np.int32)
    par[:, :2] = B.K9['co_par']; par[:, 2] = [(0, 1, 31, 32, 33, 63, 17)[i % 7] for i in range(n)]; par[:, 3] = B.CO_WORDS * 32
    fill = np.full((n, B.CO_WORDS), B.FILL, dtype=np.uint32)
    out, b1, bt = thor_amd.binding.kat_coeff_syntax(par, B.K9['co_coef'], B.CO_WORDS, fill, fill)
    fill_bits = B.word_bits(fill[:1])[0]
    bad = [f'coeff_bits_team item {i} (size {par[i, 0]} type {par[i, 1]}): {out[i, :2].tolist()} want {len(w)}' for i, w in enumerate(want) if not (out[i, 0] == out[i, 1] == len(w))]
    bad += B.check_emitted('bs_coeff', B.word_bits(b1), out[:, 2], out[:, 3], want, par[:, 2], fill_bits)
    bad += B.check_emitted('bs_coeff_team', B.word_bits(bt), out[:, 4], out[:, 5], want, par[:, 2], fill_bits)
    assert not bad, f'{len(bad)} failures:\n' + '\n'.join(bad[:8])


def test_block_syntax_matches_reference_kat():
    """write_block and write_super_mode, every item of kat9.npz, plus every recorded put_vlc codeword and write_mv string as items of their own: bs_block_head_t,
    bs_block_t<false, SP_LDS / SP_GLOBAL> without and with ybits equal the reference length (SP_LDS: where the product keeps the chroma buffers in LDS), the
    cooperative and the single-lane emission equal the reference string."""
    import thor_amd
    import kat_bits as B
    rows, want, head = B.all_rows()
    assert len(rows) >= 6000 and (rows[:, 0] == 0).sum() >= 1400 and ((rows[:, 0] == 0) & (rows[:, 25] == 1) & (rows[:, 9] >= 64)).sum() >= 40
    out, bc, b1 = thor_amd.binding.kat_block_syntax(rows, B.K9['co_coef'], B.BL_WORDS, B.FILL)
    bad = B.check_block_out(out, rows, want, head)
    bad += B.check_emitted('cooperative emission', B.word_bits(bc), out[:, 5], out[:, 6], want)
    bad += B.check_emitted('single-lane emission', B.word_bits(b1), out[:, 7], out[:, 8], want)
    assert not bad, f'{len(bad)} failures:\n' + '\n'.join(bad[:8])


def test_gather_bits_matches_numpy_concatenation():
    """k_gather_bits: 64 strings of 1 .. 3000 bits from an arbitrary first bit, most back to back (so string ends land mid-word and, for the strings sized to it, on
    word boundaries), four after a gap of zero bits (7 bits, two whole words, 45 bits, up to a word boundary plus a word), the source words filled with set bits beyond nbits (the tail mask), against a numpy bit concatenation."""
    import thor_amd
    rng = np.random.default_rng(64)
    nbits = rng.integers(1, 3001, 64)
    nbits[:4] = (1, 31, 32, 3000)
    pos, dst_bit = 13, []
    for i in range(64):
        if i % 5 == 4: nbits[i] += (-(pos + nbits[i])) % 32      # this string ends on a word boundary, the next one starts on it
        pos += {10: 7, 20: 64, 30: 45, 40: 32 + (-pos) % 32}.get(i, 0)   # four strings start after a gap: a few bits, whole words, and onto a word boundary
        dst_bit.append(pos); pos += int(nbits[i])
    assert nbits.max() <= 3031 and sum((d + n) % 32 == 0 for d, n in zip(dst_bit, nbits)) >= 12
    src_off = np.concatenate([[0], np.cumsum((nbits + 31) // 32)])
    src = rng.integers(0, 1 << 32, int(src_off[-1]), dtype=np.uint64).astype(np.uint32)
    sbits = np.unpackbits(src.astype('>u4').view(np.uint8))
    want = np.zeros(32 * ((pos + 31) // 32 + 1), dtype=np.uint8)
    for i in range(64):
        o = 32 * int(src_off[i])
        want[dst_bit[i]:dst_bit[i] + nbits[i]] = sbits[o:o + nbits[i]]
        if nbits[i] % 32: src[src_off[i + 1] - 1] |= np.uint32((1 << (32 - nbits[i] % 32)) - 1)   # garbage behind the string in its last word
    got = thor_amd.binding.kat_gather_bits(src, src_off[:-1], nbits, dst_bit, len(want) // 32)
    gbits = np.unpackbits(got.astype('>u4').view(np.uint8))
    assert np.array_equal(gbits, want), f'first differing bit {int(np.flatnonzero(gbits != want)[0])}'


def test_engine_only_codewords_longer_than_32_bits():
    """Engine-only property, no reference comparison: levels up to 32767 take the len > 32 branch of bs_vlc_t; emitted length = counted length, and the string is
    len - k zeros followed by the k significant bits of the code (kat_bits.vlc_code), for bs_coeff and bs_coeff_team on the device."""
    import thor_amd
    import kat_bits as B
    B.check_long_codewords(lambda par, coef, b1, bt: thor_amd.binding.kat_coeff_syntax(par, coef, B.CO_WORDS, b1, bt))


def test_engine_only_overflow_keeps_position_and_canaries():
    """Engine-only property: with a capacity shorter than the string ovf is set, pos still advances to the full length, and the words from the capacity on are
    unchanged, for bs_coeff and bs_coeff_team on the device."""
    import thor_amd
    import kat_bits as B
    B.check_overflow(lambda par, coef, b1, bt: thor_amd.binding.kat_coeff_syntax(par, coef, B.CO_WORDS, b1, bt))


# ---- the layer between the sample kernels and the stream on the device: the neighbour context of a coding block (tk_block_ctx.h) and the block cost (tk_block_rd.h:
# ssd_part, ssd_total, rd_cost) against the reference's own answers (tests/golden/gen_kat11.py -> kat11.npz), one launch per call --------------------------------
def test_block_context_matches_reference_kat():
    """upright_avail, downleft_avail, get_mv_pred, get_mv_cands and find_contexts on the device, one wavefront per item, at EVERY block position of three frames
    whose sizes are no multiples of the superblock (200x136, 328x264, 264x40), superblocks of 64 and 128, sizes 8..128, on random cell grids with areas of equal
    predictions: bit-exact against get_mv_pred_lbd, get_mv_skip_lbd and get_mv_merge_lbd (the generator asserts that the two return the same on every item, so
    the one recorded answer is both call sites'), find_block_contexts_lbd with enable 0 / 1 and the two availability functions."""
    import thor_amd
    from kat_block import K11, ctx_report
    total = 0
    for fi in range(3):
        par, want = K11[f'ctx{fi}_par'].astype(np.int32), K11[f'ctx{fi}_out'].astype(np.int32)
        got = thor_amd.binding.kat_block_ctx(K11[f'ctx{fi}_cells'], int(par[0][3]) // 4, par)
        rep = ctx_report(got, want, par)
        assert rep is None, f'frame {fi}: {rep}'
        total += len(par)
    assert total >= 5000


@pytest.mark.parametrize('bd', [8, 10, 12])
def test_block_cost_matches_reference_kat(bd):
    """ssd_total(ssd_part()) of the luma plane - the SP_GLOBAL instance on an original with the item's byte skew and stride (the 16 / 8 / 4 byte row loops on
    v_dot4 / v_dot2 and the per-sample loops, power-of-two and other widths), the SP_LDS instance for blocks up to the size the build keeps in LDS - against a numpy int64 sum, and rd_cost
    (three planes, 64-lane reduction, rate term, 2^30 clamp; with and without the luma SSD passed in) against the reference's cost_calc: sizes 8..128, frame-edge
    rectangles, all-max against all-zero 128x128 blocks (8 bit: 1.6e9, the 32-bit headroom; 12 bit: 4e11, the 64-bit reduction), costs at and within 1000 below
    the clamp.  No tolerance."""
    import thor_amd
    from kat_block import K11, cost_want, cost_report
    par, lam = K11[f'cost{bd}_par'], K11[f'cost{bd}_lam']
    assert len(par) >= 90
    got = thor_amd.binding.kat_block_cost(par, lam, K11[f'cost{bd}_org'], K11[f'cost{bd}_rec'], bd)
    rep = cost_report(got, cost_want(bd, thor_amd.binding.kat_lds_block()), par, lam)
    assert rep is None, rep


@pytest.mark.parametrize('bd', [8, 10])
def test_intra_sad_search_matches_reference_kat(bd):
    """intra_sad_search on the device, one wavefront per item and one launch, against the reference's search_intra_prediction_params: mode and SAD (shifted by
    bitdepth - 8), bit-exact.  A 96x80 reconstructed plane; sizes 8 / 16 / 32 at the frame corner, in the top row, the left column and inside with and without
    up-right / down-left (from the position; superblocks 64 and 128); 4 and 10 modes; random originals, originals equal or close to one mode's prediction (each
    of the ten modes wins), flat blocks on the flat part of the plane, where every mode ties and the first in evaluation order must win."""
    import thor_amd
    from kat_block import K11, intra_report
    par = K11[f'intra{bd}_par']
    assert len(par) >= 300
    got = thor_amd.binding.kat_intra_search(par, K11[f'intra{bd}_plane'], K11[f'intra{bd}_org'], bd)
    rep = intra_report(got, K11[f'intra{bd}_out'], par)
    assert rep is None, rep


@pytest.mark.parametrize('bd', [8, 10, 12])
def test_build_org8_matches_numpy(bd):
    """build_org8 (the saturated 2 * org - pred of a bi-prediction search step) on the device against numpy: sizes 8..64, the four-sample path and the per-sample
    path (originals skewed by 2 bytes, strides that break the alignment), the global-memory instance and - for blocks the build keeps in LDS - the LDS instance;
    every block saturates at both ends; samples outside the items' blocks stay untouched."""
    import thor_amd
    from kat_block import org8_items, org8_report
    par, org, pred = org8_items(bd)
    og, ol = thor_amd.binding.kat_build_org8(par, org, pred, bd, fill=5)
    rep = org8_report(bd, par, org, pred, og, ol, thor_amd.binding.kat_lds_block(), 5)
    assert rep is None, rep
