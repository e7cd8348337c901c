"""Round 6: the known answers of tests/golden/kat5.npz (recorded from the reference functions, tests/golden/gen_kat5.py) against the 1-lane HOST build of the
device functions (tests/hostsim/kat_host.cpp: make_edges + pred_intra, the two CLPF passes, cdef_find_dir, cdef_filter_px) - the CPU twin of the
device known-answer tests (tests/test_gpu_kat.py), bitdepth 8 / 10 / 12.  The motion search: the known answers of tests/golden/kat8.npz (the reference's
motion_estimate / motion_estimate_bi, tests/golden/gen_kat8.py) against the host build of tk_me.h (tests/hostsim/kat_host_me.cpp), 1-lane and 64-lane teams.
The neighbour context of a coding block and the block cost: kat11.npz (tests/golden/gen_kat11.py) against tests/hostsim/kat_host_ctx.cpp, 1-lane and 8-lane teams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K5 = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat5.npz'))
P = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope='module')
def L(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('kat') / 'kat_host.so')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-shared', '-fPIC', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostsim', 'kat_host.cpp')])
    return C.CDLL(so)


@pytest.mark.parametrize('bd', [8, 10, 12])
def test_intra_host_build_matches_reference_kat(L, bd):
    plane = np.ascontiguousarray(K5[f'in{bd}_plane'])
    k = 0
    while f'in{bd}_geo{k}' in K5.files:
        size, tb = [int(v) for v in K5[f'in{bd}_geo{k}']]
        par = np.ascontiguousarray(K5[f'in{bd}_par{k}'])
        want = K5[f'in{bd}_out{k}']
        rb = np.ascontiguousarray(K5[f'in{bd}_rb{k}']) if tb else None
        out = np.zeros_like(want)
        L.h_intra(P(plane), plane.shape[1], bd, size, tb, len(par), P(par), P(rb) if tb else None, P(out))
        assert (out == want).all(), (k, size, tb)
        k += 1
    assert k == 7


@pytest.mark.parametrize('bd', [8, 10, 12])
def test_clpf_and_cdef_host_build_match_reference_kat(L, bd):
    W, H, qp, fbl, s0, s1, s2 = [int(v) for v in K5[f'cl{bd}_par']]
    rec, org = np.ascontiguousarray(K5[f'cl{bd}_rec']), np.ascontiguousarray(K5[f'cl{bd}_org'])
    cells, fb = np.ascontiguousarray(K5[f'cl{bd}_cells']), np.ascontiguousarray(K5[f'cl{bd}_fb_on'])
    nblk = (W // 8) * (H // 8) + 2 * (W // 16) * (H // 16)
    stats = np.zeros((nblk, 4), dtype=np.uint32)
    out = np.zeros_like(rec)
    st = np.array([s0, s1, s2], dtype=np.int32)
    L.h_clpf(P(rec), P(org), W, H, bd, qp, P(cells), P(st), fbl, P(fb), P(stats), P(out))
    assert (stats == K5[f'cl{bd}_stats']).all() and (out == K5[f'cl{bd}_out']).all() and (out != rec).sum() > 500
    blocks = np.ascontiguousarray(K5[f'cd{bd}_blocks'])
    d = np.zeros(len(blocks), dtype=np.int32)
    v = np.zeros(len(blocks), dtype=np.int32)
    L.h_cdef_dir(P(blocks), bd, len(blocks), P(d), P(v))
    assert (d == K5[f'cd{bd}_dir']).all() and (v == K5[f'cd{bd}_var']).all()
    plane = np.ascontiguousarray(K5[f'cd{bd}_plane'])
    for k, bsize in enumerate((8, 4)):
        par = np.ascontiguousarray(K5[f'cd{bd}_fpar{k}'])
        want = K5[f'cd{bd}_fout{k}']
        got = np.zeros_like(want)
        L.h_cdef_filter(P(plane), plane.shape[1], plane.shape[0], plane.shape[1], bd, bsize, len(par), P(par), P(got))
        assert (got == want).all(), bsize


def test_early_skip_sub_block_tests_host_build_match_reference_kat(tmp_path):
    """early_skip_sub / early_skip_subC (tk_block.h; the luma and the chroma sub-block test of check_early_skip) in the 1-lane host build against the 288 known
    answers recorded from the reference's check_early_skip_sub_block / _sub_blockC with use_simd = 1 (tests/golden/gen_kat7.py) - luma 8 / 16 / 32, chroma 4 / 8 / 16
    (incl. the 4-wide column-pair form of calc_cbp_simd), three qp, two thresholds, residuals around the decision boundary."""
    so = str(tmp_path / 'kat_host_es.so')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-shared', '-fPIC', '-o', so,
                           os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_es.cpp')])
    H = C.CDLL(so)
    H.h_early_skip_sub.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]
    K7 = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat7.npz'))
    org, pred, arg, want = (np.ascontiguousarray(K7[k]) for k in ('es_org', 'es_pred', 'es_arg', 'es_out'))
    for k in range(len(want)):
        chroma, size, qp, thr10 = (int(v) for v in arg[k])
        got = H.h_early_skip_sub(chroma, P(org[k]), 32, P(pred[k]), 32, size, qp, thr10 / 10.0, 8)
        assert got == int(want[k]), (k, chroma, size, qp, thr10, got, int(want[k]))


# ---- the motion search: motion_estimate / motion_estimate_bi / me_stage_cb_window (thor_amd/csrc/tk_me.h) against the reference's own answers ---------------------
K8 = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat8.npz'))
ME_PAD = 160   # kPadY: the replicate padding of a reference picture (k_make_ref)
ME_PAR = 'cb_x cb_y cb pu_dx pu_dy pw ph mvc.x mvc.y mvp.x mvp.y sign bipred speed ncand cand_off stage'.split()


def me_planes(bd):
    """cur, ref0, ref1 with the replicate padding, and the offset (in samples) of sample (0, 0)."""
    pl = [np.ascontiguousarray(np.pad(K8[f'f{bd}_{k}'], ME_PAD, mode='edge')) for k in ('cur', 'ref', 'ref1')]
    return pl, ME_PAD * pl[0].shape[1] + ME_PAD


def me_host_batch(lib, bd, lanes, bi, sel=None):
    """Vector, cost (and list afterwards) of the items `sel` (default: all) of kat8.npz from the host build; returns (got, want, list_got, list_want, par)."""
    pre = ('bi' if bi else 'me') + str(bd)
    par, lam, cand, want = (np.ascontiguousarray(K8[f'{pre}_{k}']) for k in ('par', 'lam', 'cand', 'out'))
    lwant = K8[f'{pre}_list'] if bi else None
    if sel is not None:
        par, lam, want = np.ascontiguousarray(par[sel]), np.ascontiguousarray(lam[sel]), want[sel]
        lwant = lwant[sel] if bi else None
    (cur, r0, r1), o = me_planes(bd)
    S = cur.itemsize
    H, W = K8[f'f{bd}_cur'].shape
    got = np.full((len(par), 3), -1, dtype=np.int32)
    lgot = np.zeros((len(par), 6, 2), dtype=np.int16)
    at = lambda a: C.c_void_p(a.ctypes.data + o * S)
    rc = lib.h_me_batch(bi, bd, lanes, at(cur), at(r0), at(r1), cur.shape[1], W, H, len(par), P(par), P(lam), P(cand), P(got), P(lgot))
    assert rc == 0
    return got, want, lgot, lwant, par


def me_report(got, want, par, lam=None, lgot=None, lwant=None):
    """The first failing items with their parameters plus got / want vector and cost (None when everything matches)."""
    bad = np.flatnonzero((got != want).any(axis=1) | (False if lgot is None else (lgot != lwant).any(axis=(1, 2))))
    if not len(bad):
        return None
    rows = [f'{len(bad)} of {len(want)} items differ']
    for i in bad[:6]:
        rows.append(f'item {i}: ' + ' '.join(f'{k}={int(v)}' for k, v in zip(ME_PAR, par[i])) + f' got mv ({got[i][0]}, {got[i][1]}) cost {got[i][2]} want mv ({want[i][0]}, {want[i][1]}) cost {want[i][2]}'
                    + ('' if lgot is None or (lgot[i] == lwant[i]).all() else f' list got {lgot[i].tolist()} want {lwant[i].tolist()}'))
    return '\n'.join(rows)


def build_me_host(d, lanes64):
    so = str(d / ('kat_host_me64.so' if lanes64 else 'kat_host_me.so'))
    extra = ['-O2', '-DTHOR_HOSTSIM_LANES=64', '-pthread'] if lanes64 else ['-O1']
    subprocess.check_call(['g++', '-std=c++17', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-shared', '-fPIC'] + extra + ['-o', so,
                           os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_me.cpp')])
    return C.CDLL(so)


def me_lanes64_slice(bd):
    """The fixed slice the 64-lane host team runs (64 OS threads per team: slow): every 7th (8 bit) / 10th (10 bit) search of up to 32x32 samples at
    encoder_speed 0 - what takes the lane-per-candidate evaluators - in fixture order, at most 140 + 60 items."""
    par = K8[f'me{bd}_par']
    small = np.flatnonzero((par[:, 5] <= 32) & (par[:, 6] <= 32) & (par[:, 13] == 0))
    return small[::7][:140] if bd == 8 else small[::10][:60]


def test_motion_search_host_build_matches_reference_kat(tmp_path):
    """Every item of kat8.npz - motion_estimate (all PU shapes 4x4 .. 128x128, frame corners / edges / interior / tie bands, predictors on, near, far off and
    beyond the frame, both signs and filter sets, encoder_speed 0 / 1 / 2, three lambdas, candidate lists of 0 .. 48 entries incl. the 5-offset widesad of 16x16
    CBs, HOR / VER / QUAD sets on a staged CB window) and motion_estimate_bi (CBs 8 .. 64, 0 .. 6 list entries, the second clip, the list side effect) at
    bitdepth 8 and 10 - bit-exact in vector, cost and list against the reference's answers, with the 1-lane host build; and a fixed slice of 200 searches with a
    64-lane host team, i.e. the lane-per-candidate code of tk_me_lanes.h against the reference itself.
    (Sensitivity checked once by hand: a reversed tie-break in me_cand_fullpel's range_min fails 18 of the 194 searches of the 64-lane slice; a rate term off by one
    quarter-pel fails 79 of them when put into me_cand_fullpel and 897 of the 2496 motion_estimate items of the 1-lane build when put into rate_of.)"""
    L1 = build_me_host(tmp_path, False)
    for bd in (8, 10):
        for bi in (0, 1):
            got, want, lgot, lwant, par = me_host_batch(L1, bd, 1, bi)
            assert len(want) >= (100 if bi else 600)
            rep = me_report(got, want, par, None, lgot if bi else None, lwant)
            assert rep is None, f'1-lane host build, bitdepth {bd}, {"motion_estimate_bi" if bi else "motion_estimate"}: {rep}'
    L64 = build_me_host(tmp_path, True)
    total = 0
    for bd in (8, 10):
        sel = me_lanes64_slice(bd)
        total += len(sel)
        got, want, _, _, par = me_host_batch(L64, bd, 64, 0, sel)
        rep = me_report(got, want, par)
        assert rep is None, f'64-lane host team, bitdepth {bd}: {rep}'
    assert 150 <= total <= 200


# ---- the block syntax writer and its bit counter (thor_amd/csrc/tk_bits.h) against the reference's bit strings (tests/golden/gen_kat9.py -> kat9.npz) --------------
def build_bits_host(d, lanes):
    so = str(d / ('kat_host_bits_l.so' if lanes else 'kat_host_bits.so'))
    extra = ['-O2', '-DTHOR_HOSTSIM_LANES=64', '-pthread'] if lanes else ['-O1']
    subprocess.check_call(['g++', '-std=c++17', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-shared', '-fPIC'] + extra + ['-o', so,
                           os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_bits.cpp')])
    return C.CDLL(so)


def bits_host_coeff(lib, lanes, start=None):
    import kat_bits as B
    par2, coef = B.K9['co_par'], np.ascontiguousarray(B.K9['co_coef'])
    n = len(par2)
    par = np.zeros((n, 4), dtype=np.int32)
    par[:, :2] = par2; par[:, 2] = 0 if start is None else start; par[:, 3] = B.CO_WORDS * 32
    b1 = np.full((n, B.CO_WORDS), B.FILL, dtype=np.uint32); bt = b1.copy()
    out = np.full((n, 6), -7, dtype=np.int32)
    assert lib.h_coeff_syntax(lanes, n, P(par), P(coef), B.CO_WORDS, P(b1), P(bt), P(out)) == 0
    return out, b1, bt


def bits_host_block(lib, lanes, rows):
    import kat_bits as B
    pool = np.ascontiguousarray(B.K9['co_coef'])
    n = len(rows)
    bc = np.full((n, B.BL_WORDS), B.FILL, dtype=np.uint32); b1 = bc.copy()
    out = np.full((n, 10), -7, dtype=np.int32)
    assert lib.h_block_syntax(lanes, n, P(rows), P(pool), len(pool), B.BL_WORDS, P(bc), P(b1), P(out)) == 0
    return out, bc, b1


def test_block_syntax_host_build_matches_reference_kat(tmp_path):
    """Every item of kat9.npz against the 1-lane host build of tk_bits.h, bit-exact in length and string: put_vlc codewords (tables 0-8, 10-18 up to 31 bits),
    write_mv, write_coeff (both emitters - on the host bs_coeff_team takes the serial loop - and both counts, at start offsets 0, 1, 31, 32, 33, 63, 17 with the
    bits before the offset preserved), write_super_mode and write_block (bs_block_head_t, the counting instances without and with ybits, both emissions)."""
    import kat_bits as B
    L1 = build_bits_host(tmp_path, 0)
    want = B.strings('co')
    assert len(want) >= 2000
    start = np.array([(0, 1, 31, 32, 33, 63, 17)[i % 7] for i in range(len(want))], dtype=np.int32)
    out, b1, bt = bits_host_coeff(L1, 1, start)
    fill_bits = B.word_bits(np.full((1, B.CO_WORDS), B.FILL, dtype=np.uint32))[0]
    bad = [f'coeff_bits_team item {i}: {out[i, :2].tolist()} want {len(w)}' for i, w in enumerate(want) if not (out[i, 0] == out[i, 1] == len(w))]
    bad += B.check_emitted('bs_coeff', B.word_bits(b1), out[:, 2], out[:, 3], want, start, fill_bits)
    bad += B.check_emitted('bs_coeff_team', B.word_bits(bt), out[:, 4], out[:, 5], want, start, fill_bits)
    assert not bad, f'{len(bad)} failures:\n' + '\n'.join(bad[:8])
    rows, bwant, head = B.all_rows()
    assert len(rows) >= 6000
    out, bc, b1 = bits_host_block(L1, 1, rows)
    bad = B.check_block_out(out, rows, bwant, head)
    bad += B.check_emitted('cooperative emission', B.word_bits(bc), out[:, 5], out[:, 6], bwant)
    bad += B.check_emitted('single-lane emission', B.word_bits(b1), out[:, 7], out[:, 8], bwant)
    assert not bad, f'{len(bad)} failures:\n' + '\n'.join(bad[:8])


@pytest.mark.parametrize('lanes', [8, 16, 64])
def test_block_syntax_counts_host_lane_teams_match_reference_kat(tmp_path, lanes):
    """coeff_bits_team's ballot automaton with W = 8, 16 and 64 positions per round (teams of OS threads, the widths of test_reference_golden.py) against the
    reference's write_coeff lengths on every coefficient item of kat9.npz - levels 1..5 on either side of every round boundary, runs across them, the
    trailing symbols at N - 1 / N - 2 - and the counting instances of bs_block_t on every block item."""
    import kat_bits as B
    L = build_bits_host(tmp_path, 1)
    want = B.strings('co')
    out, _, _ = bits_host_coeff(L, lanes)
    bad = [f'coeff_bits_team W={lanes} item {i} (size {B.K9["co_par"][i][0]} type {B.K9["co_par"][i][1]}): {out[i, :2].tolist()} want {len(w)}'
           for i, w in enumerate(want) if not (out[i, 0] == out[i, 1] == len(w))]
    assert not bad, f'{len(bad)} failures:\n' + '\n'.join(bad[:8])
    sel = np.flatnonzero(B.K9['bl_par'][:, 0] == 0)
    allw = B.strings('bl')
    rows, bwant, head = np.ascontiguousarray(B.K9['bl_par'][sel]), [allw[i] for i in sel], B.K9['bl_head'][sel]
    out, _, _ = bits_host_block(L, lanes, rows)
    bad = B.check_block_out(out, rows, bwant, head)
    assert not bad, f'{len(bad)} failures:\n' + '\n'.join(bad[:8])


def test_block_syntax_engine_only_long_codewords_and_overflow_host_build(tmp_path):
    """Two properties of the engine's bit sink that have no reference answer (the reference's putbits is undefined from 32 bits; it has no capacity check):
    codewords longer than 32 bits (levels up to 32767, the len > 32 branch of bs_vlc_t) come out as len - k zeros and the k significant bits of the code, and
    the counted length agrees; with a capacity shorter than the string ovf is set, pos still advances to the full length and no word from the capacity on is
    written."""
    import kat_bits as B
    L1 = build_bits_host(tmp_path, 0)

    def run(par, coef, b1, bt):
        par, coef = np.ascontiguousarray(par, dtype=np.int32), np.ascontiguousarray(coef, dtype=np.int16)
        out = np.full((len(par), 6), -7, dtype=np.int32)
        assert L1.h_coeff_syntax(1, len(par), P(par), P(coef), B.CO_WORDS, P(b1), P(bt), P(out)) == 0
        return out, b1, bt
    B.check_long_codewords(run)
    B.check_overflow(run)


# ---- the neighbour context of a coding block and the block cost (thor_amd/csrc/tk_block_ctx.h, tk_block_rd.h) against the reference (tests/golden/gen_kat11.py) -----
def build_ctx_host(d, lanes):
    so = str(d / ('kat_host_ctx_l.so' if lanes else 'kat_host_ctx.so'))
    extra = ['-O2', '-DTHOR_HOSTSIM_LANES=64', '-pthread'] if lanes else ['-O1']
    subprocess.check_call(['g++', '-std=c++17', '-fno-strict-aliasing', '-DTHOR_HOSTSIM', '-ffp-contract=off', '-shared', '-fPIC'] + extra + ['-o', so,
                           os.path.join(ROOT, 'tests', 'hostsim', 'kat_host_ctx.cpp')])
    lib = C.CDLL(so)
    lib.h_block_ctx.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.h_block_cost.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    lib.h_intra_search.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    lib.h_build_org8.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def intra_host(lib, bd, lanes):
    from kat_block import K11, intra_report
    par, plane, org = (np.ascontiguousarray(K11[f'intra{bd}_{k}']) for k in ('par', 'plane', 'org'))
    got = np.full((len(par), 2), -77, dtype=np.int32)
    assert lib.h_intra_search(lanes, len(par), P(par), P(plane), plane.shape[1], plane.shape[0], P(org), len(org), bd, P(got)) == 0
    assert len(par) >= 300
    return intra_report(got, K11[f'intra{bd}_out'], par)


def org8_host(lib, bd, lanes):
    from kat_block import org8_items, org8_report
    par, org, pred = org8_items(bd)
    fill = 5
    og, ol = np.full(len(org), fill, org.dtype), np.full(len(org), fill, org.dtype)
    assert lib.h_build_org8(lanes, len(par), P(par), P(org), P(pred), len(org), bd, P(og), P(ol)) == 0
    return org8_report(bd, par, org, pred, og, ol, lib.h_lds_block(), fill)


def cost_host(lib, bd, lanes):
    from kat_block import K11
    par, lam = np.ascontiguousarray(K11[f'cost{bd}_par']), np.ascontiguousarray(K11[f'cost{bd}_lam'])
    org, rec = np.ascontiguousarray(K11[f'cost{bd}_org']), np.ascontiguousarray(K11[f'cost{bd}_rec'])
    got = np.zeros((len(par), 4), dtype=np.uint64)
    assert lib.h_block_cost(lanes, len(par), P(par), P(lam), P(org), P(rec), len(org), bd, P(got)) == 0
    return got, par, lam


def test_block_context_and_cost_host_build_match_reference_kat(tmp_path):
    """Every item of kat11.npz with 1-lane teams.  Context: every block position of three frames (200x136, 328x264, 264x40: blocks over the right and bottom
    edges), superblocks of 64 and 128, sizes 8..128 - get_mv_pred, the count and both candidates of get_mv_cands (= the reference's get_mv_skip and get_mv_merge),
    find_contexts with enable 0 / 1 and the two availability flags, bit-exact.  Cost: ssd_part + ssd_total against a numpy int64 sum and rd_cost against the
    reference's cost_calc at bitdepth 8 / 10 / 12 - every alignment path of the original (16 / 8 / 4 bytes, per sample), frame-edge rectangles, all-max blocks, the
    2^30 clamp."""
    from kat_block import K11, ctx_report, cost_want, cost_report
    L1 = build_ctx_host(tmp_path, 0)
    total = 0
    for fi in range(3):
        cells, par, want = np.ascontiguousarray(K11[f'ctx{fi}_cells']), np.ascontiguousarray(K11[f'ctx{fi}_par'].astype(np.int32)), K11[f'ctx{fi}_out'].astype(np.int32)
        got = np.full(want.shape, -77, dtype=np.int32)
        assert L1.h_block_ctx(P(cells), len(cells), int(par[0][3]) // 4, len(par), P(par), P(got)) == 0
        rep = ctx_report(got, want, par)
        assert rep is None, f'frame {fi}: {rep}'
        total += len(par)
    assert total >= 5000
    for bd in (8, 10, 12):
        got, par, lam = cost_host(L1, bd, 1)
        assert len(par) >= 90
        rep = cost_report(got, cost_want(bd, L1.h_lds_block()), par, lam)
        assert rep is None, f'bitdepth {bd}: {rep}'


def test_block_cost_host_8_lane_team_matches_reference_kat(tmp_path):
    """The cost family with teams of 8 OS threads: the lane-strided row loops of ssd_part and the cross-lane sums (team_sum, team_sum64) of ssd_total."""
    from kat_block import cost_want, cost_report
    L8 = build_ctx_host(tmp_path, 1)
    for bd in (8, 10, 12):
        got, par, lam = cost_host(L8, bd, 8)
        rep = cost_report(got, cost_want(bd, L8.h_lds_block()), par, lam)
        assert rep is None, f'bitdepth {bd}, 8 lanes: {rep}'


def test_intra_sad_search_and_build_org8_host_build_match_reference_kat(tmp_path):
    """intra_sad_search (tk_block_search.h) with 1-lane and 8-lane teams against the reference's search_intra_prediction_params at bitdepth 8 and 10: mode and
    SAD of every item of kat11.npz - sizes 8 / 16 / 32 at the frame corner, in the top row, the left column and inside with every up-right / down-left
    availability (superblocks 64 and 128), 4 and 10 modes, random originals, originals equal or close to one mode's prediction, flat blocks on a flat plane
    (every mode ties; the first one weighed wins).  build_org8 against clip(2 * org - pred) at bitdepth 8 / 10 / 12, aligned and skewed originals."""
    L1, L8 = build_ctx_host(tmp_path, 0), build_ctx_host(tmp_path, 1)
    for lib, lanes in ((L1, 1), (L8, 8)):
        for bd in (8, 10):
            rep = intra_host(lib, bd, lanes)
            assert rep is None, f'bitdepth {bd}, {lanes} lanes: {rep}'
        for bd in (8, 10, 12):
            rep = org8_host(lib, bd, lanes)
            assert rep is None, f'bitdepth {bd}, {lanes} lanes: {rep}'
