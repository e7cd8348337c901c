"""Shared by tests/test_kat_host.py and tests/test_gpu_kat.py: the known answers of the neighbour context of a coding block, of the block cost and of the intra
SAD search (tests/golden/gen_kat11.py -> kat11.npz), the expected output rows of thor_hip_kat_block_cost / h_block_cost, the inputs of the build_org8 check and
failure reports that name the item."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K11 = {}
for _name in ('kat11.npz', 'kat11_10.npz', 'kat11_12.npz'):   # context + 8-bit cost | 10-bit cost | 12-bit cost
    with np.load(os.path.join(ROOT, 'tests', 'golden', _name)) as _z:
        K11.update({k: _z[k] for k in _z.files})
CTX_PAR = 'ypos xpos size fw fh sb'.split()
CTX_OUT = ('mvp.x mvp.y ncand c0.mv0.x c0.mv0.y c0.mv1.x c0.mv1.y c0.ref0 c0.ref1 c0.dir c1.mv0.x c1.mv0.y c1.mv1.x c1.mv1.y c1.ref0 c1.ref1 c1.dir '
           'cbp(enable=0) index(enable=0) cbp(enable=1) index(enable=1) upright downleft').split()
COST_PAR = 'size bw bh nbits off skew stride'.split()


def ctx_report(got, want, par):
    """The first failing items of the context family with their parameters and every field that differs (None when everything matches).  The recorded candidates
    are the answer of get_mv_skip AND of get_mv_merge: gen_kat11.py asserts that the reference returns the same for both on every item."""
    bad = np.flatnonzero((got != want).any(axis=1))
    if not len(bad):
        return None
    rows = [f'{len(bad)} of {len(want)} items differ']
    for i in bad[:6]:
        rows.append(f'item {i}: ' + ' '.join(f'{k}={int(v)}' for k, v in zip(CTX_PAR, par[i])) + ' | '
                    + ', '.join(f'{CTX_OUT[k]} got {int(got[i][k])} want {int(want[i][k])}' for k in np.flatnonzero(got[i] != want[i])))
    return '\n'.join(rows)


def cost_want(bd, lds_blk):
    """(n, 4) expected output of the cost family: numpy SSD of the luma plane for both instances (all ones where the build has no LDS instance: blocks wider
    than `lds_blk`, which the build under test reports), the reference's cost_calc twice."""
    par, ssd, cost = K11[f'cost{bd}_par'], K11[f'cost{bd}_ssd'], K11[f'cost{bd}_cost'].astype(np.uint64)
    lds = np.where(par[:, 0] <= lds_blk, ssd, np.uint64(0xffffffffffffffff))
    return np.stack([ssd, lds, cost, cost], axis=1)


def cost_report(got, want, par, lam):
    bad = np.flatnonzero((got != want).any(axis=1))
    if not len(bad):
        return None
    rows = [f'{len(bad)} of {len(want)} items differ']
    for i in bad[:6]:
        rows.append(f'item {i}: ' + ' '.join(f'{k}={int(v)}' for k, v in zip(COST_PAR, par[i])) + f' lambda={lam[i]!r} got (ssd global, ssd lds, cost, cost with ssd_y) '
                    f'{[int(v) for v in got[i]]} want {[int(v) for v in want[i]]}')
    return '\n'.join(rows)


INTRA_PAR = 'ypos xpos size sb num_intra_modes off'.split()
INTRA_MODES = 'DC PLANAR HOR VER UPLEFT UPRIGHT UPUPRIGHT UPUPLEFT UPLEFTLEFT DOWNLEFTLEFT'.split()


def intra_report(got, want, par):
    """The first failing items of the intra search (mode and SAD against the reference's search_intra_prediction_params), None when everything matches."""
    bad = np.flatnonzero((got != want).any(axis=1))
    if not len(bad):
        return None
    name = lambda m: INTRA_MODES[m] if 0 <= m < 10 else str(m)
    rows = [f'{len(bad)} of {len(want)} items differ']
    for i in bad[:6]:
        rows.append(f'item {i}: ' + ' '.join(f'{k}={int(v)}' for k, v in zip(INTRA_PAR, par[i]))
                    + f' | got mode {name(int(got[i][0]))} sad {int(got[i][1])} want mode {name(int(want[i][0]))} sad {int(want[i][1])}')
    return '\n'.join(rows)


ORG8_PAR = 'size off skew stride'.split()


def org8_items(bd):
    """Inputs of the build_org8 check, the same for the host and the device test: (par (n, 4) size, off, skew, stride; org pool; pred pool).  Sizes 8..64, originals
    16-byte aligned and skewed by 2 (and, for the 8-bit type, 4 and 8) bytes, strides that keep or break the alignment of four samples; full-range random samples
    (2 * org - pred leaves the range at both ends in every block), plus blocks of extremes: org all-max / pred zero, org zero / pred all-max, and their mix."""
    rng = np.random.default_rng(80 + bd)
    T, S, peak = (np.uint8, 1, 255) if bd == 8 else (np.uint16, 2, (1 << bd) - 1)
    par, org, pred, off = [], [], [], 0
    for size in (8, 16, 32, 64):
        for skew, pad in ((0, 0), (2, 0), (0, 2), (0, 4), (4, 0), (8, 8)) if size < 64 else ((0, 0), (2, 0)):
            n = size * size
            kind = len(par) % 4
            if kind == 3:
                o = rng.choice([0, peak], n); p = rng.choice([0, peak], n)
            else:
                o = rng.integers(0, peak + 1, n); p = rng.integers(0, peak + 1, n)
            par.append((size, off, skew, size + pad)); org.append(o.astype(T)); pred.append(p.astype(T))
            off += n
    return np.array(par, dtype=np.int32), np.concatenate(org), np.concatenate(pred)


def org8_report(bd, par, org, pred, outg, outl, lds_blk, fill):
    """Both outputs against clip(2 * org - pred, 0, 2^bd - 1); outside the items' blocks, and in out_lds for blocks wider than `lds_blk`, the pools keep `fill`."""
    peak = (1 << bd) - 1
    want = np.clip(2 * org.astype(np.int64) - pred.astype(np.int64), 0, peak)
    rows, lo, hi = [], 0, 0
    for i, (size, off, skew, stride) in enumerate(par):
        n = size * size
        w = want[off:off + n]
        lo += int((w == 0).any()); hi += int((w == peak).any())
        for tag, out, run in (('global', outg, True), ('lds', outl, size <= lds_blk)):
            g = out[off:off + n].astype(np.int64)
            exp = w if run else np.full(n, fill, np.int64)
            if not np.array_equal(g, exp):
                k = int(np.flatnonzero(g != exp)[0])
                rows.append(f'item {i} ({tag} instance): ' + ' '.join(f'{a}={int(v)}' for a, v in zip(ORG8_PAR, par[i]))
                            + f' | first difference at sample {k} (row {k // size}, column {k % size}): org {int(org[off + k])} pred {int(pred[off + k])} got {int(g[k])} want {int(exp[k])}')
    assert lo >= len(par) - 2 and hi >= len(par) - 2, 'the items must saturate at both ends'
    return None if not rows else f'{len(rows)} outputs differ\n' + '\n'.join(rows[:6])
