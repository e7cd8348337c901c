"""tests/golden/kat10.npz (the reference's cdef_search + cdef_frame, recorded by tests/golden/gen_kat10.py) for the two tests that use it: the host build of
the CDEF passes (test_kat_host_cdef.py) and the device passes as the encoder launches them (test_gpu_cdef.py).  `check` feeds all cases of one
(size, bitdepth) group to a runner with the arguments of thor_amd.binding.kat_cdef_frame - one call, one job per case - and compares everything bit-exactly."""
import os
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K10 = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat10.npz'))
TOTAL = (64, 32, 16)   # strengths searched at speed 0 / 1 / 2


def groups(bd):
    return range(int(K10[f'k{bd}_n'][0]))


def group(bd, g):
    """The inputs of group g, one row per case: (width, height, rec, org, mode, case rows), rec = org + noise."""
    k = f'k{bd}_{g}_'
    w, h = (int(x) for x in K10[k + 'geo'])
    case = K10[k + 'case']
    org = K10[k + 'org']
    rec = (org.astype(np.int32) + K10[k + 'noise']).astype(org.dtype)
    return w, h, rec[case[:, 0]], org[case[:, 0]], K10[k + 'mode'][case[:, 1]], case


def expected_frames(bd, g):
    k = f'k{bd}_{g}_'
    _, _, rec, _, _, _ = group(bd, g)
    return (rec.astype(np.int32) + K10[k + 'delta'][K10[k + 'deltai']]).astype(rec.dtype)


def live_blocks(bd, g, c):
    """Per filter block: does the reference treat it as live (not all-skip) in case c - it left directions there."""
    k = f'k{bd}_{g}_'
    w, h = (int(x) for x in K10[k + 'geo'])
    d = K10[k + 'dir'][c]
    nfb_h, nfb_v = (w + 63) // 64, (h + 63) // 64
    return np.array([not (d[fb // nfb_h * 8:fb // nfb_h * 8 + 8, fb % nfb_h * 8:fb % nfb_h * 8 + 8] < 0).all() for fb in range(nfb_h * nfb_v)])


def check(bd, g, runner):
    """Run group g and return the list of mismatches (empty = bit-exact): strings naming case, quantity and the first differing values."""
    k = f'k{bd}_{g}_'
    w, h, rec, org, mode, case = group(bd, g)
    got = runner(rec, org, mode, w, h, case[:, 2], case[:, 3], case[:, 4], bd)
    want_out = expected_frames(bd, g)
    nfb_h = (w + 63) // 64
    bad = []
    for c in range(len(case)):
        qp, speed, bits = (int(x) for x in case[c, 2:5])
        tag = f'bd {bd} {w}x{h} case {c} ({K10[k + "name"][c]}, qp {qp} speed {speed} bits {bits})'
        live = live_blocks(bd, g, c)
        lb = np.kron(live.reshape(-1, nfb_h), np.ones((8, 8), dtype=bool))[:h // 8, :w // 8]   # 8x8 blocks of live filter blocks
        if int(got['sb_count'][c]) != int(live.sum()) or ((got['fb_compact'][c] >= 0) != live).any():
            bad.append(f'{tag}: live filter blocks {got["fb_compact"][c].tolist()} want {live.astype(int).tolist()}')
            continue
        wd, wv = K10[k + 'dir'][c], K10[k + 'var'][c]
        if (got['dir'][c][lb] != wd[lb]).any() or (got['var'][c][lb] != wv[lb]).any():
            i = np.flatnonzero((got['dir'][c][lb] != wd[lb]) | (got['var'][c][lb] != wv[lb]))[0]
            bad.append(f'{tag}: dir / var of live block #{i}: {int(got["dir"][c][lb][i])} / {int(got["var"][c][lb][i])} want {int(wd[lb][i])} / {int(wv[lb][i])}')
        if bits:
            gm, wm = got['mse'][c][:, live, :TOTAL[speed]], K10[k + 'mse'][c][:, live, :TOTAL[speed]]
            if (gm != wm).any():
                i = tuple(int(x[0]) for x in np.nonzero(gm != wm))
                bad.append(f'{tag}: {int((gm != wm).sum())} mse entries differ, first (plane group, live block, strength) {i}: {int(gm[i])} want {int(wm[i])}')
        nb = int(K10[k + 'bits'][c])
        n = 1 << nb
        if int(got['nb_bits'][c]) != nb or got['strengths'][c][:n].tolist() != K10[k + 'str'][c][:n].tolist() or got['uv_strengths'][c][:n].tolist() != K10[k + 'uv'][c][:n].tolist():
            bad.append(f'{tag}: bits {int(got["nb_bits"][c])} strengths {got["strengths"][c][:n].tolist()} uv {got["uv_strengths"][c][:n].tolist()} want {nb} '
                       f'{K10[k + "str"][c][:n].tolist()} {K10[k + "uv"][c][:n].tolist()}')
        else:
            for fb in np.flatnonzero(live):
                p = int(got['fb_sel'][c][fb])
                s, u = (int(got['strengths'][c][p]), int(got['uv_strengths'][c][p])) if 0 <= p < n else (-1, -1)
                if [s >> 2, s & 3, u >> 2, u & 3] != K10[k + 'fbsel'][c][fb].tolist():
                    bad.append(f'{tag}: filter block {fb} preset {p} = {[s >> 2, s & 3, u >> 2, u & 3]} want {K10[k + "fbsel"][c][fb].tolist()}')
                    break
        if (got['out'][c] != want_out[c]).any():
            i = int(np.flatnonzero(got['out'][c] != want_out[c])[0])
            bad.append(f'{tag}: {int((got["out"][c] != want_out[c]).sum())} filtered samples differ, first at {i}: {int(got["out"][c][i])} want {int(want_out[c][i])}')
    return bad


def assert_fixture_not_trivial(bd):
    """Properties of the recorded answers alone: the filter changed samples, some frame uses more than one preset, some search ends with fewer bits than guessed,
    and every (speed, bits) pair, the fixed strengths, every skip map and every content are there."""
    changed, multi, fewer, pairs, names, fixed = 0, 0, 0, set(), set(), set()
    for g in groups(bd):
        k = f'k{bd}_{g}_'
        case = K10[k + 'case']
        changed += int((K10[k + 'delta'] != 0).sum())
        for c in range(len(case)):
            live = live_blocks(bd, g, c)
            multi += len({tuple(r) for r in K10[k + 'fbsel'][c][live].tolist()}) > 1
            fewer += int(case[c, 4]) > 0 and int(K10[k + 'bits'][c]) < int(case[c, 4])
            pairs.add((int(case[c, 3]), int(case[c, 4])))
            names.update(str(K10[k + 'name'][c]).split('/'))
            if int(case[c, 4]) == 0:
                fixed.add(int(K10[k + 'str'][c][0]))
    assert changed > 1000 and multi > 0 and fewer > 0, (changed, multi, fewer)
    assert {(s, b) for s in (0, 1, 2) for b in (1, 2, 3)} <= pairs
    assert {'tex', 'flat', 'checker', 'rand', 'all', 'corner'} <= names and (bd == 10 or 'sat' in names)
    assert {1, 9, 24} <= fixed   # qp 20 / 30 / 44: primary 0 / 2 / 6, secondary on / on / off
