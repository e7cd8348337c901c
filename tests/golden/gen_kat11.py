#!/usr/bin/env python3
"""Known answers of the layer between the sample kernels and the stream: the neighbour context of a coding block, the block cost and the intra SAD search.

ctx_*: the reference's public get_mv_pred_lbd, get_mv_skip_lbd, get_mv_merge_lbd (common/inter_prediction.c:413-834), find_block_contexts_lbd
(common/common_block.c:283) and get_upright_available / get_downleft_available (common/common_block.h:60-95; static inline, reached through oracle/refshim.c and cross-checked
against what get_mv_pred does with them) on random deblock_data_t grids of three frames whose dimensions are no multiples of the superblock size (200x136,
328x264, and 264x40 - lower than a superblock - for the rare availability cases of the first block row), both superblock sizes, every coding-block size that fits and EVERY position on the size grid.  The grids carry 32 more cell rows than the frame has:
what a block that hangs over the bottom edge reads (the reference indexes them unconditionally).  One grid per frame, one compact int16 row per item.

cost_*: the file-static cost_calc (enc/encode_block.c:916-926, reached through oracle/refshim.c) at bitdepth 8 / 10 / 12, with a plain int64 numpy SSD beside
it: sizes 8..128, frame-edge rectangles (24x64, 40x16, 8x56, 104x128 and small ones), original pointer skews 0 / 8 / 4 / 2 bytes and strides that keep or break
each alignment (the NW = 4 / 2 / 1 row loops and the per-sample loop of ssd_part), all-max against all-zero 128x128 blocks, identical blocks, nbits 0..2^20,
lambda = lambda_coeff * squared_lambda_QP[qp], (lambda, nbits) pairs on which a fused multiply-add truncates differently (what mul_add_nofma exists for), costs at and just below the 2^30 clamp.

intra*_*: the file-static search_intra_prediction_params (enc/encode_block.c:928-1031, through oracle/refshim.c) at bitdepth 8 and 10 on a 96x80 reconstructed plane
whose lower right part is flat: sizes 8 / 16 / 32 at the frame corner, in the top row, the left column and inside with every up-right / down-left availability
(from the position, superblocks 64 and 128), 4 and 10 modes; random originals, originals equal or close to one mode's prediction (every mode wins), flat blocks
in the flat part, where every mode ties and the first one weighed must win.  Mode and SAD are recorded.

Build container only (`make -C oracle reflib`); writes tests/golden/kat11.npz (context, 8-bit cost, intra search), kat11_10.npz and kat11_12.npz (10- / 12-bit cost).  Pins thor_amd/csrc/tk_block_ctx.h and the cost of tk_block_rd.h on the host
(tests/hostsim/kat_host_ctx.cpp, tests/test_kat_host.py) and on the device (thor_hip_kat_block_ctx / thor_hip_kat_block_cost / thor_hip_kat_intra_search, tests/test_gpu_kat.py)."""
import ctypes as C, math, os
from fractions import Fraction
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L = C.CDLL(os.path.join(ROOT, 'oracle/_ref/libthorref.so'))
LH = C.CDLL(os.path.join(ROOT, 'oracle/_ref/libthorref_hbd.so'))


class MV(C.Structure):
    _fields_ = [('x', C.c_int16), ('y', C.c_int16)]


class IP(C.Structure):    # inter_pred_t (common/types.h:138-145)
    _fields_ = [('mv0', MV), ('mv1', MV), ('ref_idx0', C.c_uint32), ('ref_idx1', C.c_uint32), ('bipred_flag', C.c_uint32)]


class DD(C.Structure):    # deblock_data_t (common/types.h:178-187)
    _fields_ = [('mode', C.c_int), ('cbp_y', C.c_int), ('cbp_u', C.c_int), ('cbp_v', C.c_int), ('size', C.c_uint8), ('tb_split', C.c_uint8), ('pb_part', C.c_int),
                ('inter_pred', IP), ('inter_pred_arr', IP * 16)]


class CTX(C.Structure):   # block_context_t (common/types.h:234-241)
    _fields_ = [('split', C.c_int8), ('cbp', C.c_int8), ('mode', C.c_int8), ('size', C.c_int8), ('index', C.c_int8)]


L.get_mv_pred_lbd.restype = MV
L.get_mv_pred_lbd.argtypes = [C.c_int] * 8 + [C.POINTER(DD)]
for f in (L.get_mv_skip_lbd, L.get_mv_merge_lbd):
    f.argtypes = [C.c_int] * 7 + [C.POINTER(DD), C.POINTER(IP)]
L.find_block_contexts_lbd.argtypes = [C.c_int] * 5 + [C.POINTER(DD), C.POINTER(CTX), C.c_int]
L.find_block_contexts_lbd.restype = None
CELL = np.dtype([('mv0x', '<i2'), ('mv0y', '<i2'), ('mv1x', '<i2'), ('mv1y', '<i2'), ('mode', 'u1'), ('size', 'u1'), ('tbpb', 'u1'), ('cbp', 'u1'), ('ref0', 'i1'), ('ref1', 'i1'),
                 ('dir', 'i1'), ('pad', 'u1')])   # thor_hip_cell (include/thor_hip.h)
MARGIN = 32   # cell rows below the frame


def make_grid(rng, fw, fh):
    """Random cells: vectors anywhere in +-2047, references 0..3, dir 0 / 2 / (uint32)-1, cbp 0..7, size 8..128, every mode; about one cell in four copies its left
    or upper neighbour's prediction exactly (the duplicate rule of get_mv_skip / get_mv_merge)."""
    cs, rows = fw // 4, fh // 4 + MARGIN
    g = np.zeros(rows * cs, dtype=CELL)
    n = len(g)
    for k in ('mv0x', 'mv0y', 'mv1x', 'mv1y'): g[k] = rng.integers(-2047, 2048, n)
    g['ref0'] = rng.integers(0, 4, n); g['ref1'] = rng.integers(0, 4, n)
    g['dir'] = rng.choice([0, 0, 2, 2, -1], n)
    g['cbp'] = rng.integers(0, 8, n) * (rng.integers(0, 3, n) > 0)
    g['size'] = rng.choice([8, 16, 32, 64, 128], n)
    g['mode'] = rng.integers(0, 5, n); g['tbpb'] = rng.integers(0, 8, n)
    copy = rng.integers(0, 8, n)
    for i in range(n):
        src = i - 1 if copy[i] == 0 else i - cs if copy[i] == 1 else -1
        if src >= 0 and i % cs:
            for k in ('mv0x', 'mv0y', 'mv1x', 'mv1y', 'ref0', 'ref1'): g[k][i] = g[k][src]
            if g['dir'][i] != -1: g['dir'][i] = g['dir'][src]      # dir -1 on the second candidate matches any first one (inter_prediction.c:825)
    # ... and patches of up to 16 x 16 cells share one prediction, as the cells of a coded block do: the two candidates are the cells left of the block's last row
    # and above / right of its last column, which are never neighbours of each other, so only areas of equal predictions make the duplicate rule fire
    g2 = g.reshape(rows, cs)
    for _ in range(rows * cs // 160):
        h, w = (int(v) for v in rng.integers(2, 17, 2))
        y, x = int(rng.integers(0, rows)), int(rng.integers(0, cs))
        for k in ('mv0x', 'mv0y', 'mv1x', 'mv1y', 'ref0', 'ref1'): g2[k][y:y + h, x:x + w] = g2[k][y, x]
        keep = g2['dir'][y:y + h, x:x + w] == -1
        g2['dir'][y:y + h, x:x + w] = np.where(keep, -1, g2['dir'][y, x] if g2['dir'][y, x] != -1 else 0)
    dd = (DD * n)()
    for i in range(n):
        c, d = g[i], dd[i]
        d.mode = int(c['mode']); d.cbp_y = int(c['cbp']) & 1; d.cbp_u = (int(c['cbp']) >> 1) & 1; d.cbp_v = (int(c['cbp']) >> 2) & 1
        d.size = int(c['size']); d.tb_split = int(c['tbpb']) & 1; d.pb_part = int(c['tbpb']) >> 1
        p = d.inter_pred
        p.mv0.x, p.mv0.y, p.mv1.x, p.mv1.y = int(c['mv0x']), int(c['mv0y']), int(c['mv1x']), int(c['mv1y'])
        p.ref_idx0, p.ref_idx1, p.bipred_flag = int(c['ref0']), int(c['ref1']), int(c['dir']) & 0xffffffff
    return g, dd


def pred_row(p):
    d = p.bipred_flag
    return [p.mv0.x, p.mv0.y, p.mv1.x, p.mv1.y, p.ref_idx0, p.ref_idx1, -1 if d == 0xffffffff else d]


def ctx_family(rng, out):
    stats = dict(items=0, cases={}, n1=0, n2=0, over=0, index=set(), skip_ne_merge=0)
    for fi, (fw, fh) in enumerate(((200, 136), (328, 264), (264, 40))):
        g, dd = make_grid(rng, fw, fh)
        par, want = [], []
        for sb in (64, 128):
            size = 8
            while size <= sb:
                for ypos in range(0, fh, size):
                    for xpos in range(0, fw, size):
                        mvp = L.get_mv_pred_lbd(ypos, xpos, fw, fh, size, size, sb, 0, dd)
                        sk, mg = (IP * 4)(), (IP * 4)()
                        ns = L.get_mv_skip_lbd(ypos, xpos, fw, fh, size, size, sb, dd, sk)
                        nm = L.get_mv_merge_lbd(ypos, xpos, fw, fh, size, size, sb, dd, mg)
                        rs = [ns] + sum((pred_row(sk[k]) if k < ns else [0] * 7 for k in range(2)), [])
                        rm = [nm] + sum((pred_row(mg[k]) if k < nm else [0] * 7 for k in range(2)), [])
                        stats['skip_ne_merge'] += rs != rm
                        cx = []
                        for enable in (0, 1):
                            c = CTX()
                            L.find_block_contexts_lbd(ypos, xpos, fh, fw, size, dd, C.byref(c), enable)
                            cx += [c.cbp, c.index]
                            stats['index'].add(c.index)
                        ur, dl = L.ref_upright_available(ypos, xpos, size, size, fw, fh, sb), L.ref_downleft_available(ypos, xpos, size, size, fw, fh, sb)
                        par.append((ypos, xpos, size, fw, fh, sb))
                        want.append([mvp.x, mvp.y] + rs + cx + [ur, dl])
                        case = (int(ypos > 0), ur, int(xpos > 0), dl)
                        stats['cases'][case] = stats['cases'].get(case, 0) + 1
                        stats['n1'] += ns == 1; stats['n2'] += ns == 2
                        stats['over'] += ypos + size > fh or xpos + size > fw
                size *= 2
        out[f'ctx{fi}_cells'] = g.view(np.uint8).reshape(-1, 16)
        out[f'ctx{fi}_par'] = np.array(par, dtype=np.int16)
        out[f'ctx{fi}_out'] = np.array(want, dtype=np.int16)
        stats['items'] += len(par)
        # the recorded availability flags against get_mv_pred itself, which picks its three neighbours by (U, UR, L, DL) - recompute it from the flags
        cs = fw // 4
        for (ypos, xpos, size, _, _, sb), w in zip(par, want):
            bs, bi = size // 4, (ypos // 4) * cs + xpos // 4
            up0, up1, up2, l0, l1, l2 = bi - cs, bi - cs + (bs - 1) // 2, bi - cs + bs - 1, bi - 1, bi + cs * ((bs - 1) // 2) - 1, bi + cs * (bs - 1) - 1
            dli, uri, uli = bi + cs * bs - 1, bi - cs + bs, bi - cs - 1
            pick = {(0, 0, 0, 0): (), (1, 0, 0, 0): (up0, up1, up2), (1, 1, 0, 0): (up0, up2, uri), (0, 0, 1, 0): (l0, l1, l2), (1, 0, 1, 0): (uli, up2, l2),
                    (1, 1, 1, 0): (up0, uri, l2), (0, 0, 1, 1): (l0, l2, dli), (1, 0, 1, 1): (up2, l0, dli), (1, 1, 1, 1): (up0, uri, l0)}[(int(ypos > 0), w[-2], int(xpos > 0), w[-1])]
            med = [sorted(int(g[k][i]) for i in pick)[1] if pick else 0 for k in ('mv0x', 'mv0y')]
            assert med == w[:2], (ypos, xpos, size, sb, med, w[:2])
    assert stats['skip_ne_merge'] == 0, 'get_mv_skip and get_mv_merge differ: the engine uses one function for both'
    assert len(stats['cases']) == 9 and min(stats['cases'].values()) >= 20, stats['cases']
    assert stats['n1'] >= 100 and stats['n2'] >= 100 and stats['over'] >= 50, stats
    assert stats['index'] == set(range(-1, 9)), stats['index']
    print('context:', stats['items'], 'items; availability cases (U, UR, L, DL):', dict(sorted(stats['cases'].items())), '; one candidate', stats['n1'], 'two', stats['n2'],
          '; over the frame edge', stats['over'], '; skip == merge on every item')


# ---- block cost ------------------------------------------------------------------------------------------------------------------------------------------------
LAMQ = (C.c_double * 52).in_dll(L, 'squared_lambda_QP')
LAMBDAS = [float(np.float32(c)) * LAMQ[qp] for c in (0.8, 1.0, 1.2) for qp in range(8, 52)]
VARIANTS = [(0, 0), (0, 16), (8, 0), (0, 8), (4, 0), (0, 4), (2, 0), (0, 2)]    # (skew in bytes, stride - size in samples)


def ssd_path(S, skew, stride, size, bw):
    """the row loop ssd_part (thor_amd/csrc/tk_block_rd.h) takes for the luma plane in global memory: the `al` expression with a 16-byte aligned reconstruction"""
    al = skew | (stride * S) | (size * S) | (bw * S)
    return 4 if not al & 15 else 2 if not al & 7 else 1 if not al & 3 else 0


def fma_pairs(want=12):
    """(lambda, nbits) for which a fused lambda * nbits + 0.5 truncates to another integer than the product rounded first (what cost_calc computes: -std=c99
    keeps the two roundings): lambda a free double next to 0.5 / nbits, where the product rounds up to 0.5 and the sum to 1 while the exact sum stays below 1 -
    the magnitude of the low-qp end of squared_lambda_QP.  Decided by exact rational arithmetic (float(Fraction) rounds once, correctly)."""
    found = []
    for nb in range(3, 400, 2):
        lam = 0.5 / nb
        for _ in range(3):
            fused = float(Fraction(lam) * nb + Fraction(1, 2))
            if int(fused) != int(lam * nb + 0.5):
                found.append((lam, nb))
                break
            lam = float(np.nextafter(lam, 0.0))
        if len(found) >= want: break
    return found


def squares(target, peak):
    """sample differences whose squares sum to `target`"""
    d = []
    while target > 0:
        v = min(peak, math.isqrt(target))
        d.append(v); target -= v * v
    return d


def cost_family(rng, out):
    fused = fma_pairs()
    assert len(fused) >= 8, len(fused)
    total = dict(items=0, clamp=0, near=0, fused=0)
    for bd in (8, 10, 12):
        T, S, peak = (np.uint8, 1, 255) if bd == 8 else (np.uint16, 2, (1 << bd) - 1)
        lib = L if bd == 8 else LH
        fn = lib.ref_cost_calc if bd == 8 else lib.ref_cost_calc_hbd
        fn.restype = C.c_uint32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
        items = []   # (size, bw, bh, nbits, lambda, skew, stride, org, rec)

        def noisy(size, amp):
            n = size * size * 3 // 2
            base = (peak // 3 + (np.arange(n) % size) * (peak // 400 + 1) + rng.integers(0, peak // 16 + 2, n)) % (peak + 1)
            rec = np.clip(base + rng.integers(-amp, amp + 1, n), 0, peak)
            return base.astype(T), rec.astype(T)

        def rnd_rate():
            return int(2 ** rng.uniform(0, 20)) - 1 if rng.integers(0, 8) else int(rng.choice([0, 1 << 20])), float(rng.choice(LAMBDAS))
        shapes = [(s, s, s, VARIANTS) for s in (8, 8, 16, 16, 32)] + [(64, 64, 64, VARIANTS[::2]), (128, 128, 128, [(0, 0), (2, 0)])]
        shapes += [(16, 8, 16, VARIANTS[::2]), (16, 16, 8, VARIANTS[1::2]), (32, 24, 32, VARIANTS[::2])]                   # frame-edge rectangles
        shapes += [(64, 24, 64, [(0, 0), (2, 0), (0, 4)]), (64, 40, 16, [(0, 0), (2, 0), (8, 0)]), (64, 8, 56, [(0, 0), (2, 0), (4, 0)]), (128, 104, 128, [(2, 0)])]
        for size, bw, bh, variants in shapes:
            for skew, padw in variants:
                if skew % S: continue
                o, r = noisy(size, int(rng.choice([1, 3, peak // 8, peak])))
                nb, lam = rnd_rate()
                items.append((size, bw, bh, nb, lam, skew, size + padw, o, r))
        n128 = 128 * 128 * 3 // 2
        hi, lo = np.full(n128, peak, T), np.zeros(n128, T)
        items.append((128, 128, 128, 0, LAMBDAS[0], 0, 128, hi, lo))          # 8 bit: 3 planes sum to 1.6e9 (32-bit headroom); 12 bit: 4e11 (64-bit reduction)
        items.append((128, 128, 128, 1 << 20, LAMBDAS[-1], 0, 128, lo, hi))
        items.append((128, 128, 128, 77, LAMBDAS[5], 2 if S == 2 else 4, 132, hi, lo))
        for size in (8, 32, 64):
            o, _ = noisy(size, 1)
            items.append((size, size, size, rnd_rate()[0], LAMBDAS[40], 0, size, o, o.copy()))     # identical blocks
        for lam, nb in fused:                                                      # lambda * nbits + 0.5 where contraction changes the integer
            o, r = noisy(8, 2)
            items.append((8, 8, 8, nb, lam, 0, 8, o, r))
        # costs at the 2^30 clamp and within 1000 below it: the luma SSD built from squares to land the sum where it is wanted
        big = [l for l in LAMBDAS if l >= 1100.0]
        assert big
        for k in range(24):
            size = (16, 32)[k % 2]
            lam = float(rng.choice(big))
            nb = int(((1 << 30) - int(lam)) / lam)
            assert 0 < nb <= (1 << 20)
            rate = int(lam * nb + 0.5)
            delta = int(rng.integers(1, 1000)) if k < 12 else -int(rng.integers(0, 3000))     # cost = 2^30 - delta
            ssd = (((1 << 30) - delta - rate) << (2 * bd - 16)) + int(rng.integers(0, 1 << (2 * bd - 16)))
            d = squares(ssd, peak)
            assert ssd >= 0 and len(d) <= size * size
            o, _ = noisy(size, 0)
            r = o.copy()
            o[:size * size] = 0; r[:size * size] = 0
            o[:len(d)] = d
            items.append((size, size, size, nb, lam, 0, size, o, r))
        org, rec, par, lams, ssd_y, cost, paths = [], [], [], [], [], [], {4: 0, 2: 0, 1: 0, 0: 0}
        off = 0
        for size, bw, bh, nb, lam, skew, stride, o, r in items:
            o = np.ascontiguousarray(o); r = np.ascontiguousarray(r)
            want = fn(o.ctypes.data, r.ctypes.data, size, bw, bh, nb, lam, bd)
            n, c, sc = size * size, size * size // 4, size // 2
            pl = lambda a: (a[:n].reshape(size, size)[:bh, :bw].astype(np.int64), a[n:n + c].reshape(sc, sc)[:bh // 2, :bw // 2].astype(np.int64),
                            a[n + c:].reshape(sc, sc)[:bh // 2, :bw // 2].astype(np.int64))
            s3 = [int(((a - b) ** 2).sum()) for a, b in zip(pl(o), pl(r))]
            mine = min((sum(s3) >> (2 * bd - 16)) + int(lam * nb + 0.5), 1 << 30)
            assert mine == want, ('cost_calc and the numpy SSD disagree', bd, size, bw, bh, nb, lam, mine, want)
            par.append((size, bw, bh, nb, off, skew, stride)); lams.append(lam); ssd_y.append(s3[0]); cost.append(want)
            org.append(o); rec.append(r)
            off += (len(o) + 15) // 16 * 16
            if len(o) % 16: org.append(np.zeros(-len(o) % 16, T)); rec.append(np.zeros(-len(o) % 16, T))
            paths[ssd_path(S, skew, stride, size, bw)] += 1
            total['clamp'] += want == 1 << 30; total['near'] += (1 << 30) - 1000 <= want < 1 << 30
        total['items'] += len(items); total['fused'] += len(fused)
        out[f'cost{bd}_org'] = np.concatenate(org); out[f'cost{bd}_rec'] = np.concatenate(rec)
        out[f'cost{bd}_par'] = np.array(par, dtype=np.int32); out[f'cost{bd}_lam'] = np.array(lams, dtype=np.float64)
        out[f'cost{bd}_ssd'] = np.array(ssd_y, dtype=np.uint64); out[f'cost{bd}_cost'] = np.array(cost, dtype=np.uint32)
        print(f'cost, bitdepth {bd}:', len(items), 'items; luma row loops NW 4 / 2 / 1 / per sample:', [paths[k] for k in (4, 2, 1, 0)])
        assert min(paths.values()) >= 10, paths        # per fixture file, so per sample type as well
    assert total['clamp'] >= 10 and total['near'] >= 10, total
    print('cost:', total['items'], 'items;', total['clamp'], 'at the 2^30 clamp,', total['near'], 'within 1000 below it,', total['fused'], 'with a contraction-sensitive rate term')


# ---- intra SAD search ------------------------------------------------------------------------------------------------------------------------------------------
IW, IH, FLATY, FLATX = 96, 80, 24, 56     # the reconstructed plane; rows from FLATY and columns from FLATX on hold one value (every prediction of a block in there is that value)
EVAL_ORDER = [0, 2, 3, 1, 4, 5, 6, 7, 8, 9]     # intra_mode_t in the order search_intra_prediction_params weighs them: DC, HOR, VER, PLANAR, then the angular ones


def intra_family(rng, out):
    total = dict(items=0, wins={m: 0 for m in range(10)}, ties=0, cats=set())
    for bd in (8, 10):
        T, peak = (np.uint8, 255) if bd == 8 else (np.uint16, 1023)
        lib = L if bd == 8 else LH
        search = lib.ref_search_intra if bd == 8 else lib.ref_search_intra_hbd
        preds = lib.ref_intra_preds if bd == 8 else lib.ref_intra_preds_hbd
        search.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_int)]
        preds.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
        preds.restype = None
        plane = rng.integers(0, peak + 1, (IH, IW)).astype(T)
        flat = int(peak * 0.6)
        plane[FLATY:, FLATX:] = flat
        plane = np.ascontiguousarray(plane)
        items = []    # (ypos, xpos, size, sb, num_modes, org)

        def all_preds(y, x, size, sb):
            p = np.zeros((10, size * size), T)
            preds(plane.ctypes.data, IW, IH, y, x, size, sb, bd, p.ctypes.data)
            return p
        for size in (8, 16, 32):
            for sb in (64, 128):
                # positions by category: frame corner, top row, left column, interior by up-right / down-left availability - two of each kind that occurs
                cats = {}
                for y in range(0, IH - size + 1, size):
                    for x in range(0, IW - size + 1, size):
                        ur, dl = L.ref_upright_available(y, x, size, size, IW, IH, sb), L.ref_downleft_available(y, x, size, size, IW, IH, sb)
                        cats.setdefault((y == 0, x == 0, ur, dl), []).append((y, x))
                for key, pos in sorted(cats.items()):
                    total['cats'].add(key)
                    for k in rng.permutation(len(pos))[:2]:
                        y, x = pos[k]
                        for nm in (4, 10):
                            items.append((y, x, size, sb, nm, rng.integers(0, peak + 1, size * size).astype(T)))                  # random original
                        p = all_preds(y, x, size, sb)
                        m = int(rng.integers(0, 10))
                        near = np.clip(p[m].astype(np.int64) + rng.integers(-2, 3, size * size), 0, peak).astype(T)                 # close to one mode's prediction
                        items.append((y, x, size, sb, 10, near))
            # originals equal to one mode's prediction, at interior positions in the random part of the plane (the predictions differ there)
            inner = [(size, size)] + ([(size, 2 * size)] if size < 32 else [])
            for y, x in inner:
                for sb in (64, 128):
                    p = all_preds(y, x, size, sb)
                    for m in range(10):
                        items.append((y, x, size, sb, 10, p[m].copy()))
                        if m < 4: items.append((y, x, size, sb, 4, p[m].copy()))
            # flat blocks inside the flat part: every mode predicts `flat`, every SAD is equal (0, or the same positive number) and the first mode weighed must win
            fpos = [(y, x) for y in range(-(-(FLATY + 1) // size) * size, IH - size + 1, size) for x in range(-(-(FLATX + 1) // size) * size, IW - size + 1, size)]
            for k, (y, x) in enumerate(fpos[:6]):
                for nm in (4, 10):
                    items.append((y, x, size, (64, 128)[k % 2], nm, np.full(size * size, flat, T)))
                items.append((y, x, size, (64, 128)[k % 2], 10, np.full(size * size, flat + 3, T)))
        par, org, want, off = [], [], [], 0
        for y, x, size, sb, nm, o in items:
            o = np.ascontiguousarray(o)
            mode = C.c_int(-1)
            sad = search(o.ctypes.data, plane.ctypes.data, IW, IH, y, x, size, sb, nm, bd, C.byref(mode))
            par.append((y, x, size, sb, nm, off)); want.append((mode.value, sad)); org.append(o)
            off += len(o)          # size * size: a multiple of 16
            total['wins'][mode.value] += 1
            if sad == 0:
                p = all_preds(y, x, size, sb)
                zero = [m for m in EVAL_ORDER[:nm] if np.array_equal(p[m], o)]
                if len(zero) >= 3:
                    assert mode.value == zero[0]
                    total['ties'] += 1
        total['items'] += len(items)
        out[f'intra{bd}_plane'] = plane; out[f'intra{bd}_org'] = np.concatenate(org)
        out[f'intra{bd}_par'] = np.array(par, dtype=np.int32); out[f'intra{bd}_out'] = np.array(want, dtype=np.int32)
        print(f'intra search, bitdepth {bd}:', len(items), 'items')
    assert min(total['wins'].values()) >= 3, total['wins']
    assert total['ties'] >= 12, total['ties']
    assert (True, True, 0, 0) in total['cats'] and any(k[0] and not k[1] for k in total['cats']) and {(False, True, 0, 0), (False, True, 1, 0)} <= total['cats'], total['cats']
    assert {(0, 0), (0, 1), (1, 0), (1, 1)} <= {k[2:] for k in total['cats'] if not k[0] and not k[1]}, total['cats']
    print('intra search:', total['items'], 'items; wins per mode', total['wins'], '; items with three or more modes tied at SAD 0:', total['ties'],
          '; position kinds (top row, left column, up-right, down-left):', sorted(total['cats']))


def main():
    rng = np.random.default_rng(111111)
    out = {}
    ctx_family(rng, out)
    cost_family(rng, out)
    intra_family(np.random.default_rng(111113), out)      # a generator of its own: the two families above stay what they were
    # no committed file above 1 MiB: the 10- and 12-bit sample pools go to files of their own (as kat4.npz / kat4_12.npz do)
    for name, keep in (('kat11.npz', lambda k: not k.startswith(('cost10', 'cost12'))), ('kat11_10.npz', lambda k: k.startswith('cost10')),
                       ('kat11_12.npz', lambda k: k.startswith('cost12'))):
        path = os.path.join(ROOT, 'tests', 'golden', name)
        np.savez_compressed(path, **{k: v for k, v in out.items() if keep(k)})
        print(name + ':', os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
