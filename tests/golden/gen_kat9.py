#!/usr/bin/env python3
"""Known answers of the reference's block syntax as bit STRINGS: put_vlc (enc/putvlc.c:73-160), write_mv (enc/write_bits.c:123-143), write_coeff (:145-241),
write_super_mode (:257-358) and write_block (:360-600), reached through oracle/refshim.c (ref_put_vlc, ref_write_mv, ref_write_coeff, ref_write_super_mode,
ref_write_block in oracle/_ref/libthorref.so; every wrapper writes into a fresh stream_t).  Pins the host build of thor_amd/csrc/tk_bits.h
(tests/hostsim/kat_host_bits.cpp, tests/test_kat_host.py) and the device build (thor_hip_kat_coeff_syntax / thor_hip_kat_block_syntax, tests/test_gpu_kat.py).

Regenerate (needs the reference tree that oracle/Makefile builds from; seeded, byte for byte reproducible):
  make -C oracle reflib && python tests/golden/gen_kat9.py   -> tests/golden/kat9.npz

Strings: X_len[i] bits; X_str holds ceil(X_len[i] / 8) bytes per item back to back, first bit in the MSB, bits beyond the length zero.
  vlc_par (n, 2): table, symbol.            mv_par (n, 4): mv.x, mv.y, mvp.x, mvp.y.
  co_par (n, 2): size, type (bit 0 chroma, bit 1 intra block); co_coef (n, 256): the qs x qs block row-major in the first qs^2 entries (qs = min(size, 16)),
    built in scan order through the reference's own zigzag tables (ref_zigzag).  Every item has a non-zero coefficient, as write_block calls write_coeff.
  bl_par (n, 57): the rows of thor_amd/csrc/tk_kat_bits.h (kind 0 write_block, 1 write_super_mode; SynCtx and BlkParam flat; [45..56] index into co_coef of
    luma TU 0..3, U 0..3, V 0..3 or -1 - laid out for the reference as block_param_t holds them, TU t at t * MAX_QUANT_SIZE^2).  bl_head: for kind 0 the length
    of the part before the cbp code.  It is read off the reference's strings alone: the item is written eight more times with the eight cbp triples of an
    unsplit block (which all start after the same head, and whose first residual bit takes both values); the shortest common prefix with the item's own
    string is the head.
The super-mode, head and block items are seeded draws from the cross product (frame type, num_ref, enable_bipred, interp_ref, size, context index,
encode_this_size, split_flag, mode, ref_idx0, num_intra_modes, max_pb_part x pb_part, num_skip / num_merge), restricted to combinations the syntax allows; that
every named value and combination is present, and that the cbp remaps actually fire in every mode x tb_split cell, is asserted from the inputs (gen_blocks).
Every codeword is at most 31 bits long (the reference's putbits shifts by n through mask(n), undefined from 32): asserted with the oracle's VLC-length
function, hence |coefficient| <= 4000 (the run-mode level code reaches 32 bits at level 4098).
The chroma two-bit shortcut has 20 distinct inputs only (5 sizes x intra x sign); each is recorded twice to reach the 30 items asked of every class."""
import ctypes as C, os, sys, itertools, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from util import build_oracle_c
R = C.CDLL(os.path.join(ROOT, 'oracle', '_ref', 'libthorref.so'))
O = build_oracle_c()
O.orc_vlc_len.argtypes = [C.c_int, C.c_uint]
P = lambda a: a.ctypes.data_as(C.c_void_p)
OUTB = 1 << 16
_out = np.zeros(OUTB, dtype=np.uint8)
NP = 57
SKIP, INTRA, INTER, BIPRED, MERGE = range(5)
MAXLEN = 31


class Strings:
    def __init__(self): self.len, self.str = [], []
    def add(self, n):
        assert 0 <= n <= 8 * OUTB
        self.len.append(n); self.str.append(_out[:(n + 7) // 8].copy())
        return self.str[-1]
    def arrays(self): return np.array(self.len, dtype=np.int32), (np.concatenate(self.str) if self.str else np.zeros(0, np.uint8))


def zigzag(qs):
    z = np.zeros(qs * qs, dtype=np.int32)
    R.ref_zigzag(qs, P(z))
    return z


ZZ = {q: zigzag(q) for q in (4, 8, 16)}


# ---- (a) VLC ----------------------------------------------------------------------------------------------------------------------------------------------
def gen_vlc():
    par = []
    for n in list(range(8)) + [10]:
        cns = set(range(301))
        for k in range(1, 32):
            for d in (-1, 0, 1):
                cns.add((1 << k) + d)
        par += [(n, cn) for cn in sorted(cns) if cn < (1 << 31) and O.orc_vlc_len(n, cn) <= MAXLEN]
    par += [(8, cn) for cn in range(10)]
    for n in range(11, 19):
        par += [(n, cn) for cn in range(n - 10 + 1)]
    S = Strings()
    for n, cn in par:
        ln = R.ref_put_vlc(n, C.c_uint(cn), P(_out), OUTB)
        assert ln == O.orc_vlc_len(n, cn) <= MAXLEN, (n, cn, ln)
        S.add(ln)
    return np.array(par, dtype=np.int32), S


# ---- (b) motion vector differences ----------------------------------------------------------------------------------------------------------------------
def gen_mv(rng):
    par = []
    for dx, dy in itertools.product(range(-5, 6), repeat=2):
        px, py = (int(v) for v in rng.integers(-300, 300, 2))
        par.append((px + dx, py + dy, px, py))
    for _ in range(200):
        px, py = (int(v) for v in rng.integers(-2000, 2000, 2))
        dx, dy = (int(v) for v in rng.integers(-2000, 2001, 2))
        par.append((px + dx, py + dy, px, py))
    par += [(30000, -5, -30000, 7), (-30000, 11, 30000, -3)]   # mv - mvp wraps as int16, one case each way
    S = Strings()
    for q in par:
        for a, b in ((q[0], q[2]), (q[1], q[3])):
            d = ((a - b + 32768) & 0xffff) - 32768
            assert abs(d) < 32768 and O.orc_vlc_len(7, abs(d)) <= MAXLEN
        S.add(R.ref_write_mv(*q, P(_out), OUTB))
    return np.array(par, dtype=np.int32), S


# ---- (c) coefficient blocks -----------------------------------------------------------------------------------------------------------------------------
def walk(s, N, chroma):
    """Plain walk of write_coeff's scan: (classes of the item, as a set of names)."""
    last = max(i for i in range(N) if s[i])
    if chroma and last == 0 and abs(s[0]) == 1:
        return {'shortcut'}
    pos, level_mode, level, mode, runs = 0, 1, 1, {}, []
    while pos <= last:
        if level_mode:
            while pos <= last and level > 0:
                mode[pos] = 'L'; level = abs(s[pos]); pos += 1
        c, start = 0, pos
        while c == 0 and pos <= last:
            c = s[pos]; mode[pos] = 'R'; pos += 1
            if c:
                level = abs(c); level_mode = level > 1
                if pos - 1 > start: runs.append((start, pos - 1))   # zeros [start, pos - 1), coefficient at pos - 1
    cl = set()
    for p in range(64, N, 64):
        if mode.get(p) == 'L' and mode.get(p - 1) == 'L':
            cl.add('lvl64_prev_gt3' if abs(s[p - 1]) > 3 else 'lvl64_prev_le3')
        if any(a < p <= b for a, b in runs): cl.add('run_cross64')
    if last == N - 1: cl.add('last_N1_level' if mode[last] == 'L' else 'last_N1_run')
    if last == N - 2 and mode[last] == 'L': cl.add('last_N2_level')
    return cl


CLASSES = ['lvl64_prev_gt3', 'lvl64_prev_le3', 'run_cross64', 'last_N1_level', 'last_N1_run', 'last_N2_level', 'shortcut', 'runtab10', 'runtab6_chroma']


def gen_coeff(rng):
    items = []   # (size, type, scan-order array)
    for size, chroma, intra in itertools.product((4, 8, 16, 32, 64), (0, 1), (0, 1)):
        qs = min(size, 16); N = qs * qs; ty = chroma | (intra << 1)
        def put(s): items.append((size, ty, np.array(s, dtype=np.int64)))
        def z(): return [0] * N
        for v in (1, -1, 2, -2):
            s = z(); s[0] = v; put(s)
            if chroma and abs(v) == 1: put(s)
        for p, vals in ((N - 1, (1, -3)), (N - 2, (1, 2, -5))):
            for v in vals:
                s = z(); s[p] = v; put(s)
        for k in range(3):   # dense
            mag = rng.geometric(0.35, N) * (rng.random(N) < 0.75) + (rng.random(N) < 0.03) * rng.integers(0, 200, N)
            s = (mag * rng.choice((-1, 1), N)).tolist()
            if k == 0: s[N - 1] = 3
            if k == 1: s[N - 1] = 0; s[N - 2] = -2; s[N - 3] = 6
            if not any(s): s[0] = 2
            put(s)
        for k in range(3):   # sparse, long runs
            s = z()
            for p in rng.choice(N, size=max(2, N // 40), replace=False): s[p] = int(rng.choice((-1, 1))) * int(rng.choice((1, 1, 1, 2, 3, 7)))
            put(s)
        for fill in (2, 5):  # level mode up to the end / up to N - 2
            s = [fill * (-1) ** i for i in range(N)]; put(s)
            s = [fill * (-1) ** i for i in range(N)]; s[N - 1] = 0; put(s)
        for b in (8, 16, 64, 128, 192):
            if b >= N: continue
            for lvl, p, fill in itertools.product((1, 2, 3, 4, 5), (b - 1, b), (2, 5)):
                s = z()
                for i in range(b + 1): s[i] = fill if (i * 7 + lvl) % 3 else -fill
                s[p] = lvl if (p + lvl) % 2 else -lvl
                put(s)
            for k, j in itertools.product((1, 2, 5), (0, 1, 3)):   # zeros [b - k, b + j), coefficient at b + j
                if b + j >= N or b - k - 1 < 0: continue
                s = z(); s[0] = 3; s[b - k - 1] = -1 if k == 2 else 2; s[b + j] = (1, -2, 6)[j % 3]
                put(s)
        s = z(); s[0] = 4000; put(s)
        s = z(); s[0] = -4000; s[1] = 4000; put(s)
        s = z(); s[min(5, N - 1)] = -4000; s[min(9, N - 1)] = 4000 if N > 9 else -4000; put(s)
    par, coef, S, count = [], [], Strings(), dict.fromkeys(CLASSES, 0)
    for size, ty, s in items:
        qs = min(size, 16); N = qs * qs
        assert np.any(s) and np.abs(s).max() <= 4000
        c = np.zeros(256, dtype=np.int16)
        c[:N] = s[ZZ[qs]]            # scoeff[zigzag[i]] = coeff[i]
        cl = walk(s.tolist(), N, ty & 1)
        if ty & 1: cl.add('runtab10' if size <= 8 else 'runtab6_chroma')
        for k in cl: count[k] += 1
        ln = R.ref_write_coeff(P(c), size, ty, P(_out), OUTB)
        assert ln == R.ref_coeff_bits(P(c), size, ty)
        S.add(ln); par.append((size, ty)); coef.append(c)
    for k in CLASSES: assert count[k] >= 30, (k, count)
    print('coefficient classes:', count)
    # the 31-bit cap, from the inputs: every symbol write_coeff can form from these levels and runs
    amax = max(int(np.abs(c).max()) for c in coef)
    assert max(O.orc_vlc_len(t, amax) for t in (0, 1)) <= MAXLEN and O.orc_vlc_len(0, (amax - 2) * 2 + 1) <= MAXLEN
    assert max(O.orc_vlc_len(t, 255 * 5 + 5) for t in (6, 10)) <= MAXLEN
    return np.array(par, dtype=np.int32), np.array(coef), S


# ---- (d) + (e) super-mode, heads, whole blocks --------------------------------------------------------------------------------------------------------------
def sample_head(rng, mode=None, frame_type=None):
    """One consistent (frame, block context, block parameter) row without residual fields, drawn from the cross product the issue lists."""
    q = [0] * NP
    for k in range(45, 57): q[k] = -1
    ft = int(rng.integers(0, 3)) if frame_type is None else frame_type
    q[2] = ft
    q[3] = int(rng.integers(1, 5)); q[4] = int(rng.integers(0, 2)); q[5] = int(rng.integers(0, 4))
    q[6] = int(rng.choice((1, 4))); q[7] = int(rng.choice((1, 2))); q[8] = int(rng.choice((4, 8, 10)))
    q[9] = int(rng.choice((8, 16, 32, 64, 128))); q[10] = int(rng.random() < 0.85); q[11] = int(rng.integers(0, 6)); q[12] = int(rng.integers(0, 2))
    q[13] = int(rng.integers(1, 5)); q[14] = int(rng.integers(1, 5))
    q[15], q[16] = (int(v) for v in rng.integers(-400, 400, 2))
    if mode == BIPRED and ft != 0: q[3] = int(rng.integers(2, 5)); q[4] = 1      # a bi-predicted block needs two references and the tool switched on
    bip = q[3] > 1 and q[4]
    if ft == 0: m = INTRA
    else:
        ok = [SKIP, MERGE, INTER, INTRA] + ([BIPRED] if bip else [])
        m = mode if mode in ok else int(rng.choice(ok))
    q[17] = m
    q[18] = int(rng.integers(0, 4 if q[8] <= 4 else 10))
    q[19] = int(rng.integers(0, q[13] if m == SKIP else q[14]))
    q[20] = int(rng.integers(0, 4)) if (q[6] > 1 or m == BIPRED) and m in (INTER, BIPRED) else 0
    lo = 1 if (m == INTER and q[5] > 2) else 0     # interp_ref > 2: ref_idx 0 is not allowed for a uni-predicted block
    if m == INTER and lo >= q[3]: q[3] = 2
    q[21] = int(rng.integers(lo, q[3])) if m in (INTER, BIPRED) else 0
    q[22] = int(rng.integers(0, q[3])) if m == BIPRED else 0
    if m == BIPRED: q[21] = int(rng.integers(0, q[3]))
    for k in range(29, 45):
        q[k] = int(q[15 + (k - 29) % 2] + rng.choice((0, 0, 1, -1, 2, -3, 17, -40, 300)))
    return q


def call_block(q, pool):
    cy, cu, cv = (np.zeros(1024, dtype=np.int16) for _ in range(3))
    for pl, a in enumerate((cy, cu, cv)):
        for t in range(4):
            if q[45 + 4 * pl + t] >= 0: a[256 * t:256 * t + 256] = pool[q[45 + 4 * pl + t]]
    qa = np.array(q, dtype=np.int32)
    ln = R.ref_write_block(P(qa), P(cy), P(cu), P(cv), P(_out), OUTB)
    assert ln >= 0
    return ln


def bits(n): return np.unpackbits(_out[:(n + 7) // 8])[:n].copy()


def head_len(q, pool, dc2):
    """Length of the part of write_block before the cbp code, from the reference's strings alone (see the module docstring)."""
    if q[17] == SKIP: return call_block(q, pool)
    own = bits(call_block(q, pool))
    best = len(own)
    for y, u, v in itertools.product((0, 1), repeat=3):
        v_ = list(q); v_[25] = 0; v_[26:29] = [y, u, v]
        for k in range(45, 57): v_[k] = -1
        sz = q[9]
        if y: v_[45] = dc2[(sz, 0)]
        if u: v_[49] = dc2[(sz // 2, 1)]
        if v: v_[53] = dc2[(sz // 2, 1)]
        o = bits(call_block(v_, pool))
        n = min(len(o), len(own)); d = np.flatnonzero(o[:n] != own[:n])
        best = min(best, int(d[0]) if len(d) else n)
    return best


def gen_blocks(rng, co_par, co_coef, co_len):
    by = {}
    for i, (size, ty) in enumerate(co_par):
        if co_len[i] <= 1400: by.setdefault((int(size), int(ty) & 1), []).append(i)
    by[(128, 0)] = by[(64, 0)]       # a 128x128 luma unit codes 16x16 coefficients like a 64x64 one (size only enters through min(size, 16) for luma)
    dc2 = {}
    for (size, ch), lst in by.items():
        dc2[(size, ch)] = next(i for i in lst if co_coef[i][0] == 2 and np.count_nonzero(co_coef[i]) == 1)
    rows = []
    # (d) super-mode alone: split_flag 0 / 1, encode_this_size 0 / 1
    for _ in range(1500):
        q = sample_head(rng); q[0] = 1; q[1] = int(rng.integers(0, 2))
        if q[1] and q[9] == 8: q[1] = 0 if q[2] else q[1]     # an 8x8 block of an inter frame cannot split
        rows.append(q)
    # (d) heads: whole blocks without residual (cbp = 0, unsplit)
    for mode in (SKIP, INTRA, INTER, BIPRED, MERGE):
        for _ in range(160):
            q = sample_head(rng, mode, frame_type=int(rng.integers(1, 3))); q[0] = 0
            rows.append(q)
    for _ in range(60):
        q = sample_head(rng, frame_type=0); q[0] = 0; rows.append(q)
    # (e) whole blocks
    cells = {}
    nblk = 0
    while nblk < 600:
        mode = (INTRA, INTER, BIPRED, MERGE)[nblk % 4]
        q = sample_head(rng, mode, frame_type=None if mode == INTRA else int(rng.integers(1, 3))); q[0] = 0
        if q[17] != mode: continue
        size = q[9]
        q[7] = int(rng.choice((1, 2))); tb = int(q[7] == 2 and rng.random() < 0.6)
        if nblk % 10 == 9: size = q[9] = int(rng.choice((64, 128))); q[7] = 2; tb = 1      # chroma buffers in global memory
        q[25] = tb; q[24] = tb
        suv = size // 2
        if not tb:
            y, u, v = ((nblk // 4) >> 0) & 1, ((nblk // 4) >> 1) & 1, ((nblk // 4) >> 2) & 1
            q[26:29] = [y, u, v]
            if y: q[45] = int(rng.choice(by[(size, 0)]))
            if u: q[49] = int(rng.choice(by[(suv, 1)]))
            if v: q[53] = int(rng.choice(by[(suv, 1)]))
        else:
            masks = [int(rng.choice((0, 1, 2, 4, 8, 15, int(rng.integers(0, 16))))) for _ in range(3)]
            if suv == 4: masks[1] &= 1; masks[2] &= 1
            q[26:29] = masks
            for t in range(4):
                if (masks[0] >> (3 - t)) & 1: q[45 + t] = int(rng.choice(by[(size // 2, 0)]))
            if suv > 4:
                for pl in (1, 2):
                    for t in range(4):
                        if (masks[pl] >> (3 - t)) & 1: q[45 + 4 * pl + t] = int(rng.choice(by[(suv // 2, 1)]))
            else:
                for pl in (1, 2):
                    if masks[pl]: q[45 + 4 * pl] = int(rng.choice(by[(suv, 1)]))
        remap = (mode == MERGE and not tb and q[26:29] == [0, 0, 0])
        cells[(mode, tb, 'ctx_cbp%d' % q[12])] = cells.get((mode, tb, 'ctx_cbp%d' % q[12]), 0) + 1
        if mode == MERGE and not tb: cells[(mode, tb, 'remap%d' % remap)] = cells.get((mode, tb, 'remap%d' % remap), 0) + 1
        rows.append(q); nblk += 1
    # (d): the combinations the issue names, counted from the inputs (super-mode items and heads, i.e. everything before the whole blocks)
    dn = len(rows) - nblk
    D = np.array(rows[:dn])
    sm, hd, inter_f = D[:, 0] == 1, D[:, 0] == 0, D[:, 2] > 0
    cov = {}
    for ft in (0, 1, 2): cov['frame_type%d' % ft] = int((D[:, 2] == ft).sum())
    for v in (1, 2, 3, 4): cov['num_ref%d' % v] = int((inter_f & (D[:, 3] == v)).sum())
    for v in (0, 1, 2, 3): cov['interp_ref%d' % v] = int((inter_f & sm & (D[:, 5] == v) & (D[:, 10] == 1)).sum())
    for v in (8, 16, 32, 64, 128): cov['size%d' % v] = int((sm & (D[:, 9] == v)).sum())
    for v in range(6): cov['ctx_index%d' % v] = int((sm & inter_f & (D[:, 10] == 1) & (D[:, 11] == v)).sum())
    for v in (0, 1):
        cov['encode_this_size%d' % v] = int((sm & (D[:, 10] == v)).sum()); cov['split_flag%d' % v] = int((sm & (D[:, 1] == v)).sum())
        cov['enable_bipred%d' % v] = int((sm & inter_f & (D[:, 3] > 1) & (D[:, 4] == v)).sum())
        cov['split_moved%d' % v] = int((sm & inter_f & (D[:, 10] == 1) & (D[:, 1] == 1) & (np.isin(D[:, 11], (2, 4, 5)) == bool(v))).sum())
    for m in (SKIP, INTRA, INTER, BIPRED, MERGE):
        cov['sm_mode%d' % m] = int((sm & inter_f & (D[:, 1] == 0) & (D[:, 10] == 1) & (D[:, 17] == m)).sum()); cov['head_mode%d' % m] = int((hd & (D[:, 17] == m)).sum())
    cov['inter_ref0_0'] = int((inter_f & (D[:, 17] == INTER) & (D[:, 21] == 0)).sum()); cov['inter_ref0_gt0'] = int((inter_f & (D[:, 17] == INTER) & (D[:, 21] > 0)).sum())
    cov['inter_ref0_gt0_interp_gt2'] = int((sm & (D[:, 17] == INTER) & (D[:, 21] > 0) & (D[:, 5] > 2)).sum())
    cov['intra_modes_le4'] = int((hd & (D[:, 17] == INTRA) & (D[:, 8] <= 4)).sum()); cov['intra_modes_gt4'] = int((hd & (D[:, 17] == INTRA) & (D[:, 8] > 4)).sum())
    for pb in range(4):
        cov['inter_pb4_part%d' % pb] = int((hd & (D[:, 17] == INTER) & (D[:, 6] == 4) & (D[:, 20] == pb)).sum())
        cov['bipred_part%d' % pb] = int((hd & (D[:, 17] == BIPRED) & (D[:, 20] == pb)).sum())
    cov['inter_pb1'] = int((hd & (D[:, 17] == INTER) & (D[:, 6] == 1)).sum())
    cov['bipred_P_numref2'] = int((hd & (D[:, 17] == BIPRED) & (D[:, 2] == 1) & (D[:, 3] == 2)).sum()); cov['bipred_P_numref_gt2'] = int((hd & (D[:, 17] == BIPRED) & (D[:, 2] == 1) & (D[:, 3] > 2)).sum())
    cov['bipred_B'] = int((hd & (D[:, 17] == BIPRED) & (D[:, 2] == 2)).sum())
    for m, col in ((SKIP, 13), (MERGE, 14)):
        for v in (1, 2, 3, 4): cov['nvec_mode%d_%d' % (m, v)] = int((hd & (D[:, 17] == m) & (D[:, col] == v)).sum())
    print('(d) coverage:', cov)
    for k, v in cov.items(): assert v >= 8, (k, v)
    # (e): the cbp remaps as they actually fire, from the inputs: the ctx_cbp flip needs a code below 2 (cbp of the block, or of a TU, 0 or 1 = luma only)
    E = np.array(rows[dn:])
    for mode, tb in itertools.product((INTRA, INTER, BIPRED), (0, 1)):
        for c in (0, 1):
            if tb: hit = [q for q in E if q[17] == mode and q[25] == 1 and q[9] > 8 and q[12] == c and any((((q[27] | q[28]) >> (3 - t)) & 1) == 0 for t in range(4))]
            else: hit = [q for q in E if q[17] == mode and q[25] == 0 and q[12] == c and q[27] == 0 and q[28] == 0]
            assert len(hit) >= 5, ('cbp code < 2 with ctx_cbp', mode, tb, c, len(hit))
    assert sum(1 for q in E if q[17] == MERGE and q[25] == 1 and q[9] > 8 and q[12] == 0 and any((((q[27] | q[28]) >> (3 - t)) & 1) == 0 for t in range(4))) >= 5
    assert sum(1 for q in E if q[25] == 1 and q[9] == 8) >= 5 and sum(1 for q in E if q[25] == 0 and q[7] == 2) >= 20 and sum(1 for q in E if q[7] == 1) >= 20
    for mode, tb, c in itertools.product((INTRA, INTER, BIPRED, MERGE), (0, 1), (0, 1)):
        assert cells.get((mode, tb, 'ctx_cbp%d' % c), 0) >= 5, (mode, tb, c, cells)
    assert cells.get((MERGE, 0, 'remap1'), 0) >= 5 and cells.get((MERGE, 0, 'remap0'), 0) >= 5, cells
    S, head = Strings(), []
    for q in rows:
        if q[0] == 1:
            qa = np.array(q, dtype=np.int32)
            S.add(R.ref_write_super_mode(P(qa), P(_out), OUTB)); head.append(-1)
        else:
            h = head_len(q, co_coef, dc2)
            ln = call_block(q, co_coef)
            assert h <= ln <= 20000
            S.add(ln); head.append(h)
    return np.array(rows, dtype=np.int32), S, np.array(head, dtype=np.int32)


def main():
    rng = np.random.default_rng(9009)
    R.ref_init(1)
    vlc_par, vs = gen_vlc()
    mv_par, ms = gen_mv(rng)
    co_par, co_coef, cs = gen_coeff(rng)
    co_len, co_str = cs.arrays()
    bl_par, bs, bl_head = gen_blocks(rng, co_par, co_coef, co_len)
    d = dict(vlc_par=vlc_par, mv_par=mv_par, co_par=co_par, co_coef=co_coef, co_len=co_len, co_str=co_str, bl_par=bl_par, bl_head=bl_head)
    d['vlc_len'], d['vlc_str'] = vs.arrays(); d['mv_len'], d['mv_str'] = ms.arrays(); d['bl_len'], d['bl_str'] = bs.arrays()
    out = os.path.join(ROOT, 'tests', 'golden', 'kat9.npz')
    np.savez_compressed(out, **d)
    print({k: v.shape for k, v in d.items()}, os.path.getsize(out), 'bytes')
    assert os.path.getsize(out) <= 332 * 1024


if __name__ == '__main__':
    main()
