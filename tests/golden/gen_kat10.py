#!/usr/bin/env python3
"""Known answers of the reference's CDEF at frame level: cdef_search (enc/encode_frame.c:228-489) followed by cdef_frame for planes 0, 1, 2
(common/common_frame.c:826-1003) exactly as encode_frame runs them (:768-774, cdef_damping 5), through oracle/refshim.c (ref_cdef_frame in
oracle/_ref/libthorref.so, the 16-bit build in libthorref_hbd.so; build container only, `make -C oracle reflib`).  The per-strength distortions, which
cdef_search keeps in locals, come from ref_cdef_mse: cdef_search's own loop over the reference's own functions (cdef_prepare_input, cdef_find_dir_simd,
cdef_filter_block_simd, the file-static dist_8x8).  They are VALIDATED against cdef_search before anything is written (validate): the bits, the strengths
and every filter block's preset that cdef_search returned follow from them, and where the search kept the bits it was given the preset of every live filter
block is the argmin of mse0[strength] + mse1[uv_strength] over the final presets.
Writes tests/golden/kat10.npz.  Pins the host build of tk_cdef.h (tests/hostsim/kat_host_cdef.cpp, tests/test_kat_host_cdef.py) and the device passes as the
encoder launches them (thor_hip_kat_cdef_frame, tests/test_gpu_cdef.py).

Per bitdepth bd (8, 10, 12) and size group g (k{bd}_n = number of groups):
  k{bd}_{g}_geo      width, height
  k{bd}_{g}_org      pool of original frames, packed planar 4:2:0       k{bd}_{g}_noise   deblocked frame minus original (int16), same pool
  k{bd}_{g}_mode     pool of block_mode_t maps, one byte per 4x4 cell (0 = skip), constant over 8x8
  k{bd}_{g}_case     rows: frame index, mode index, qp, speed (= -cdef minus 1), cdef_bits guess
  k{bd}_{g}_bits     what cdef_search returned          k{bd}_{g}_str / _uv   the 8 header strengths each (127 = not written)
  k{bd}_{g}_fbsel    per filter block: level and sec_strength of luma, then of chroma (encoder_info->cdef[].plane[])
  k{bd}_{g}_dir/_var per 8x8 luma block (-1 / 0 in all-skip filter blocks)
  k{bd}_{g}_mse      [2][filter block][64] (zero for cdef_bits 0, where the reference computes none)
  k{bd}_{g}_delta    pool of (filtered frame minus deblocked frame) (int16); k{bd}_{g}_deltai: the pool entry of each case
  k{bd}_{g}_name     a label per case (content / skip map)"""
import ctypes as C, os, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
L8 = C.CDLL(os.path.join(ROOT, 'oracle/_ref/libthorref.so'))
L16 = C.CDLL(os.path.join(ROOT, 'oracle/_ref/libthorref_hbd.so'))
P = lambda a: a.ctypes.data_as(C.c_void_p)
PRICONV = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [0, 1, 2, 3, 5, 7, 10, 13], [0, 1, 3, 6])   # enc/encode_frame.c:50-52, to map header values back
SIZES = ((200, 136), (208, 120), (72, 72), (128, 64))


def dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def smooth(rng, h, w, bd):
    """Low-pass random field + a vertical edge, in the style of gen_kat5.py:smooth (no noise: that is added to the deblocked frame only)."""
    sc = 1 << (bd - 8)
    base = rng.integers(20, 236, size=(h // 8 + 2, w // 8 + 2)).astype(np.float64)
    img = np.kron(base, np.ones((8, 8)))[:h, :w]
    k = np.ones(5) / 5
    img = np.apply_along_axis(lambda r: np.convolve(r, k, mode='same'), 1, img)
    img = np.apply_along_axis(lambda r: np.convolve(r, k, mode='same'), 0, img)
    img[:, w // 3] += 40
    return np.clip(np.rint(img) * sc, 0, (1 << bd) - 1)


def planes(fn, w, h):
    return np.concatenate([fn(h, w).ravel(), fn(h // 2, w // 2).ravel(), fn(h // 2, w // 2).ravel()])


def content(kind, rng, w, h, bd):
    """(deblocked, original) packed frames."""
    T, mx, sc = dt(bd), (1 << bd) - 1, 1 << (bd - 8)
    sig = (2.5 if bd < 12 else 1.5) * sc
    if w * h > 10000 and bd > 8:   # the two large sizes: noise in steps of half an 8-bit level (the fixture's size); the small frames keep every low bit busy
        step = sc // 2
        noise = lambda shape: np.rint(rng.normal(0, sig / step, size=shape)) * step
    else:
        noise = lambda shape: rng.normal(0, sig, size=shape)
    if kind == 'tex':
        org = planes(lambda hh, ww: smooth(rng, hh, ww, bd), w, h)
        rec = np.clip(np.rint(org + noise(org.shape)), 0, mx)
    elif kind == 'flat':     # every strength filters to the same frame: ties in the joint search, variance 0
        rec = planes(lambda hh, ww: np.full((hh, ww), 100.0 * sc), w, h)
        org = rec + 3 * sc
    elif kind == 'checker':  # 4x4 checkerboard of two levels + a little noise: edges in every block, both diagonals equally strong
        def cb(hh, ww):
            yy, xx = np.mgrid[0:hh, 0:ww]
            return np.where(((yy // 4) + (xx // 4)) % 2 == 0, 60.0, 190.0) * sc
        org = planes(cb, w, h)
        rec = np.clip(np.rint(org + noise(org.shape)), 0, mx)
    elif kind == 'sat':      # the largest sums the packed dot products can see
        rec = planes(lambda hh, ww: np.full((hh, ww), float(mx)), w, h)
        org = np.zeros_like(rec)
    else:
        raise ValueError(kind)
    return rec.astype(T), org.astype(T)


def skipmap(kind, rng, w, h):
    bw, bh, nfb_h, nfb_v = w // 8, h // 8, (w + 63) // 64, (h + 63) // 64
    m = rng.integers(1, 5, size=(bh, bw))
    if kind == 'rand':       # about 30 % skipped 8x8 blocks; one whole filter block skipped where the frame has eight or more
        m[rng.random(m.shape) < 0.3] = 0
        if nfb_h * nfb_v >= 8:
            m[0:8, 8:16] = 0
    elif kind == 'all':
        m[:] = 0
    elif kind == 'corner':   # exactly one live filter block: the bottom-right (partial) one
        keep = m[(nfb_v - 1) * 8:, (nfb_h - 1) * 8:].copy()
        m[:] = 0
        m[(nfb_v - 1) * 8:, (nfb_h - 1) * 8:] = keep
    elif kind == 'none':
        pass
    return np.kron(m, np.ones((2, 2))).astype(np.uint8)


GRID = [(s, b) for s in (0, 1, 2) for b in (3, 2, 1)]
# per size: (content, skip map, qp, speed, cdef_bits, bitdepths or None = all).  The full speed x bits grid runs on the two small sizes; the large ones carry a
# thinned grid.  Every edge - partial blocks, fixed strengths, skip maps, contents - appears at every bitdepth.
CASES = {
    (200, 136): [('tex', 'rand', 32, 0, 3, None), ('checker', 'rand2', 32, 0, 3, (8,)), ('tex', 'corner', 32, 2, 1, None)],
    (208, 120): [('tex', 'rand', 32, 1, 3, None), ('tex', 'rand', 32, 2, 2, None), ('tex', 'rand', 32, 0, 1, None), ('flat', 'rand', 32, 1, 2, None),
                 ('tex', 'rand', 44, 1, 0, None), ('tex', 'all', 32, 1, 3, None), ('tex', 'corner', 32, 0, 2, None)],
    (72, 72): [('tex', 'rand', 32, s, b, None) for s, b in GRID] + [('flat', 'rand', 32, 0, 3, None), ('checker', 'rand', 32, 2, 3, None), ('sat', 'none', 32, 0, 3, (8, 12)),
               ('sat', 'none', 32, 1, 3, (8, 12)), ('tex', 'all', 32, 0, 2, None), ('tex', 'corner', 32, 1, 3, None), ('tex', 'rand', 20, 0, 0, None),
               ('tex', 'rand', 30, 2, 0, None), ('tex', 'rand', 44, 0, 0, None), ('checker', 'none', 40, 0, 3, None)],
    (128, 64): [('tex', 'rand', 32, s, b, None) for s, b in GRID] + [('flat', 'rand', 32, 2, 1, None), ('tex', 'all', 44, 2, 0, None), ('tex', 'rand', 30, 0, 0, None),
                ('checker', 'corner', 26, 1, 3, None)],
}


def record(bd, rec, org, mode, w, h, qp, speed, bits):
    L = L8 if bd == 8 else L16
    sfx = '' if bd == 8 else '_hbd'
    nfb, nb = ((w + 63) // 64) * ((h + 63) // 64), (w // 8) * (h // 8)
    out = rec.copy(); o = org.copy(); m = np.ascontiguousarray(mode)
    st = np.zeros(8, np.int32); uv = np.zeros(8, np.int32); fbsel = np.zeros((nfb, 4), np.int32); d = np.zeros(nb, np.int32); v = np.zeros(nb, np.int32)
    bp = C.c_int(0)
    fn = getattr(L, 'ref_cdef_frame' + sfx); fn.restype = C.c_int
    got = fn(P(out), P(o), P(m), w, h, bd, qp, bits, speed, P(st), P(uv), P(fbsel), P(d), P(v), C.byref(bp))
    mse = np.zeros((2, nfb, 64), np.uint64)
    if bits:
        r2 = rec.copy()
        getattr(L, 'ref_cdef_mse' + sfx)(P(r2), P(o), P(m), w, h, bd, speed, P(mse))
        assert (r2 == rec).all()
        validate(mse, bits, got, st, uv, fbsel, d.reshape(h // 8, w // 8), speed, bp.value, w, h)
    return got, st, uv, fbsel, d.reshape(h // 8, w // 8).astype(np.int8), v.reshape(h // 8, w // 8), mse, (out.astype(np.int32) - rec).astype(np.int16)


def replay_search(m0, m1, speed, bits):
    """cdef_search's selection (enc/encode_frame.c:95-141, :168-192, :390-469) restated on the recorded distortions of the live filter blocks, in the order
    the reference scans: the greedy + refinement sequence of search_one_dual (first strict minimum, j major / k minor), sort + dedupe, the reduced number of
    bits and the per-block assignment - which scans only the first 1 << nb_bits of the ORIGINAL presets and clips their sorted index, so that after a reduction
    the assigned preset need not be the cheapest one.  Returns nb_bits, header strengths, header uv strengths, per live block the assigned preset."""
    total = (64, 32, 16)[speed]
    m0 = m0[:, :total].astype(np.int64); m1 = m1[:, :total].astype(np.int64)
    n = 1 << bits
    lev0, lev1 = [0] * n, [0] * n

    def search_one(nsel):
        best = np.full(len(m0), 1 << 62, np.int64)
        for g in range(nsel):
            best = np.minimum(best, m0[:, lev0[g]] + m1[:, lev1[g]])
        tot = np.minimum(m0[:, :, None] + m1[:, None, :], best[:, None, None]).sum(axis=0) if len(m0) else np.zeros((total, total), np.int64)
        lev0[nsel], lev1[nsel] = divmod(int(np.argmin(tot)), total)

    for i in range(n):
        search_one(i)
    for i in range(4 * n):
        lev0[:n - 1] = lev0[1:]; lev1[:n - 1] = lev1[1:]
        search_one(n - 1)
    st, uv = list(lev0), list(lev1)
    lst = sorted((st[i] << 16) + (uv[i] << 8) + i for i in range(n))
    trans, j = [0] * n, 0
    for i, v in enumerate(lst):
        trans[v & 255] = j
        if i == 0 or (v >> 8) != (lst[i - 1] >> 8):
            st[j] = v >> 16; uv[j] = (v >> 8) & 255; j += 1
    nb_bits = j.bit_length() - 1
    nb = 1 << nb_bits
    sel = []
    for i in range(len(m0)):
        best, best_gi = 1 << 63, 0
        for gi in range(nb):
            c = int(m0[i, st[trans[gi]]]) + int(m1[i, uv[trans[gi]]])
            if c < best:
                best, best_gi = c, min(nb - 1, trans[gi])
        sel.append(best_gi)
    hdr = lambda x: PRICONV[speed][x // 4] * 4 + x % 4
    return nb_bits, [hdr(x) for x in st[:nb]], [hdr(x) for x in uv[:nb]], sel


def validate(mse, bits, nb_bits, st, uv, fbsel, d, speed, bit_pos, w, h):
    """The recorded distortions against cdef_search's own result; raises if they disagree (then nothing is written).  Everything cdef_search returned must
    follow from them (replay_search); and where the search kept the number of bits it was given - every preset distinct, every one scanned - the preset of each
    live filter block is the argmin of mse0[strength] + mse1[uv_strength] over the final presets."""
    nfb_h, nfb_v = (w + 63) // 64, (h + 63) // 64
    live = [fb for fb in range(nfb_h * nfb_v) if not (d[fb // nfb_h * 8:fb // nfb_h * 8 + 8, fb % nfb_h * 8:fb % nfb_h * 8 + 8] < 0).all()]
    n = 1 << nb_bits
    r_bits, r_st, r_uv, r_sel = replay_search(mse[0][live], mse[1][live], speed, bits)
    assert (r_bits, r_st, r_uv) == (nb_bits, [int(x) for x in st[:n]], [int(x) for x in uv[:n]]), ('recorded mse disagrees with cdef_search', r_bits, r_st, r_uv, nb_bits, st, uv)
    pair = lambda p: (int(st[p]) >> 2, int(st[p]) & 3, int(uv[p]) >> 2, int(uv[p]) & 3)
    for fb, p in zip(live, r_sel):
        assert pair(p) == tuple(int(x) for x in fbsel[fb]), ('recorded mse disagrees with the preset cdef_search assigned', fb, p, fbsel[fb])
    if nb_bits == bits:
        inv = lambda x: PRICONV[speed].index(int(x) >> 2) * 4 + (int(x) & 3)
        for fb in live:
            cost = [int(mse[0, fb, inv(st[p])]) + int(mse[1, fb, inv(uv[p])]) for p in range(n)]
            arg = [p for p in range(n) if cost[p] == min(cost)]   # several on exact ties: the reference takes the first in ITS scan order (replayed above)
            assert tuple(int(x) for x in fbsel[fb]) in [pair(p) for p in arg], ('argmin differs from the assigned preset', fb, cost, fbsel[fb])
    assert bit_pos == len(live) * nb_bits, (bit_pos, len(live), nb_bits)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that a re-run reproduces the file byte for byte."""
    import io, zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main():
    out = {}
    for bd in (8, 10, 12):
        rng = np.random.default_rng(1000 + bd)
        for g, (w, h) in enumerate(SIZES):
            frames, modes, fkey, mkey = [], [], {}, {}
            rows, res, names = [], [], []
            for kind, skip, qp, speed, bits, bds in CASES[(w, h)]:
                if bds is not None and bd not in bds:
                    continue
                if kind not in fkey:
                    fkey[kind] = len(frames); frames.append(content(kind, rng, w, h, bd))
                if skip not in mkey:
                    mkey[skip] = len(modes); modes.append(skipmap(skip.rstrip('2'), rng, w, h))
                rec, org = frames[fkey[kind]]
                rows.append([fkey[kind], mkey[skip], qp, speed, bits])
                res.append(record(bd, rec, org, modes[mkey[skip]], w, h, qp, speed, bits))
                names.append(f'{kind}/{skip}')
            k = f'k{bd}_{g}_'
            out[k + 'geo'] = np.array([w, h], np.int32)
            out[k + 'org'] = np.array([f[1] for f in frames]); out[k + 'mode'] = np.array(modes)
            out[k + 'noise'] = np.array([f[0].astype(np.int32) - f[1] for f in frames]).astype(np.int16)
            out[k + 'case'] = np.array(rows, np.int32); out[k + 'name'] = np.array(names)
            for i, name in enumerate(('bits', 'str', 'uv', 'fbsel', 'dir', 'var', 'mse')):
                out[k + name] = np.array([r[i] for r in res])
            pool, where = [], []   # cases that filter to the same frame share one delta
            for r in res:
                hit = [q for q, dlt in enumerate(pool) if (dlt == r[7]).all()]
                where.append(hit[0] if hit else len(pool))
                if not hit:
                    pool.append(r[7])
            out[k + 'delta'] = np.array(pool); out[k + 'deltai'] = np.array(where, np.int32)
            print(bd, (w, h), len(rows), 'cases; bits', out[k + 'bits'].tolist(), 'changed samples', [int((r[7] != 0).sum()) for r in res])
        out[f'k{bd}_n'] = np.array([len(SIZES)], np.int32)
    p = os.path.join(ROOT, 'tests/golden/kat10.npz')
    save_npz(p, out)
    print('wrote kat10.npz:', len(out), 'arrays,', os.path.getsize(p), 'bytes')


if __name__ == '__main__':
    main()
