"""The temporally interpolated reference (thor_amd/csrc/tk_interp_dev.h) stage by stage: cases, fixture and comparison shared by the generator
(tests/golden/gen_kat12.py, which records the reference's common/temporal_interp.c through oracle/interp_shim.c), the host build
(test_kat_host_interp.py) and the device (test_gpu_interp.py).

The inputs are not stored: `make_pair` builds them from integer arithmetic alone (a hash of the sample coordinates, no floating point, no library random
generator), and the fixture keeps a CRC of every input frame next to the recorded answers - kat12.npz (8 bit), kat12_10.npz, kat12_12.npz.  Nor are the
pyramid planes: `pyramid` restates scale_frame_down2x2 + pad_yuv_frame in numpy, and the generator asserts it equal to the reference's planes on every case.

ratio = 2, pos = 1 throughout (the engine's only operating point): the vectors of the two pictures are v and -v, the motion-compensation margin is 4."""
import math
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
PAD_Y = 160        # kPadY: padding of reference pictures and of the interpolated picture
PAD_PYR = 32       # padding of the pyramid planes
# id -> (width, height, levels, bit depths, pairs)
CASES = {
    'A': (200, 136, 3, (8, 10, 12), ('scene',)),       # both dimensions 16 n + 8: the last unit column / row lies outside the picture
    'B': (264, 256, 4, (8, 12), ('pan',)),             # top level 33x32; displacement +-(20, 12): edge blocks more than the margin outside
    'C': (512, 64, 2, (8, 10), ('shear',)),            # 32 block columns x 4 rows: long rows for the row pipeline, vectors that change along them
    'D': (64, 64, 2, (8, 12), ('same', 'flat', 'noise')),   # smallest legal size: every block skips / SAD ties everywhere / full search budget
    # the only content here on which mv_absdist_filter's last-minimum rule decides anything.  With two neighbours (first and last block
    # column below row 0) both cost the same, and the choice shows only where the skip test then passes with either vector: a flat area below a band of
    # 16 rows whose 16-column strips move by +8 / -8 horizontally.  (On flat frames, D, every vector is zero and the rule has nothing to choose from.)
    'E': (128, 64, 2, (8,), ('band',)),
}
_FILES = {8: 'kat12.npz', 10: 'kat12_10.npz', 12: 'kat12_12.npz'}
_K = {}


def pix(bd):
    return np.uint8 if bd == 8 else np.uint16


def levels_of(w, h):
    """temporal_interp.c:914, in double as written."""
    return min(4, int(math.log10(min(w, h)) / math.log10(2.0) - 4.0))


def grid(w, h, l):
    """(bw, bh) of level l: 8x8 units, two per 16x16 block and dimension."""
    return 2 * (((w >> l) + 15) // 16), 2 * (((h >> l) + 15) // 16)


# ---- inputs: integer arithmetic only -------------------------------------------------------------------------------------------------------------
def _hash(x, y, seed):
    """32-bit mix of integer coordinates (arrays of any equal shape) and a seed; uint64 arithmetic masked to 32 bits."""
    M = np.uint64(0xffffffff)
    v = (x.astype(np.int64) & 0xffffffff).astype(np.uint64) * np.uint64(0x9e3779b1) & M
    v ^= (y.astype(np.int64) & 0xffffffff).astype(np.uint64) * np.uint64(0x85ebca77) & M
    v ^= np.uint64((seed * 0xc2b2ae3d) & 0xffffffff)
    for mul, sh in ((0x7feb352d, 15), (0x846ca68b, 16)):
        v ^= v >> np.uint64(sh)
        v = v * np.uint64(mul) & M
    v ^= v >> np.uint64(16)
    return v.astype(np.int64)


def _lattice(x, y, seed, log2cell):
    """Value noise 0..255: hashed lattice of cell size 1 << log2cell, bilinear in integers."""
    c = 1 << log2cell
    gx, gy, fx, fy = x >> log2cell, y >> log2cell, x & (c - 1), y & (c - 1)
    g = lambda dx, dy: _hash(gx + dx, gy + dy, seed) & 255
    return (g(0, 0) * (c - fx) * (c - fy) + g(1, 0) * fx * (c - fy) + g(0, 1) * (c - fx) * fy + g(1, 1) * fx * fy) >> (2 * log2cell)


def _texture(x, y, seed, bd):
    """A texture defined at every integer world coordinate: two octaves of value noise (cells of 16 and 4) in 24..231, low bits of deeper samples hashed."""
    s = bd - 8
    v = 24 + ((5 * _lattice(x, y, seed, 4) + 3 * _lattice(x, y, seed + 1, 2)) * 13 >> 7)
    return (v << s) | (_hash(x, y, seed + 2) & ((1 << s) - 1))


def _noise(shape, seed, amp, bd):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return ((_hash(xx, yy, seed) % (2 * amp + 1)) - amp) << (bd - 8)


def _planes(w, h, bd, fy, fc):
    """Y from fy(x, y), U and V from fc(x, y, plane) on the half-size grid, clipped; one packed planar frame."""
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    mx = (1 << bd) - 1
    return np.concatenate([np.clip(p, 0, mx).astype(pix(bd)).ravel() for p in (fy(xx, yy), fc(cx, cy, 1), fc(cx, cy, 2))])


def _moving(w, h, bd, seed, disp, noise, k, rect=None):
    """Frame k (0 / 1) of a scene whose content at middle-frame position (x, y) is displaced by disp(x, y) = (dx, dy) samples from frame 0 to frame 1 (even
    numbers: half of it each way); rect = (x, y, w, h, dx, dy, seed): a rectangle of its own texture moving over it."""
    sg = 1 if k == 0 else -1

    def layer(x, y, sub, sd, plane):
        dx, dy = disp(x << sub, y << sub)
        v = _texture(x + sg * (dx >> (1 + sub)), y + sg * (dy >> (1 + sub)), sd + 10 * plane, bd)
        if rect:
            rx, ry, rw, rh, rdx, rdy, rs = rect
            px, py = (rx - sg * (rdx // 2)) >> sub, (ry - sg * (rdy // 2)) >> sub   # the rectangle's corner in this frame
            inside = (x >= px) & (x < px + (rw >> sub)) & (y >= py) & (y < py + (rh >> sub))
            v = np.where(inside, _texture(x - px, y - py, rs + 10 * plane, bd), v)
        return v + (_noise(x.shape, sd + 100 + 7 * k + plane, noise, bd) if noise else 0)
    return _planes(w, h, bd, lambda x, y: layer(x, y, 0, seed, 0), lambda x, y, p: layer(x, y, 1, seed, p))


def make_pair(case, pair, bd):
    """The two reference frames of a pair, packed planar 4:2:0 (Y, U, V)."""
    w, h = CASES[case][:2]
    const = lambda dx, dy: (lambda x, y: (np.full(x.shape, dx), np.full(x.shape, dy)))
    if pair == 'scene':    # background panning by (6, -2) and, in every other band of 32 rows, (8, -2); a 64x48 rectangle moving by (-20, 12) over it; noise of +-2
        return tuple(_moving(w, h, bd, 11, lambda x, y: (6 + 2 * ((y >> 5) & 1), np.full(x.shape, -2)), 2, k, rect=(84, 40, 64, 48, -20, 12, 500)) for k in (0, 1))
    if pair == 'pan':
        return tuple(_moving(w, h, bd, 24, const(40, 24), 0, k) for k in (0, 1))
    if pair == 'shear':    # horizontal motion per strip of 64 columns: 0 at the left, 24 at the right; vertical motion 0 / 2 / 4 / 6 per block row, so that
        steps = np.array([0, 4, 6, 10, 14, 18, 20, 24])   # a block's up-right neighbour moves differently all along a row, not only at the strip boundaries
        return tuple(_moving(w, h, bd, 37, lambda x, y: (steps[x >> 6], 2 * (y >> 4)), 1, k) for k in (0, 1))
    if pair == 'band':
        def frame(k):
            f = _moving(w, h, bd, 71, lambda x, y: (8 - 16 * ((x >> 4) & 1), np.zeros_like(x)), 0, k)
            for p, rows in zip(split(f, w, h), (16, 8, 8)):
                p[rows:] = 128 << (bd - 8)    # split returns views: the frame below the band becomes flat
            return f
        return frame(0), frame(1)
    if pair == 'same':
        f = _moving(w, h, bd, 41, const(0, 0), 0, 0)
        return f, f.copy()
    if pair == 'flat':
        f = np.full(w * h * 3 // 2, (1 << bd) - 1, dtype=pix(bd))
        return f, f.copy()
    if pair == 'noise':
        full = lambda sd: _planes(w, h, bd, lambda x, y: _hash(x, y, sd) & ((1 << bd) - 1), lambda x, y, p: _hash(x, y, sd + p) & ((1 << bd) - 1))
        return full(51), full(61)
    raise KeyError(pair)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# ---- the reference's stages restated where that spares storing them ---------------------------------------------------------------------------------
def split(yuv, w, h):
    y, u, v = np.split(yuv, [w * h, w * h + (w // 2) * (h // 2)])
    return y.reshape(h, w), u.reshape(h // 2, w // 2), v.reshape(h // 2, w // 2)


def pyramid(luma, levels):
    """scale_frame_down2x2 (temporal_interp.c:143-160, luma) + pad_yuv_frame for levels 1 .. levels-1: planes with their padding of 32."""
    out, p = [], luma.astype(np.int32)
    for _ in range(1, levels):
        ho, wo = p.shape[0] >> 1, p.shape[1] >> 1
        q = p[:2 * ho, :2 * wo]
        p = (((q[0::2, 0::2] + q[1::2, 0::2] + 1) >> 1) + ((q[0::2, 1::2] + q[1::2, 1::2] + 1) >> 1)) >> 1
        out.append(np.pad(p, PAD_PYR, mode='edge').astype(luma.dtype))
    return out


def padded(planes):
    """pad_yuv_frame of a picture: Y by PAD_Y, U and V by PAD_Y / 2, nearest picture sample."""
    return [np.pad(p, PAD_Y if k == 0 else PAD_Y // 2, mode='edge') for k, p in enumerate(planes)]


def branches(mv1, w, h, chroma):
    """The branch mot_comp_avg (temporal_interp.c:319-375) takes for every unit of the level-0 grid, from the final mv[1] field (bh, bw, 2): 0 both blocks
    inside, 1 only block 1, 2 only block 0, 3 the per-sample clamped average.  chroma: the 4x4 units with halved vectors (interpolate_comp :868-872)."""
    bh, bw = mv1.shape[:2]
    v1 = mv1.astype(np.int64)
    size, pad, wP, hP = 8, 4, w + 4, h + 4
    if chroma:
        v1, size, pad, wP, hP = v1 >> 1, 4, 2, wP >> 1, hP >> 1
    v0 = -v1
    ys, xs = np.mgrid[0:bh, 0:bw] * size
    inside = []
    for v in (v0, v1):
        x, y = xs + ((v[..., 0] + 4) >> 3), ys + ((v[..., 1] + 4) >> 3)
        inside.append((x >= -pad) & (x + size <= wP) & (y >= -pad) & (y + size <= hP))
    return np.where(inside[0] & inside[1], 0, np.where(inside[1], 1, np.where(inside[0], 2, 3)))


# ---- fixture ----------------------------------------------------------------------------------------------------------------------------------------
def fixture(bd):
    if bd not in _K:
        _K[bd] = np.load(os.path.join(GOLD, _FILES[bd]))
    return _K[bd]


def pairs_of(bd):
    return [(c, p) for c in CASES for p in CASES[c][4] if bd in CASES[c][3]]


_INPUTS = {}


def inputs(case, pair, bd):
    """The pair's frames, checked against the CRCs recorded with the answers; built once."""
    k = (case, pair, bd)
    if k not in _INPUTS:
        a, b = make_pair(case, pair, bd)
        want = fixture(bd)[f'{case}_{pair}_crc'].tolist()
        assert [crc(a), crc(b)] == want, f'case {case} {pair} bd {bd}: the generated inputs are not the ones the answers were recorded for'
        _INPUTS[k] = (a, b)
    return _INPUTS[k]


def expected(case, pair, bd):
    """Recorded answers: mv (per level a (2, bh, bw, 2) array: mv[0], mv[1]), raster (per level mv[1] before the merge pass), out (Y, U, V pictures)."""
    K, (w, h, levels) = fixture(bd), CASES[case][:3]
    k = f'{case}_{pair}_'
    mv, raster = [], []
    for l in range(levels):
        bw, bh = grid(w, h, l)
        mv.append(K[k + f'mv{l}'].reshape(2, bh, bw, 2))
        raster.append(K[k + f'raster{l}'].reshape(bh, bw, 2))
    return dict(mv=mv, raster=raster, out=split(K[k + 'out'], w, h))


# ---- what a runner returns: raw buffers of thor_hip_kat_interp_stages (include/thor_hip.h) and their shapes ---------------------------------------
def stage_sizes(w, h):
    """Samples of pyramid planes, int16 entries of vector fields and samples of the padded output, per stream."""
    levels = levels_of(w, h)
    pyr = 2 * sum(((h >> l) + 2 * PAD_PYR) * ((w >> l) + 2 * PAD_PYR) for l in range(1, levels))
    nmv = sum(4 * grid(w, h, l)[0] * grid(w, h, l)[1] for l in range(levels))
    out = (h + 2 * PAD_Y) * (w + 2 * PAD_Y) + 2 * (h // 2 + PAD_Y) * (w // 2 + PAD_Y)
    return levels, pyr, nmv, out


def unpack(w, h, pyr, nmv, out):
    """One stream's buffers as arrays: pyr[r][l - 1] padded planes, mv[l] (2, bh, bw, 2), out padded Y, U, V."""
    levels = levels_of(w, h)
    P, o = [[], []], 0
    for r in range(2):
        for l in range(1, levels):
            ph, pw = (h >> l) + 2 * PAD_PYR, (w >> l) + 2 * PAD_PYR
            P[r].append(pyr[o:o + ph * pw].reshape(ph, pw)); o += ph * pw
    M, o = [], 0
    for l in range(levels):
        bw, bh = grid(w, h, l)
        M.append(nmv[o:o + 4 * bw * bh].reshape(2, bh, bw, 2)); o += 4 * bw * bh
    O, o = [], 0
    for k in range(3):
        ph, pw = ((h + 2 * PAD_Y), (w + 2 * PAD_Y)) if k == 0 else ((h // 2 + PAD_Y), (w // 2 + PAD_Y))
        O.append(out[o:o + ph * pw].reshape(ph, pw)); o += ph * pw
    return dict(pyr=P, mv=M, out=O)


def compare(case, pair, bd, got, tag=''):
    """Mismatches of one stream's stages against the recorded answers, in stage order (empty = bit-exact): pyramid planes with padding, final vectors per
    level from the top down (the order they are computed in), picture area, borders of the padded output."""
    w, h, levels = CASES[case][:3]
    a, b = inputs(case, pair, bd)
    want = expected(case, pair, bd)
    tag = f'case {case} {pair} bd {bd} {w}x{h}{tag}'
    bad = []
    for r, f in enumerate((a, b)):
        for l, p in enumerate(pyramid(split(f, w, h)[0], levels), 1):
            g = got['pyr'][r][l - 1]
            if (g != p).any():
                i, j = (int(x[0]) for x in np.nonzero(g != p))
                bad.append(f'{tag}: stage 1 pyramid, reference {r} level {l}: {int((g != p).sum())} samples differ, first at row {i - PAD_PYR} column {j - PAD_PYR}: '
                           f'{int(g[i, j])} want {int(p[i, j])}')
    for l in range(levels - 1, -1, -1):
        g, m = got['mv'][l], want['mv'][l]
        if (g != m).any():
            k, i, j = (int(x[0]) for x in np.nonzero((g != m).any(axis=3)))
            bad.append(f'{tag}: stage 2 vectors, level {l}: {int((g != m).any(axis=3).sum())} entries differ, first nmv[{k}] unit {i * m.shape[2] + j} (row {i} column {j}): '
                       f'{g[k, i, j].tolist()} want {m[k, i, j].tolist()}')
    pic = [p[pd:p.shape[0] - pd, pd:p.shape[1] - pd] for p, pd in zip(got['out'], (PAD_Y, PAD_Y // 2, PAD_Y // 2))]
    for k, (g, p) in enumerate(zip(pic, want['out'])):
        if (g != p).any():
            i, j = (int(x[0]) for x in np.nonzero(g != p))
            bad.append(f'{tag}: stage 3 picture, plane {"YUV"[k]}: {int((g != p).sum())} samples differ, first at row {i} column {j} (unit row {i // (8 if k == 0 else 4)} '
                       f'column {j // (8 if k == 0 else 4)}): {int(g[i, j])} want {int(p[i, j])}')
    for k, (g, p) in enumerate(zip(got['out'], padded(want['out']))):
        pd = PAD_Y if k == 0 else PAD_Y // 2
        border = np.ones(p.shape, dtype=bool)
        border[pd:-pd, pd:-pd] = False
        d = (g != p) & border
        if d.any():
            i, j = (int(x[0]) for x in np.nonzero(d))
            bad.append(f'{tag}: stage 4 borders, plane {"YUV"[k]}: {int(d.sum())} samples differ, first at row {i - pd} column {j - pd}: {int(g[i, j])} want {int(p[i, j])}')
    return bad


def check(bd, items, runner, tag=''):
    """Run `items` = [(case, pair), ...] of ONE geometry as the streams of one call of `runner(yuv0, yuv1, width, height, bitdepth)` (arrays of one packed frame
    per stream; returns the three raw buffers, one row per stream) and compare every stream with its own recorded answer."""
    w, h = CASES[items[0][0]][:2]
    assert all(CASES[c][:2] == (w, h) for c, _ in items)
    fr = [inputs(c, p, bd) for c, p in items]
    pyr, nmv, out = runner(np.array([f[0] for f in fr]), np.array([f[1] for f in fr]), w, h, bd)
    bad = []
    for s, (c, p) in enumerate(items):
        bad += compare(c, p, bd, unpack(w, h, pyr[s], nmv[s], out[s]), tag=f' stream {s} of {len(items)}{tag}')
    return bad


# ---- conditions the fixture must meet: from the reference's recorded vectors alone -----------------------------------------------------------------
def fixture_figures(bd):
    """The figures the conditions are about, per (case, pair) present at this bit depth."""
    fig = {}
    for case, pair in pairs_of(bd):
        w, h = CASES[case][:2]
        e = expected(case, pair, bd)
        m1, r1 = e['mv'][0][1], e['raster'][0]
        blk = m1[0::2, 0::2]   # one entry per 16x16 block (its top-left unit)
        blk_r = r1[0::2, 0::2]
        f = dict(luma=np.bincount(branches(m1, w, h, 0).ravel(), minlength=4).tolist(), chroma=np.bincount(branches(m1, w, h, 1).ravel(), minlength=4).tolist(),
                 distinct=len({tuple(v) for v in m1.reshape(-1, 2).tolist()}),
                 upright=min(float((x[1:, :-1] != x[:-1, 1:]).any(axis=2).sum()) / (x.shape[0] * x.shape[1]) for x in (blk, blk_r)),
                 merged=float((m1 != r1).any(axis=2).mean()), zero=bool((np.concatenate([x.ravel() for x in e['mv']]) == 0).all()),
                 # blocks of the first column whose two skip-vector neighbours (up-right, up) differ and which kept the LAST of them, the upper one
                 lastmin=int(((blk_r[:-1, 0] != blk_r[:-1, 1]).any(axis=1) & (blk_r[1:, 0] == blk_r[:-1, 0]).all(axis=1)).sum()))
        fig[(case, pair)] = f
    return fig


def assert_fixture_not_trivial(bd):
    """Case B: at least 8 luma and 4 chroma units in each of the four motion-compensation branches.  Case A: at least 8 luma units in the clamped branch.
    Cases A and C, level 0: at least 6 distinct final vectors, at least 25 % of ALL 16x16 blocks with an up-right neighbour whose vector differs
    from their own - in the final field and in the raster-pass field, which is the one the search reads -, the merge pass changed at least 5 % of the 8x8 units.
    Case D: identical frames give all-zero fields, independent noise at least 4 distinct vectors.  Case E: at least one block of the first column took the
    upper of two differing neighbour vectors as its skip vector (the last minimum of mv_absdist_filter)."""
    fig = fixture_figures(bd)
    for (case, pair), f in fig.items():
        if case == 'B':
            assert min(f['luma']) >= 8 and min(f['chroma']) >= 4, (case, bd, f)
        if case == 'A':
            assert f['luma'][3] >= 8, (case, bd, f)
        if case in 'AC':
            assert f['distinct'] >= 6 and f['upright'] >= 0.25 and f['merged'] >= 0.05, (case, bd, f)
        if case == 'E':
            assert f['lastmin'] >= 1, (case, bd, f)
        if pair == 'same':
            assert f['zero'], (case, pair, bd, f)
        if pair == 'noise':
            assert f['distinct'] >= 4, (case, pair, bd, f)
    return fig
