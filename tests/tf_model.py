"""The temporal noise filter restated in numpy (include/thor_hip.h: thor_hip_temporal_filter is the normative text; thor_amd/csrc/tk_tf.h the code): block
search, block and sample weights, the blend of luma and chroma, the neighbour list of the front ends, and the cases the host twin and the device are compared on.
Integers only (int64 arrays)."""
import numpy as np

BLK, RANGE, SPAN = 8, 8, 17
B_Q8 = {1: 192, 2: 128}
MAX_REFS, MAX_STRENGTH = 4, 16


def rank(dx, dy):
    return 0 if dx == 0 and dy == 0 else 1 + (dy + RANGE) * SPAN + (dx + RANGE)


def search(cur_y, ref_y):
    """Per 8x8 block the vector of [-8, 8]^2 with the least (SAD, rank) among those whose displaced block lies inside the plane: (dx, dy, sad) arrays."""
    h, w = cur_y.shape
    bh, bw = h // BLK, w // BLK
    c = cur_y.astype(np.int64)
    r = np.zeros((h + 2 * RANGE, w + 2 * RANGE), dtype=np.int64)
    r[RANGE:RANGE + h, RANGE:RANGE + w] = ref_y
    x0 = (np.arange(bw) * BLK)[None, :]
    y0 = (np.arange(bh) * BLK)[:, None]
    best = np.full((bh, bw), np.iinfo(np.int64).max, dtype=np.int64)
    for dy in range(-RANGE, RANGE + 1):
        for dx in range(-RANGE, RANGE + 1):
            sad = np.abs(c - r[RANGE + dy:RANGE + dy + h, RANGE + dx:RANGE + dx + w]).reshape(bh, BLK, bw, BLK).sum(axis=(1, 3))
            ok = (x0 + dx >= 0) & (x0 + dx + BLK <= w) & (y0 + dy >= 0) & (y0 + dy + BLK <= h)
            key = np.where(ok, (sad << 9) | rank(dx, dy), np.iinfo(np.int64).max)
            best = np.minimum(best, key)
    rk = best & 511
    dy = np.where(rk == 0, 0, (rk - 1) // SPAN - RANGE)
    dx = np.where(rk == 0, 0, (rk - 1) % SPAN - RANGE)
    return dx, dy, best >> 9


def block_weight(sad, depth, strength, dist):
    tb = 128 * strength
    return B_Q8[dist] * np.maximum(0, tb - (sad >> (depth - 8))) // tb


def _blend_plane(cur, refs, dxs, dys, wbs, blk, depth, strength):
    """cur, refs: one plane; dxs, dys, wbs: per neighbour the per-block arrays, vectors already in this plane's units; blk: the block size in this plane."""
    h, w = cur.shape
    ts = 4 * strength
    w0 = 256 * ts
    c = cur.astype(np.int64)
    num, den = c * w0, np.full((h, w), w0, dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for ref, dx, dy, wb in zip(refs, dxs, dys, wbs):
        up = lambda a: np.repeat(np.repeat(a, blk, axis=0), blk, axis=1)
        ry, rx = yy + up(dy), xx + up(dx)
        live = up(wb) > 0                         # a block with wb = 0 reads nothing
        r = np.where(live, ref.astype(np.int64)[np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)], 0)
        assert (~live | ((ry >= 0) & (ry < h) & (rx >= 0) & (rx < w))).all()
        wt = up(wb) * np.maximum(0, ts - (np.abs(c - r) >> (depth - 8)))
        num += r * wt
        den += wt
    assert den.max() <= 1 << 16 and num.max() < 1 << 29
    return ((num + den // 2) // den).astype(cur.dtype)


def filter_frame(cur, refs, dists, depth, strength):
    """cur: (Y, U, V); refs: up to four such triples; dists: 1 or 2 each.  Returns (Y, U, V) filtered, mv int array (nrefs, bh, bw, 2) as (dx, dy), wb (nrefs, bh, bw)."""
    assert 1 <= strength <= MAX_STRENGTH and len(refs) == len(dists) <= MAX_REFS and all(d in (1, 2) for d in dists)
    h, w = cur[0].shape
    dxs, dys, wbs = [], [], []
    for ref, dist in zip(refs, dists):
        dx, dy, sad = search(cur[0], ref[0])
        dxs.append(dx); dys.append(dy); wbs.append(block_weight(sad, depth, strength, dist))
    out = [_blend_plane(cur[0], [r[0] for r in refs], dxs, dys, wbs, BLK, depth, strength)]
    for p in (1, 2):
        out.append(_blend_plane(cur[p], [r[p] for r in refs], [d >> 1 for d in dxs], [d >> 1 for d in dys], wbs, BLK // 2, depth, strength))
    mv = np.zeros((len(refs), h // BLK, w // BLK, 2), dtype=np.int32)
    wb = np.zeros((len(refs), h // BLK, w // BLK), dtype=np.int32)
    for k in range(len(refs)):
        mv[k, :, :, 0], mv[k, :, :, 1], wb[k] = dxs[k], dys[k], wbs[k]
    return tuple(out), mv, wb


def neighbours(f, n, past, future):
    """The front ends' list for frame f of an n-frame chunk: [(frame, dist)], past frames first, nearest first; frames outside the chunk are dropped."""
    return [(f - d, d) for d in range(1, past + 1) if f - d >= 0] + [(f + d, d) for d in range(1, future + 1) if f + d < n]


def filter_clip(frames, depth, strength, past, future):
    """Every frame of a chunk filtered against its neighbours (non-recursive: the inputs are the originals)."""
    out = []
    for f in range(len(frames)):
        nb = neighbours(f, len(frames), past, future)
        out.append(filter_frame(frames[f], [frames[k] for k, _ in nb], [d for _, d in nb], depth, strength)[0])
    return out


def split_frames(clip_bytes, w, h, n, depth=8):
    a = np.frombuffer(clip_bytes, dtype=np.uint8 if depth == 8 else np.dtype('<u2'))
    fsz, ny, nc = w * h * 3 // 2, w * h, (w // 2) * (h // 2)
    return [(a[i * fsz:i * fsz + ny].reshape(h, w), a[i * fsz + ny:i * fsz + ny + nc].reshape(h // 2, w // 2), a[i * fsz + ny + nc:(i + 1) * fsz].reshape(h // 2, w // 2))
            for i in range(n)]


def join_frames(frames):
    return b''.join(np.ascontiguousarray(p).tobytes() for f in frames for p in f)


# ---- the cases of the known-answer tests ----------------------------------------------------------------------------------------------------------------

SHAPES = ((16, 16), (24, 40), (136, 72))
DEPTHS = (8, 10, 12)
CONTENTS = ('random', 'max', 'identical', 'unrelated', 'flat', 'pan_8_m8', 'pan_9', 'edge_ties')
NREFS = {'random': (0, 1, 2, 3, 4)}   # every other content runs with four neighbours
DISTS = (1, 1, 2, 2)                  # neighbour k: past for even k, future for odd k


def _dtype(depth):
    return np.uint8 if depth == 8 else np.dtype('<u2')


def _yuv(rng, w, h, depth, lo=0, hi=None):
    hi = (1 << depth) if hi is None else hi
    return tuple(rng.integers(lo, hi, size=s).astype(_dtype(depth)) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))


def _texture(rng, w, h, depth, margin):
    """A smooth texture with some noise on a canvas `margin` larger on every side, at 4:2:0."""
    def plane(hh, ww):
        g = rng.integers(0, 1 << depth, size=(hh // 4 + 2, ww // 4 + 2)).astype(np.int64)
        return np.repeat(np.repeat(g, 4, axis=0), 4, axis=1)[:hh, :ww]
    H, W = h + 2 * margin, w + 2 * margin
    return plane(H, W), plane(H // 2, W // 2), plane(H // 2, W // 2)


def _crop(canvas, w, h, margin, ox, oy, depth, rng, noise):
    out = []
    for p, (c, s) in enumerate(zip(canvas, (1, 2, 2))):
        m, x, y = margin // s, ox // s, oy // s
        v = c[m + y:m + y + h // s, m + x:m + x + w // s]
        if noise:
            v = v + rng.integers(-noise, noise + 1, size=v.shape)
        out.append(np.clip(v, 0, (1 << depth) - 1).astype(_dtype(depth)))
    return tuple(out)


def kat_case(w, h, depth, content, nrefs=4):
    """(cur, refs, dists): the frames of one case, seeded by its parameters."""
    rng = np.random.default_rng([w, h, depth, CONTENTS.index(content), nrefs])
    maxv, sh = (1 << depth) - 1, depth - 8
    dists = list(DISTS[:nrefs])
    if content == 'random':   # neighbours a few code values off the current frame: weights of every size
        cur = _yuv(rng, w, h, depth)
        refs = [tuple(np.clip(p.astype(np.int64) + rng.integers(-(6 << sh), (6 << sh) + 1, size=p.shape), 0, maxv).astype(_dtype(depth)) for p in cur) for _ in range(nrefs)]
    elif content == 'max':    # every sample at the maximum: the numerator and D at their bounds
        cur = tuple(np.full(s, maxv, dtype=_dtype(depth)) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
        refs = [cur] * nrefs
    elif content == 'identical':
        cur = _yuv(rng, w, h, depth)
        refs = [cur] * nrefs
    elif content == 'unrelated':
        cur = _yuv(rng, w, h, depth)
        refs = [_yuv(rng, w, h, depth) for _ in range(nrefs)]
    elif content == 'flat':
        cur = tuple(np.full(s, 100 << sh, dtype=_dtype(depth)) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
        refs = [tuple(np.full(p.shape, (100 + k) << sh, dtype=_dtype(depth)) for p in cur) for k in range(nrefs)]
    elif content in ('pan_8_m8', 'pan_9'):   # neighbour k shows the scene displaced by the pan (even k) or its opposite (odd k)
        px, py = (8, -8) if content == 'pan_8_m8' else (9, 0)
        canvas = _texture(rng, w, h, depth, 16)
        cur = _crop(canvas, w, h, 16, 0, 0, depth, rng, 0)
        refs = [_crop(canvas, w, h, 16, px * (1 if k % 2 == 0 else -1), py * (1 if k % 2 == 0 else -1), depth, rng, 1 << sh) for k in range(nrefs)]
    else:                     # 'edge_ties': a vertical edge that moved: every vertical displacement gives the same SAD, and so do the columns beyond the edge
        def edge(at):
            y = np.zeros((h, w), dtype=np.int64); y[:, at:] = 200 << sh
            c = np.zeros((h // 2, w // 2), dtype=np.int64); c[:, at // 2:] = 150 << sh
            return y.astype(_dtype(depth)), c.astype(_dtype(depth)), c.astype(_dtype(depth))
        cur = edge(w // 2 + 3)
        refs = [edge(w // 2 + 3 + (k + 1) * (1 if k % 2 == 0 else -1)) for k in range(nrefs)]
    return cur, refs, dists


def kat_cases():
    for (w, h) in SHAPES:
        for depth in DEPTHS:
            for content in CONTENTS:
                for nrefs in NREFS.get(content, (4,)):
                    yield w, h, depth, content, nrefs


STRENGTH = 6
