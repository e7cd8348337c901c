"""Shared by tests/test_rgb_format.py, tests/test_rgb_streams.py, tests/test_gpu_rgb.py and tests/golden/gen_streams_rgb.py: RGB frames restated in
numpy from the text of include/thor_hip.h (thor_hip_rgb_format) - where the samples lie, the integer coefficients and their derivation, RGB ->
Y'CbCr 4:2:0 with both chroma sitings, and back - plus the textbook formula in float64 and the cases the row functions and the kernels are run on.
Nothing here calls the code under test."""
import numpy as np
from mixed_depth import round_to_input_depth

RGBA, BGRA, ARGB, ABGR, RGB, BGR, PLANAR = range(7)
ORDER_NAMES = ['rgba', 'bgra', 'argb', 'abgr', 'rgb', 'bgr', 'planar']
BT601, BT709, BT2020 = 0, 1, 2
KR_KB = {BT601: (2990, 1140), BT709: (2126, 722), BT2020: (2627, 593)}   # over 10000
F, G = 24, 20       # fractional bits, RGB -> Y'CbCr and back
CANARY = 0xA5
GUARD = 64          # bytes after the frame that must come back untouched
# position of R, G, B (and of the unused sample) inside a packed pixel
POSITIONS = {RGBA: (0, 1, 2, 3), BGRA: (2, 1, 0, 3), ARGB: (1, 2, 3, 0), ABGR: (3, 2, 1, 0), RGB: (0, 1, 2, None), BGR: (2, 1, 0, None)}


def rdiv(a, b):
    """a / b rounded to nearest, halves up (a, b positive)."""
    return (2 * a + b) // (2 * b)


class Format:
    """A thor_hip_rgb_format against a w x h picture: geometry with the zeros resolved, and the fields to hand to the library."""

    def __init__(self, w, h, order, depth=8, msb=0, matrix=BT709, full=0, site=1, pitch=0, plane_stride=0):
        self.w, self.h, self.order, self.depth, self.msb, self.matrix, self.full, self.site = w, h, order, depth, msb, matrix, full, site
        self.B = 1 if depth == 8 else 2
        self.dtype = np.dtype(np.uint8) if depth == 8 else np.dtype('<u2')
        self.nch = 4 if order < RGB else 3 if order < PLANAR else 1
        self.row = w * self.B * self.nch
        self.pitch = pitch or self.row
        self.plane = (plane_stride or self.pitch * h) if order == PLANAR else 0
        self.bytes = 2 * self.plane + self.pitch * h if order == PLANAR else self.pitch * h
        self.shift = 16 - depth if msb else 0
        self.M = (1 << depth) - 1
        self.fields = dict(order=order, depth=depth, msb_aligned=msb, matrix=matrix, full_range=full, chroma_site=site, pitch=pitch,
                           plane_stride=plane_stride)

    def constants(self, n):
        """SY, SC, OY, OC for input_bitdepth n."""
        if self.full:
            return (1 << n) - 1, (1 << n) - 1, 0, 1 << (n - 1)
        return 219 << (n - 8), 224 << (n - 8), 16 << (n - 8), 1 << (n - 1)

    def coefficients(self, n):
        kr, kb = KR_KB[self.matrix]
        kg = 10000 - kr - kb
        M = self.M
        SY, SC, _, _ = self.constants(n)
        c = {}
        c['yr'] = rdiv((kr * SY) << F, 10000 * M)
        c['yb'] = rdiv((kb * SY) << F, 10000 * M)
        c['yg'] = rdiv(SY << F, M) - c['yr'] - c['yb']
        c['ub'] = rdiv(SC << F, 2 * M)
        c['ur'] = -rdiv((kr * SC) << F, 2 * (10000 - kb) * M)
        c['ug'] = -c['ub'] - c['ur']
        c['vr'] = rdiv(SC << F, 2 * M)
        c['vb'] = -rdiv((kb * SC) << F, 2 * (10000 - kr) * M)
        c['vg'] = -c['vr'] - c['vb']
        c['iy'] = rdiv(M << G, SY)
        c['rv'] = rdiv((2 * (10000 - kr) * M) << G, 10000 * SC)
        c['bu'] = rdiv((2 * (10000 - kb) * M) << G, 10000 * SC)
        c['gu'] = -rdiv((2 * kb * (10000 - kb) * M) << G, 10000 * kg * SC)
        c['gv'] = -rdiv((2 * kr * (10000 - kr) * M) << G, 10000 * kg * SC)
        return c


def format_id(f):
    return '%s%d%s_m%d%s_%s' % (ORDER_NAMES[f.order], f.depth, 'msb' if f.msb else '', f.matrix, 'full' if f.full else '', 'left' if f.site else 'centre')


# ---- where the samples lie ----------------------------------------------------------------------------------------------------------------------

def _plane_view(buf, f, k):
    """Rows of plane k (or of the packed frame) as a (h, row bytes) list of slices."""
    return [(k * f.plane + i * f.pitch, k * f.plane + i * f.pitch + (f.row if f.order != PLANAR else f.w * f.B)) for i in range(f.h)]


def unpack(buf, f):
    """(R, G, B): h x w int64 arrays of sample values out of a buffer in format f."""
    buf = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf
    if f.order == PLANAR:
        out = []
        for k in range(3):
            rows = np.stack([buf[a:b] for a, b in _plane_view(buf, f, k)])
            out.append((np.ascontiguousarray(rows).view(f.dtype).astype(np.int64) >> f.shift))
        return tuple(out)
    rows = np.stack([buf[a:b] for a, b in _plane_view(buf, f, 0)])
    px = (np.ascontiguousarray(rows).view(f.dtype).astype(np.int64) >> f.shift).reshape(f.h, f.w, f.nch)
    pr, pg, pb, _ = POSITIONS[f.order]
    return px[:, :, pr], px[:, :, pg], px[:, :, pb]


def pack(R, G, B, f, into=None):
    """(R, G, B) -> f.bytes bytes in format f; the unused sample is 2^depth - 1; padding and gaps: CANARY, or what `into` holds."""
    buf = np.full(f.bytes, CANARY, dtype=np.uint8) if into is None else into
    if f.order == PLANAR:
        for k, P in enumerate((R, G, B)):
            b = np.ascontiguousarray((P.astype(np.int64) << f.shift).astype(f.dtype)).view(np.uint8).reshape(f.h, -1)
            for i, (a, e) in enumerate(_plane_view(buf, f, k)):
                buf[a:e] = b[i]
        return buf
    px = np.full((f.h, f.w, f.nch), f.M, dtype=np.int64)
    pr, pg, pb, _ = POSITIONS[f.order]
    px[:, :, pr], px[:, :, pg], px[:, :, pb] = R, G, B
    b = np.ascontiguousarray((px << f.shift).astype(f.dtype)).view(np.uint8).reshape(f.h, -1)
    for i, (a, e) in enumerate(_plane_view(buf, f, 0)):
        buf[a:e] = b[i]
    return buf


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------------------

def _taps(P, site):
    """Sum over a chroma sample's taps, and log2 of their total weight."""
    P = P.astype(np.int64)
    w = P.shape[1]
    if site == 0:
        t = P[:, 0::2] + P[:, 1::2]
        return t[0::2] + t[1::2], 2
    E = np.concatenate([P[:, :1], P], axis=1)   # column -1 is column 0
    t = E[:, 0:w:2] + 2 * E[:, 1:w + 1:2] + E[:, 2:w + 2:2]
    return t[0::2] + t[1::2], 3


def to_yuv(R, G, B, f, n):
    """The packed planar 4:2:0 frame of n-bit samples that staging an RGB frame stages."""
    c = f.coefficients(n)
    _, _, OY, OC = f.constants(n)
    top = (1 << n) - 1
    R, G, B = (np.asarray(P).astype(np.int64) for P in (R, G, B))
    Y = np.clip((c['yr'] * R + c['yg'] * G + c['yb'] * B + (OY << F) + (1 << (F - 1))) >> F, 0, top)
    (tR, L), (tG, _), (tB, _) = _taps(R, f.site), _taps(G, f.site), _taps(B, f.site)
    sh = F + L
    U = np.clip((c['ur'] * tR + c['ug'] * tG + c['ub'] * tB + (OC << sh) + (1 << (sh - 1))) >> sh, 0, top)
    V = np.clip((c['vr'] * tR + c['vg'] * tG + c['vb'] * tB + (OC << sh) + (1 << (sh - 1))) >> sh, 0, top)
    return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(np.uint8 if n == 8 else np.uint16)


def to_rgb(frame, f, n):
    """(R, G, B) of a packed planar 4:2:0 frame of n-bit samples: chroma replicated over its quad."""
    c = f.coefficients(n)
    _, _, OY, OC = f.constants(n)
    w, h = f.w, f.h
    a = np.asarray(frame).astype(np.int64)
    ny, nc = w * h, (w // 2) * (h // 2)
    Y = a[:ny].reshape(h, w)
    U = np.repeat(np.repeat(a[ny:ny + nc].reshape(h // 2, w // 2), 2, axis=0), 2, axis=1)
    V = np.repeat(np.repeat(a[ny + nc:ny + 2 * nc].reshape(h // 2, w // 2), 2, axis=0), 2, axis=1)
    l = c['iy'] * (Y - OY) + (1 << (G - 1))
    R = np.clip((l + c['rv'] * (V - OC)) >> G, 0, f.M)
    Gn = np.clip((l + c['gu'] * (U - OC) + c['gv'] * (V - OC)) >> G, 0, f.M)
    B = np.clip((l + c['bu'] * (U - OC)) >> G, 0, f.M)
    return R, Gn, B


def textbook_yuv(R, G, B, f, n):
    """The textbook conversion in float64, not rounded: (Y, Cb, Cr) planes."""
    kr, kb = (k / 10000.0 for k in KR_KB[f.matrix])
    kg = 1.0 - kr - kb
    SY, SC, OY, OC = f.constants(n)
    r, g, b = (np.asarray(P).astype(np.float64) / f.M for P in (R, G, B))
    Y = OY + SY * (kr * r + kg * g + kb * b)
    mean = lambda P: _taps(np.asarray(P), f.site)[0].astype(np.float64) / (1 << _taps(np.asarray(P), f.site)[1]) / f.M
    mr, mg, mb = mean(R), mean(G), mean(B)
    my = kr * mr + kg * mg + kb * mb
    return Y, OC + SC * (mb - my) / (2 * (1 - kb)), OC + SC * (mr - my) / (2 * (1 - kr))


# ---- what the library must produce --------------------------------------------------------------------------------------------------------------

def expect_in(buf, f, n, bd):
    """The planes after staging `buf`: the model's 4:2:0 frame, every sample << (bitdepth - input_bitdepth)."""
    return (to_yuv(*unpack(buf, f), f, n).astype(np.uint32) << (bd - n)).astype(np.uint16 if bd > 8 else np.uint8)


def expect_out(rec, f, n, bd, into):
    """`into` after fetching the reconstruction `rec` (packed planar, bitdepth bd): rounded back to n bits, converted, written; the rest untouched."""
    r = round_to_input_depth(rec, bd, n) if bd > n else np.asarray(rec)
    pack(*to_rgb(r, f, n), f, into=into[:f.bytes])
    return into


def random_rgb(f, seed):
    """(R, G, B) of f.w x f.h: noise over the whole range on a gradient, with black, white and saturated primaries in the first pixels."""
    rng = np.random.default_rng(seed)
    M = f.M
    out = []
    for k in range(3):
        P = rng.integers(0, M + 1, (f.h, f.w)).astype(np.int64)
        P[0, :8] = [0, M, M if k == 0 else 0, M if k == 1 else 0, M if k == 2 else 0, 0 if k == 0 else M, 0 if k == 1 else M, 0 if k == 2 else M]
        out.append(P)
    return tuple(out)


def random_rec(w, h, bd, seed):
    rng = np.random.default_rng(seed)
    top = (1 << bd) - 1
    a = rng.integers(0, top + 1, w * h * 3 // 2).astype(np.uint16 if bd > 8 else np.uint8)
    a[:2] = [0, top]
    a[-1] = top
    return a


def skewed(nbytes, skew_bytes, fill=CANARY):
    """A uint8 array of nbytes whose address is skew_bytes past a 16-byte boundary."""
    raw = np.full(nbytes + 32, fill, dtype=np.uint8)
    off = (skew_bytes - raw.ctypes.data) % 16
    a = raw[off:off + nbytes]
    assert a.ctypes.data % 16 == skew_bytes % 16
    return a


def shapes(order, depth):
    """(w, h, pitch - row, plane gap, base skew in bytes) the issue's table lists: the smallest picture; a width that leaves a tail after the last
    whole vector; pitch = row + 4 and base + 4 (the unaligned path); for three samples per pixel a pitch one sample above the row (byte path); for
    planes a plane stride larger than a plane."""
    B = 1 if depth == 8 else 2
    s = [(16, 16, 0, 0, 0), (24, 16, 0, 0, 0), (72, 40, 4, 0, 4)]
    if order in (RGB, BGR):
        s.append((40, 24, B, 0, 0))
    if order == PLANAR:
        s += [(24, 16, 0, 48, 0), (40, 24, 8, 6, 0)]
    return s


def shaped(order, depth, msb, matrix, full, site, shape):
    w, h, dp, gap, skew = shape
    t = Format(w, h, order, depth, msb, matrix, full, site)
    pitch = t.row + dp if dp else 0
    plane = ((pitch or t.row) * h + gap) if gap else 0
    return Format(w, h, order, depth, msb, matrix, full, site, pitch, plane), skew


DEPTHS = [(8, 0), (10, 1), (12, 0), (16, 0)]   # (depth, msb_aligned)


# ---- the clip of tests/golden (gen_streams_rgb.py) ----------------------------------------------------------------------------------------------

def make_clip(w=80, h=48, n=4, seed=11):
    """A deterministic BGRA clip (bytes): gradients that move by 2 pixels a frame, plus seeded noise of +-6; alpha 255."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    noise = rng.integers(-6, 7, (3, h, w))
    frames = []
    for t in range(n):
        R = np.clip(40 + 2 * ((xx + 2 * t) % w) + noise[0], 0, 255)
        Gc = np.clip(30 + 4 * ((yy + t) % h) + noise[1], 0, 255)
        B = np.clip(200 - ((xx + yy + 3 * t) % 64) * 3 + noise[2], 0, 255)
        frames.append(pack(R, Gc, B, Format(w, h, BGRA)).tobytes())
    return b''.join(frames)
