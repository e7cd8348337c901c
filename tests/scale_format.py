"""Shared by tests/test_scale_format.py, tests/test_scale_streams.py and tests/test_gpu_scale.py: staging a frame of another size restated from the
text of include/thor_hip.h (thor_hip_scale) - the taps in Python integers, both passes of a whole frame in numpy int64, for a source in any
layout of tests/frame_layout.py - plus the cases the host functions and the kernel are run on.  Nothing here calls the code under test."""
import numpy as np
import frame_layout as fl

BILINEAR, BICUBIC = 0, 1
FILTER_NAMES = ['bilinear', 'bicubic']
ONE = 16384
GUARD_BITS = 2
MAX_ABS = 26214


def taps(S, T, filt, cosited, i):
    """(first source index, coefficients) of destination index i on an axis S -> T."""
    D = 2 * max(S, T)
    A = 2 if filt == BICUBIC else 1

    def num(k):
        return 2 * (i * S - k * T) if cosited else (2 * i + 1) * S - (2 * k + 1) * T
    k = (i * S) // T - 2 * A * (max(S, T) // T + 2)       # safely left of the support
    while abs(num(k)) >= A * D:
        k += 1
    first, W = k, []
    while abs(num(k)) < A * D:
        a = abs(num(k))
        if filt == BILINEAR:
            W.append(D - a)
        elif a < D:
            W.append(3 * a ** 3 - 5 * a * a * D + 2 * D ** 3)
        else:
            W.append(-a ** 3 + 5 * a * a * D - 8 * a * D * D + 4 * D ** 3)
        k += 1
    sw = sum(W)
    c = [(2 * w * ONE + sw) // (2 * sw) for w in W]     # Python's // is floor division
    c[W.index(max(W))] += ONE - sum(c)
    return first, c


_TABLES = {}


def table(S, T, filt, cosited):
    key = (S, T, filt, cosited)
    if key not in _TABLES:
        _TABLES[key] = [taps(S, T, filt, cosited, i) for i in range(T)]
    return _TABLES[key]


def _pass(X, S, T, filt, cosited, axis):
    """sum c(k) * X[k] along `axis` for every destination index, edges replicated; int64, not yet rounded."""
    X = np.moveaxis(np.asarray(X, dtype=np.int64), axis, 0)
    assert X.shape[0] == S
    out = np.empty((T,) + X.shape[1:], dtype=np.int64)
    for i, (first, c) in enumerate(table(S, T, filt, cosited)):
        idx = np.clip(np.arange(first, first + len(c)), 0, S - 1)
        out[i] = np.tensordot(np.array(c, dtype=np.int64), X[idx], axes=1)
    return np.moveaxis(out, 0, axis)


def scale_plane(P, T_w, T_h, filt, cosited_h, n):
    """One plane: horizontally, then vertically."""
    g = GUARD_BITS
    S_h, S_w = P.shape
    inter = (_pass(P, S_w, T_w, filt, cosited_h, 1) + (1 << (13 - g))) >> (14 - g)
    out = (_pass(inter, S_h, T_h, filt, 0, 0) + (1 << (13 + g))) >> (14 + g)
    return np.clip(out, 0, (1 << n) - 1)


def scale_frame(frame, sw, sh, w, h, filt, site, n):
    """A packed planar 4:2:0 frame of n-bit samples at sw x sh -> the packed planar frame at w x h that staging it stages (before widening)."""
    y, u, v = fl.planes(np.asarray(frame), sw, sh)
    o = [scale_plane(y, w, h, filt, 0, n), scale_plane(u, w // 2, h // 2, filt, site, n), scale_plane(v, w // 2, h // 2, filt, site, n)]
    return np.concatenate([p.reshape(-1) for p in o]).astype(np.uint16 if n > 8 else np.uint8)


def expect_in(buf, g, w, h, filt, site, n, bd):
    """The planes after staging `buf` (a source frame in layout g, a frame_layout.Geometry at the source size) into a w x h engine."""
    f = scale_frame(fl.unpack(buf, g), g.w, g.h, w, h, filt, site, n)
    return (f.astype(np.uint32) << (bd - n)).astype(np.uint16 if bd > 8 else np.uint8)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------

# (src_w, src_h, w, h): down by 3 and 2; up by 1.88 and 2.67 from a size that is no multiple of 8; down by 2 and 1.93; up by 1.31 and 1.33
SIZES = [(48, 32, 16, 16), (34, 18, 64, 48), (400, 232, 200, 120), (208, 120, 272, 160)]
DEPTHS = [(8, 8), (10, 10), (12, 12), (10, 8)]     # (bitdepth, input_bitdepth)
CONTENTS = ['noise', 'constant', 'columns']


def source_layouts(sw, sh, n):
    """(name, Geometry at the source size, base skew in bytes): packed planar; planar and NV12 with pitch = row + 6 bytes and the base 2 bytes off a
    16-byte boundary; with 16-bit samples also P010 (msb_aligned)."""
    B = 2 if n > 8 else 1
    out = [('planar', fl.Geometry(sw, sh, n, fl.PLANAR), 0),
           ('planar_pitch6_skew2', fl.Geometry(sw, sh, n, fl.PLANAR, 0, sw * B + 6, sw // 2 * B + 6), 2),
           ('nv12_pitch6_skew2', fl.Geometry(sw, sh, n, fl.UV, 0, sw * B + 6, sw * B + 6), 2),
           ('nv12', fl.Geometry(sw, sh, n, fl.UV), 0)]
    if n > 8:
        out.append(('p010', fl.Geometry(sw, sh, n, fl.UV, 1), 0))
    return out


def content(kind, sw, sh, n, seed=5):
    """A packed planar source frame of n-bit samples."""
    top = (1 << n) - 1
    dt = np.uint16 if n > 8 else np.uint8
    ny, nc = sw * sh, (sw // 2) * (sh // 2)
    if kind == 'noise':
        a = np.random.default_rng(seed + sw + 7 * n).integers(0, top + 1, ny + 2 * nc).astype(dt)
        a[:2] = [0, top]
        return a
    if kind == 'constant':
        return np.concatenate([np.full(ny, top * 3 // 5, dtype=dt), np.full(nc, top // 3, dtype=dt), np.full(nc, top, dtype=dt)])
    cols = lambda w_, h_: np.tile(np.where(np.arange(w_) % 2 == 0, 0, top).astype(dt), h_)    # 0, max, 0, max ...: both clamps with bicubic
    return np.concatenate([cols(sw, sh), cols(sw // 2, sh // 2), cols(sw // 2, sh // 2)])


def scale_clip(clip, sw, sh, w, h, filt, site, nframes):
    """`nframes` tight 8-bit planar frames at sw x sh -> the same at w x h (bytes)."""
    a = np.frombuffer(clip, dtype=np.uint8)
    fsz = sw * sh * 3 // 2
    return b''.join(scale_frame(a[f * fsz:(f + 1) * fsz], sw, sh, w, h, filt, site, 8).tobytes() for f in range(nframes))
