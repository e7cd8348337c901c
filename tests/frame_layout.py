"""Shared by tests/test_frame_layout.py and tests/test_gpu_frame_layout.py: frames in a caller's layout (NV12 / NV21 / P010, a row pitch, planes at
explicit offsets) restated in numpy - slicing and interleaving, >> and << - and the grid of cases the row functions and the kernels are run on.
Nothing here calls the code under test."""
import numpy as np
from mixed_depth import round_to_input_depth

PLANAR, UV, VU = 0, 1, 2
CANARY = 0xA5
GUARD = 64   # bytes after the layout that must come back untouched

# 16x16: 8-sample chroma rows, the smallest picture; 208x120: 104-sample chroma rows, no multiple of 16 or 64 (vector tail, idle lanes in the last
# pass); 192x128: every row a whole number of vectors
SIZES = [(16, 16), (208, 120), (192, 128)]
# (chroma, msb_aligned, input_bitdepth, bitdepth, planes at explicit offsets with gaps)
LAYOUTS = [(UV, 0, 8, 8, False), (VU, 0, 8, 8, False), (UV, 0, 8, 10, False), (UV, 1, 10, 10, False), (UV, 1, 10, 12, False), (UV, 1, 12, 12, False),
           (PLANAR, 1, 10, 10, False), (PLANAR, 0, 8, 8, True)]
PITCHES = ['tight', 'round256', 'plus1']   # row bytes; rounded up to 256; plus one sample (no row but the first is 16-byte aligned)
SKEWS = [0, 1]                             # the base: on a 16-byte boundary, one sample off it


def layout_id(l):
    return '%s%s_in%d_bd%d%s' % (['planar', 'uv', 'vu'][l[0]], '_msb' if l[1] else '', l[2], l[3], '_gaps' if l[4] else '')


class Geometry:
    """Where the rows of a w x h 4:2:0 frame lie (bytes): what include/thor_hip.h says about thor_hip_frame_layout, zeros resolved."""

    def __init__(self, w, h, inp, chroma, msb=0, pitch_y=0, pitch_c=0, offset_u=0, offset_v=0):
        self.w, self.h, self.inp, self.chroma, self.msb = w, h, inp, chroma, msb
        self.B = 2 if inp > 8 else 1
        self.dtype = np.dtype('<u2') if inp > 8 else np.dtype(np.uint8)
        self.row_y = w * self.B
        self.row_c = self.row_y // 2 if chroma == PLANAR else self.row_y
        self.pitch_y = pitch_y or self.row_y
        self.pitch_c = pitch_c or self.row_c
        ch = h // 2
        self.off_u = offset_u or self.pitch_y * h
        self.off_v = (offset_v or self.off_u + self.pitch_c * ch) if chroma == PLANAR else None
        ends = [self.pitch_y * h, self.off_u + self.pitch_c * ch] + ([self.off_v + self.pitch_c * ch] if chroma == PLANAR else [])
        self.bytes = max(ends)
        self.shift = 16 - inp if msb else 0
        self.fields = dict(chroma=chroma, msb_aligned=msb, pitch_y=pitch_y, pitch_c=pitch_c, offset_u=offset_u, offset_v=offset_v)


def case_geometry(w, h, layout, pitch):
    chroma, msb, inp, _, gaps = layout
    g = Geometry(w, h, inp, chroma, msb)
    if pitch == 'round256':
        py, pc = -(-g.row_y // 256) * 256, -(-g.row_c // 256) * 256
    elif pitch == 'plus1':
        py, pc = g.row_y + g.B, g.row_c + g.B
    else:
        py, pc = 0, 0
    ou = ov = 0
    if gaps:   # a gap of 32 bytes after luma and of 48 after U
        t = Geometry(w, h, inp, chroma, msb, py, pc)
        ou = t.pitch_y * h + 32
        ov = ou + t.pitch_c * (h // 2) + 48
    return Geometry(w, h, inp, chroma, msb, py, pc, ou, ov)


def planes(frame, w, h):
    """Y, U, V of a packed planar 4:2:0 frame as 2-D views."""
    ny, nc = w * h, (w // 2) * (h // 2)
    return frame[:ny].reshape(h, w), frame[ny:ny + nc].reshape(h // 2, w // 2), frame[ny + nc:ny + 2 * nc].reshape(h // 2, w // 2)


def _put(buf, off, pitch, rows, g):
    b = np.ascontiguousarray((rows.astype(np.uint32) << g.shift).astype(g.dtype)).view(np.uint8).reshape(rows.shape[0], -1)
    for i in range(b.shape[0]):
        buf[off + i * pitch:off + i * pitch + b.shape[1]] = b[i]


def _get(buf, off, pitch, nrows, rowbytes, g):
    rows = np.stack([buf[off + i * pitch:off + i * pitch + rowbytes] for i in range(nrows)])
    return np.ascontiguousarray(rows).view(g.dtype) >> g.shift


def pack(frame, g, into=None):
    """A packed planar frame of input-depth samples -> g.bytes bytes in layout g (padding and gaps: CANARY, or what `into` holds)."""
    y, u, v = planes(np.asarray(frame), g.w, g.h)
    buf = np.full(g.bytes, CANARY, dtype=np.uint8) if into is None else into
    _put(buf, 0, g.pitch_y, y, g)
    if g.chroma == PLANAR:
        _put(buf, g.off_u, g.pitch_c, u, g)
        _put(buf, g.off_v, g.pitch_c, v, g)
    else:
        uv = np.empty((g.h // 2, g.w), dtype=u.dtype)
        uv[:, 0::2], uv[:, 1::2] = (u, v) if g.chroma == UV else (v, u)
        _put(buf, g.off_u, g.pitch_c, uv, g)
    return buf


def unpack(buf, g):
    """The inverse: a packed planar frame of input-depth samples out of a buffer in layout g."""
    buf = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf
    y = _get(buf, 0, g.pitch_y, g.h, g.row_y, g)
    if g.chroma == PLANAR:
        u, v = _get(buf, g.off_u, g.pitch_c, g.h // 2, g.row_c, g), _get(buf, g.off_v, g.pitch_c, g.h // 2, g.row_c, g)
    else:
        uv = _get(buf, g.off_u, g.pitch_c, g.h // 2, g.row_c, g)
        u, v = (uv[:, 0::2], uv[:, 1::2]) if g.chroma == UV else (uv[:, 1::2], uv[:, 0::2])
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).astype(g.dtype)


def convert_clip(clip, g, n, back=False):
    """`n` tight frames: planar -> layout g, or (back) layout g -> planar.  For tight layouts both have the same size."""
    a = np.frombuffer(clip, dtype=np.uint8)
    fsz = g.w * g.h * 3 // 2 * g.B
    assert g.bytes == fsz and a.size >= n * fsz
    if back:
        return b''.join(unpack(a[f * fsz:(f + 1) * fsz], g).tobytes() for f in range(n))
    return b''.join(pack(a[f * fsz:(f + 1) * fsz].view(g.dtype), g).tobytes() for f in range(n))


def vectors(w, h, inp, bd, seed=3):
    """(frame_in, frame_rec): full-range packed planar frames of input-depth and of engine-depth samples; every plane starts with 0 and the maximum
    and, where the depths differ, holds the values around the rounding step and the ones that saturate."""
    rng = np.random.default_rng(seed + 100 * inp + bd + w)
    n = w * h * 3 // 2
    small, big = (1 << inp) - 1, (1 << bd) - 1
    fin = rng.integers(0, small + 1, n).astype(np.uint16 if inp > 8 else np.uint8)
    rec = rng.integers(0, big + 1, n).astype(np.uint16 if bd > 8 else np.uint8)
    ny, nc = w * h, (w // 2) * (h // 2)
    s = bd - inp
    edge = [0, big] + ([(1 << (s - 1)) - 1, 1 << (s - 1), (small << s) + (1 << (s - 1)) - 1, (small << s) + (1 << (s - 1)), big - 1] if s else [])
    for off, size in ((0, ny), (ny, nc), (ny + nc, nc)):
        fin[off:off + 2] = [0, small]
        fin[off + size - 1] = small
        rec[off:off + len(edge)] = edge
        rec[off + size - 1] = big
    return fin, rec


def expect_in(fin, inp, bd):
    """What staging leaves in the planes: x << (bitdepth - input_bitdepth)."""
    return (fin.astype(np.uint32) << (bd - inp)).astype(np.uint16 if bd > 8 else np.uint8)


def expect_out(rec, inp, bd):
    """What fetching writes, before the layout's own shift: the reconstruction rounded and saturated to the input depth (tests/mixed_depth.py)."""
    return round_to_input_depth(rec, bd, inp) if bd > inp else rec


def skewed(nbytes, skew_bytes, fill=CANARY):
    """A uint8 array of nbytes whose address is skew_bytes past a 16-byte boundary."""
    raw = np.full(nbytes + 32, fill, dtype=np.uint8)
    off = (skew_bytes - raw.ctypes.data) % 16
    a = raw[off:off + nbytes]
    assert a.ctypes.data % 16 == skew_bytes % 16
    return a
