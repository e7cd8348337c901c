"""Shared by tests/test_mixed_depth.py, tests/test_gpu_mixed_depth.py and tests/golden/gen_streams_mixed.py: what can be compared with the
reference's -rf file when the input has more than 8 bits and the encoder works at a higher depth still (-bitdepth 12 -input_bitdepth 10).

The reference's write_yuv_frame (common/common_frame.c:546-654) rounds such a row into `buf16`, which it declares `uint8_t *`: every sample's
LOW BYTE lands in the first `width` bytes of the row buffer, the other `width` bytes are never written, and fwrite sends all 2 * width bytes to
the file.  So half of that file is uninitialised heap memory (its md5 is not a property of the encoder), and the half that is defined holds the
low byte of every rounded sample.  `defined_rec_bytes` extracts exactly that half from the reference's file (from_reference=True) or forms it
from a correct file of little-endian 16-bit samples (from_reference=False); the two are equal when the reconstructions are.
The whole file is pinned as well, by a second run of the reference (gen_streams_mixed.py: rec_equal_depth_md5): the same clip widened beforehand
and coded with input_bitdepth == bitdepth gives the same reconstruction inside the encoder, the reference writes that one out correctly, and
`round_to_input_depth` applies write_yuv_frame's formula to it."""
import numpy as np


def rows_of_frame(w, h):
    """Row widths (in samples) of one planar 4:2:0 frame in file order: Y rows, then U, then V."""
    return [w] * h + [w // 2] * h


def defined_rec_bytes(rec, w, h, n, from_reference):
    """The bytes of an -rf file of `n` frames with two bytes per sample that the reference defines.  from_reference: `rec` is the reference's
    own file (first half of every row); else `rec` holds correct little-endian 16-bit samples (low byte of every sample)."""
    a = np.frombuffer(rec, dtype=np.uint8)
    assert a.size == w * h * 3 * n, 'not %d frames of %dx%d 4:2:0 with two bytes per sample' % (n, w, h)
    if not from_reference:
        return a[0::2].tobytes()
    out, pos = [], 0
    for _ in range(n):
        for rw in rows_of_frame(w, h):
            out.append(a[pos:pos + rw])
            pos += 2 * rw
    return np.concatenate(out).tobytes()


def round_to_input_depth(samples, bitdepth, input_bitdepth):
    """write_yuv_frame's formula (common/common_frame.c:552, :572) on uint16 samples at `bitdepth`: saturate((v + half) >> shift, input_bitdepth)."""
    s = bitdepth - input_bitdepth
    v = (np.asarray(samples).astype(np.int64) + (1 << (s - 1))) >> s
    return np.minimum(v, (1 << input_bitdepth) - 1).astype(np.uint8 if input_bitdepth == 8 else np.uint16)


# ---- vectors for the three frame-level kernels (tests/hostsim/unit_depth.cpp on the host, the thor_hip_kat_depth_* entry points on the GPU) ----
DEPTH_PAIRS = [(10, 8), (12, 8), (12, 10)]
# 16x16: one vector per chroma row and less than a workgroup of rows; 40x24: chroma rows of 20 samples, no multiple of any 16-byte vector
DEPTH_GEOMETRIES = [(16, 16), (40, 24)]


def depth_vectors(w, h, bitdepth, input_bitdepth, seed=1):
    """(inp, a, b): a packed 4:2:0 frame of input-depth samples and two of engine-depth samples (uint16), full range.  Every plane of `a`
    starts with 0, the values around the first rounding step, the largest value that does not saturate, the ones that do (1022 and 1023 at
    (10, 8)) and ends with the maximum; `b` is `a` with noise, clipped, so that differences of both signs and saturated pairs occur."""
    rng = np.random.default_rng(seed + 1000 * bitdepth + input_bitdepth + w)
    s = bitdepth - input_bitdepth
    n, ny, nc = w * h * 3 // 2, w * h, (w // 2) * (h // 2)
    big, small = (1 << bitdepth) - 1, (1 << input_bitdepth) - 1
    inp = rng.integers(0, small + 1, n).astype(np.uint8 if input_bitdepth == 8 else np.uint16)
    a = rng.integers(0, big + 1, n).astype(np.uint16)
    half = 1 << (s - 1)
    edge = [0, half - 1, half, half + 1, (small << s) - half - 1, (small << s) - half, (small << s) + half - 1, (small << s) + half, big - 1, big]
    for off, size in ((0, ny), (ny, nc), (ny + nc, nc)):
        a[off:off + len(edge)] = edge
        a[off + size - 1] = big
        inp[off:off + 2] = [0, small]
        inp[off + size - 1] = small
    b = np.clip(a.astype(np.int64) + rng.integers(-3 * (1 << s), 3 * (1 << s) + 1, n), 0, big).astype(np.uint16)
    return inp, a, b


def depth_expected(w, h, bitdepth, input_bitdepth, inp, a, b):
    """numpy restatement of the reference: read_yuv_frame's widening (common/common_frame.c:491-499), write_yuv_frame's rounding (:557-575)
    and the per-plane sums of snr_yuv (common/snr.c:51-91).  Returns (up, down, [sse_y, sse_u, sse_v])."""
    s = bitdepth - input_bitdepth
    small = (1 << input_bitdepth) - 1

    def down(x):
        return np.minimum((x.astype(np.int64) + (1 << (s - 1))) >> s, small)
    up = (inp.astype(np.int64) << s).astype(np.uint16)
    d = down(a) - down(b)
    ny, nc = w * h, (w // 2) * (h // 2)
    sse = [int((d[o:o + k] ** 2).sum()) for o, k in ((0, ny), (ny, nc), (ny + nc, nc))]
    return up, down(a).astype(inp.dtype), sse
