#!/usr/bin/env python3
"""Known answers of the temporally interpolated reference, stage by stage: interpolate_frames(new, ref0, ref1, 2, 1) (common/temporal_interp.c:909-992) on
the cases of tests/kat_interp.py, recorded through oracle/interp_shim.c (`make -C oracle reflib interpshim`), which #includes temporal_interp.c by path and
walks its static stages in the order of interpolate_frames: the pyramid planes with their padding, per level the vector field after the raster pass and
mv[0] / mv[1] after the merge pass, the padded picture.

Asserted here, on every case and bit depth:
  * the shim's picture == what the unmodified interpolate_frames_lbd / _hbd of libthorref.so produces on the same input (the shim is pinned to the real
    entry point);
  * kat_interp.pyramid == the reference's scale_frame_down2x2_simd + pad_yuv_frame planes (so the planes need not be stored);
  * the borders of the padded picture == np.pad(picture, mode='edge') (pad_yuv_frame, enc/mainenc.c:354);
  * the conditions of kat_interp.assert_fixture_not_trivial, from the recorded vectors.

Build container only.  Writes tests/golden/kat12.npz (8 bit), kat12_10.npz, kat12_12.npz: answers plus a CRC of every input frame (the inputs come from
kat_interp.make_pair, integer arithmetic only); no file may exceed 1 MiB.  Pins thor_amd/csrc/tk_interp_dev.h on the host (tests/hostsim/kat_host_interp.cpp,
tests/test_kat_host_interp.py) and on the device (thor_hip_kat_interp_stages, tests/test_gpu_interp.py)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import kat_interp as KI   # noqa: E402

L = C.CDLL(os.path.join(ROOT, 'oracle/_ref/libthorref.so'))
SH = C.CDLL(os.path.join(ROOT, 'oracle/_ref/libinterpshim.so'))
P = lambda a: a.ctypes.data_as(C.c_void_p)


class YuvFrame(C.Structure):  # common/types.h:58-80
    _fields_ = [('y', C.c_void_p), ('u', C.c_void_p), ('v', C.c_void_p)] + [(n, C.c_int) for n in (
        'width', 'height', 'stride_y', 'stride_c', 'offset_y', 'offset_c', 'pad_hor_y', 'pad_hor_c', 'pad_ver_y', 'pad_ver_c',
        'area_y', 'area_c', 'sub', 'subsample', 'frame_num', 'bitdepth', 'input_bitdepth')]


def sfx(bd):
    return '_lbd' if bd == 8 else '_hbd'


def frame_planes(fr, bd):
    T = C.c_uint8 if bd == 8 else C.c_uint16
    h, w = fr.height, fr.width
    view = lambda p, rows, stride, cols: np.ctypeslib.as_array(C.cast(p, C.POINTER(T)), shape=(rows * stride,)).reshape(rows, stride)[:, :cols]
    return view(fr.y, h, fr.stride_y, w), view(fr.u, h // 2, fr.stride_c, w // 2), view(fr.v, h // 2, fr.stride_c, w // 2)


def make_frame(bd, w, h, planes=None):
    fr = YuvFrame()
    getattr(L, 'create_yuv_frame' + sfx(bd))(C.byref(fr), w, h, 420, KI.PAD_Y, KI.PAD_Y, bd, bd)
    if planes is not None:
        for d, s in zip(frame_planes(fr, bd), planes):
            d[:] = s
        getattr(L, 'pad_yuv_frame' + sfx(bd))(C.byref(fr))
    return fr


def public_entry(a, b, w, h, bd):
    """interpolate_frames_lbd / _hbd of libthorref.so, as gen_kat5.py calls it."""
    L.ref_init(1)
    f0, f1, fo = make_frame(bd, w, h, KI.split(a, w, h)), make_frame(bd, w, h, KI.split(b, w, h)), make_frame(bd, w, h)
    getattr(L, 'interpolate_frames' + sfx(bd))(C.byref(fo), C.byref(f0), C.byref(f1), 2, 1)
    res = np.concatenate([np.ascontiguousarray(p).ravel() for p in frame_planes(fo, bd)])
    for f in (f0, f1, fo):
        getattr(L, 'close_yuv_frame' + sfx(bd))(C.byref(f))
    return res


def record(out, case, pair, bd):
    w, h, levels = KI.CASES[case][:3]
    assert KI.levels_of(w, h) == levels, (case, KI.levels_of(w, h))
    T = KI.pix(bd)
    a, b = KI.make_pair(case, pair, bd)
    _, n_pyr, n_mv, n_out = KI.stage_sizes(w, h)
    pyr = np.zeros(n_pyr, dtype=T); mv = np.zeros(n_mv, dtype=np.int16); raster = np.zeros(n_mv // 2, dtype=np.int16); pic = np.zeros(n_out, dtype=T)
    fn = getattr(SH, 'ref_interp_stages' + ('' if bd == 8 else '_hbd'))
    got_levels = fn(P(a), P(b), w, h, bd, KI.PAD_Y, 2, 1, P(pyr), P(mv), P(raster), P(pic))
    assert got_levels == levels, (case, pair, bd, got_levels)
    g = KI.unpack(w, h, pyr, mv, pic)
    planes = [p[pd:-pd, pd:-pd] for p, pd in zip(g['out'], (KI.PAD_Y, KI.PAD_Y // 2, KI.PAD_Y // 2))]
    flat = np.concatenate([np.ascontiguousarray(p).ravel() for p in planes])
    assert (flat == public_entry(a, b, w, h, bd)).all(), f'{case} {pair} {bd}: the shim and interpolate_frames{sfx(bd)} differ'
    for r, f in enumerate((a, b)):
        for l, p in enumerate(KI.pyramid(KI.split(f, w, h)[0], levels), 1):
            assert (p == g['pyr'][r][l - 1]).all(), f'{case} {pair} {bd}: numpy pyramid differs from the reference, reference {r} level {l}'
    for p, q in zip(g['out'], KI.padded(planes)):
        assert (p == q).all(), f'{case} {pair} {bd}: pad_yuv_frame is not edge replication'
    k = f'{case}_{pair}_'
    out[k + 'crc'] = np.array([KI.crc(a), KI.crc(b)], dtype=np.int64)
    out[k + 'out'] = flat
    o = 0
    for l in range(levels):
        bw, bh = KI.grid(w, h, l)
        out[k + f'mv{l}'] = g['mv'][l].copy()
        out[k + f'raster{l}'] = raster[o:o + 2 * bw * bh].reshape(bh, bw, 2).copy(); o += 2 * bw * bh
        assert (g['mv'][l][0] == -g['mv'][l][1]).all()   # ratio 2, pos 1: scale_mv(v, -1, 1)


def main():
    for bd, name in KI._FILES.items():
        out = {}
        for case, pair in KI.pairs_of(bd):
            record(out, case, pair, bd)
        path = os.path.join(ROOT, 'tests', 'golden', name)
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) <= 1 << 20, (name, os.path.getsize(path))
        KI._K.pop(bd, None)
        for k, f in KI.fixture_figures(bd).items():
            print(bd, k, f)
        KI.assert_fixture_not_trivial(bd)
        print('wrote', name, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
