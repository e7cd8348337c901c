#!/usr/bin/env python3
"""Known answers of the reference's motion search: motion_estimate (enc/encode_block.c:517-711) and motion_estimate_bi (:798-913), both file-static and reached
through oracle/refshim.c (ref_motion_estimate / ref_motion_estimate_bi in oracle/_ref/libthorref.so, the 16-bit build of the same wrappers in
libthorref_hbd.so), called as search_inter_prediction_params calls them (:1033-1095): the original block is the coding block's compact copy (stride = CB size),
the reference pointer sits at the PU position, xpos / ypos at the CB position, use_simd = 1.  Build container only (`make -C oracle reflib`); writes
tests/golden/kat8.npz.  Pins the host build of the device search (tests/hostsim/kat_host_me.cpp, tests/test_kat_host.py) and the device search itself
(thor_hip_kat_motion_estimate / _bi, tests/test_gpu_kat.py).

One current / reference frame pair of 320x192 luma per bitdepth (8 and 10; plus the second reference of the joint search): the texture of
tests/hostsim/unit_me_lanes.cpp, the current frame displaced by (5, -3) samples plus noise, and three full-width bands that create exact ties - flat, period-2
columns, period-4 columns.  The reference planes carry the replicate padding k_make_ref produces (rebuilt from the frames with np.pad by the tests).

Per item (rows of me{bd}_par / bi{bd}_par): cb_x, cb_y, cb, pu_dx, pu_dy, pw, ph, mvc.x, mvc.y, mvp.x, mvp.y, sign, enable_bipred, encoder_speed, ncand, cand_off,
stage ("stage the CB window first": me_stage_cb_window centred on mvc).  *_lam: lambda (double).  *_cand: full-pel list entries (x, y), item i owns
[cand_off, cand_off + ncand) (bi: six slots, the unused ones hold a sentinel the call must overwrite).  *_out: mv.x, mv.y, cost.  bi{bd}_list: the six slots
as the call leaves them.  me{bd}_cov: per item - winner from the candidate list, sub-pel winner, winner changed by clip_mv, number of exact cost ties between
distinct candidates the full-pel scan met (found by replaying the scan with the oracle's C SAD, oracle/thor_oracle.c)."""
import ctypes as C, os, sys, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
W, H, PAD = 320, 192, 160
PITCH = W + 2 * PAD
BANDS = ((72, 96), (96, 120), (120, 144))   # rows of the flat / period-2 / period-4 band
SENTINEL = (77, -77)
SHAPES = [(4, 4, 8), (8, 8, 8), (8, 4, 8), (4, 8, 8), (16, 16, 16), (16, 8, 16), (8, 16, 16), (32, 32, 32), (32, 16, 32), (16, 32, 32), (32, 8, 32), (8, 32, 32)]
SHAPES_BIG = [(64, 64, 64), (64, 32, 64), (128, 128, 128), (128, 64, 128)]   # 8 bit: keep the 64-lane row-segment evaluator on the plane
LAMS = (2.1, 9.5, 28.3)


def aligned(shape, dtype, align=64):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(n + align, dtype=np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off:off + n].view(dtype).reshape(shape)


def frames(bd):
    """cur, ref0, ref1 (H x W).  8 bit: the texture of unit_me_lanes.cpp; 10 bit: 4 * the 8-bit frames + two noise bits.  No noise inside the bands."""
    rng = np.random.default_rng(8080)
    x = np.arange(W)[None, :].astype(np.float64) + np.zeros((H, 1)); y = np.arange(H)[:, None].astype(np.float64) + np.zeros((1, W))
    tex = lambda x, y: np.clip(128 + np.trunc(50.0 * np.sin(x * 0.07) * np.cos(y * 0.05) + 30.0 * np.sin(x * 0.31 + y * 0.23) + 14.0 * np.sin(x * 1.3) * np.sin(y * 1.1)), 0, 255).astype(np.int64)
    ref0 = tex(x, y)
    cur = np.clip(tex(x + 5, y - 3) + rng.integers(0, 4, size=(H, W)) - 1, 0, 255)
    ref1 = tex(x + 10, y - 6)
    n16 = rng.integers(0, 4, size=(3, H, W))
    xi = np.arange(W)[None, :] + np.zeros((H, 1), dtype=np.int64)
    band = [np.full((H, W), 90), np.where(xi % 2 == 0, 64, 192), np.where(xi % 4 < 2, 0, 255)]
    out = []
    for k, f in enumerate((cur, ref0, ref1)):
        if bd > 8:
            f = f * 4 + n16[k]
        for (r0, r1), b in zip(BANDS, band):
            f[r0:r1] = (b * (4 if bd > 8 else 1))[r0:r1]
        out.append(np.ascontiguousarray(f.astype(np.uint16 if bd > 8 else np.uint8)))
    return out


def padded(f):
    """Replicate padding of PAD samples on every side inside a larger buffer (slack rows for the reference's SIMD loads); returns (buffer, address of sample (0, 0))."""
    p = np.pad(f, PAD, mode='edge')
    buf = aligned((p.shape[0] + 16, PITCH), f.dtype)
    buf[8:8 + p.shape[0]] = p
    return buf, buf.ctypes.data + ((8 + PAD) * PITCH + PAD) * f.dtype.itemsize


def tdiv4(v):
    return -((-v) // 4) if v < 0 else v // 4


def clip_mv(mx, my, ypos, xpos, size, sign):
    ext = PAD - 16
    y, x = (-my, -mx) if sign else (my, mx)
    if ypos + tdiv4(y) < -ext: y = 4 * (-ext - ypos)
    if ypos + tdiv4(y) + size > H + ext: y = 4 * (H + ext - ypos - size)
    if xpos + tdiv4(x) < -ext: x = 4 * (-ext - xpos)
    if xpos + tdiv4(x) + size > W + ext: x = 4 * (W + ext - xpos - size)
    return (-x, -y) if sign else (x, y)


class Replay:
    """The full-pel scan of motion_estimate (telescope, candidate list, hexagon) restated with the oracle's C SAD: which stage the full-pel winner came from,
    whether clip_mv changed it, and how many exact cost ties between distinct candidates the scan met."""

    def __init__(self, O, bd, ref_addr):
        self.O, self.bd, self.S = O, bd, 2 if bd > 8 else 1
        self.sad = O.orc_sad16 if bd > 8 else O.orc_sad
        self.wsad = O.orc_widesad16 if bd > 8 else O.orc_widesad
        self.ref_addr = ref_addr

    def run(self, q, lam, cands, orig_addr):
        cbx, cby, cb, pdx, pdy, pw, ph, mcx, mcy, mpx, mpy, sign, bip, speed = [int(v) for v in q[:14]]
        s = -1 if sign else 1
        rp = self.ref_addr + ((cby + pdy) * PITCH + cbx + pdx) * self.S
        st = {'min': 0xffffffff, 'opt': None, 'ties': 0, 'src': None, 'clipped': 0}
        xv = C.c_int()

        def ev(mx, my, wide, src):
            cx, cy = clip_mv(mx, my, cby, cbx, cb, sign)
            clipped = (cx, cy) != (mx, my)
            p = C.c_void_p(rp + (s * (cx >> 2) + s * (cy >> 2) * PITCH) * self.S)
            if wide:
                sad = self.wsad(C.c_void_p(orig_addr), cb, p, PITCH, pw, ph, C.byref(xv))
                cx += (s * xv.value) << 2
            else:
                sad = self.sad(C.c_void_p(orig_addr), cb, p, PITCH, pw, ph)
            cost = (sad >> (self.bd - 8)) + int(lam * float(self.O.orc_quote_mv_bits(cy - mpy, cx - mpx)) + 0.5)
            if cost == st['min'] and (cx, cy) != st['opt']:
                st['ties'] += 1
            if cost < st['min']:
                st.update(min=cost, opt=(cx, cy), src=src, clipped=int(clipped))
                return True
            return False
        ref = (((mcx + 2) >> 2) << 2, ((mcy + 2) >> 2) << 2)
        if (cb == 16 and bip) or speed == 0:
            step = 32
            while step >= 4:
                for k in range(-2 * step, 2 * step + 1, step):
                    for l in range(-2 * step, 2 * step + 1, step):
                        if step < 32 and not k and not l:
                            continue
                        ev(ref[0] + l, ref[1] + k, step == 32 and cb == 16 and speed == 1, 'tele')
                ref = st['opt']
                step >>= 1
        for (cx, cy) in cands:
            ev(int(cx) << 2, int(cy) << 2, cb == 16, 'list')
        ref = st['opt']
        maxsteps = 6 if (cb <= 16 or speed == 0) else 0
        start, end = 0, 5
        diy, dix = (1, 2, 1, -1, -2, -1), (-1, 0, 1, 1, 0, -1)
        for _ in range(1, maxsteps):
            d, best = start - 1, -1
            while True:
                d = 0 if d + 1 == 6 else d + 1
                if ev(ref[0] + diy[d] * 4, ref[1] + dix[d] * 4, False, 'hex'):
                    best = d
                if d == end:
                    break
            ref = st['opt']
            start = best - 1 if best else 5
            end = (start + 2) % 6
            if best < 0:
                break
        return st


def me_items(bd, rng):
    """(par rows without cand_off, lambda, candidate list) of every motion_estimate item."""
    items = []
    shapes = SHAPES + (SHAPES_BIG if bd == 8 else [])
    true_mv = lambda sign: (-20, 12) if sign else (20, -12)

    def add(cbx, cby, cb, pdx, pdy, pw, ph, mvc, mvp, sign, bip, speed, lam, cands, stage):
        if speed > 0 and not (cb == 16 and bip) and len(cands) == 0:   # the encoder never searches an empty list there (the predictor is added first): mv_opt would be uninitialised
            cands = [((mvp[0] + 2) >> 2, (mvp[1] + 2) >> 2)]
        items.append(([cbx, cby, cb, pdx, pdy, pw, ph, mvc[0], mvc[1], mvp[0], mvp[1], sign, bip, speed, len(cands), 0, stage], lam, [(int(a), int(b)) for a, b in cands]))

    def positions(cb):
        g = 8
        xm, ym = W - cb, H - cb
        rx = lambda: int(rng.integers(1, max(2, xm // g))) * g
        ry = lambda: int(rng.integers(1, max(2, ym // g))) * g
        pos = [(0, 0), (xm, 0), (0, ym), (xm, ym), (rx() if xm else 0, 0), (rx() if xm else 0, ym), (0, ry() if ym else 0), (xm, ry() if ym else 0), (rx(), ry()), (rx(), ry())]
        if cb <= 16:   # inside the tie bands (block and its near candidates)
            pos += [(rx(), b[0] + (8 if cb == 8 else 8 * int(rng.integers(0, 2)))) for b in BANDS] + [(rx(), BANDS[int(rng.integers(0, 3))][0])]
        else:
            pos += [(rx(), 72), (rx(), 96 if cb <= 32 else 64)]
        return [(min(max(x, 0), xm), min(max(y, 0), ym)) for x, y in pos]

    def predictor(kind, sign, cbx, cby, cb):
        t = true_mv(sign)
        if kind == 0: return t
        if kind == 1: return (t[0] + (1 if sign else -1) * (int(rng.integers(0, 8)) - 12), t[1] + int(rng.integers(0, 8)) - 4)
        if kind == 2: return (0, 0)
        if kind == 3: return (int(rng.integers(-80, 81)), int(rng.integers(-48, 49)))
        # far beyond the frame, towards the nearest frame edges: clip_mv changes the candidates (and the padding there is flat: ties)
        s = -1 if sign else 1
        dx = -(cbx + PAD - 16) * 4 - int(rng.integers(0, 120)) if cbx < W // 2 else (W + PAD - 16 - cbx - cb) * 4 + int(rng.integers(0, 120))
        dy = -(cby + PAD - 16) * 4 - int(rng.integers(0, 120)) if cby < H // 2 else (H + PAD - 16 - cby - cb) * 4 + int(rng.integers(0, 120))
        m = int(rng.integers(0, 3))
        return (s * dx if m != 1 else t[0], s * dy if m != 0 else t[1])

    def near_list(n, sign, centre):
        """n full-pel entries: the true motion, its neighbours, telescope grid points of the centre, scattered ones."""
        t = true_mv(sign)
        c = ((centre[0] + 2) >> 2, (centre[1] + 2) >> 2)
        out = []
        for k in range(n):
            m = k % 4
            if m == 0: out.append((t[0] // 4 + int(rng.integers(-2, 3)), t[1] // 4 + int(rng.integers(-2, 3))))
            elif m == 1: out.append((c[0] + int(rng.integers(-2, 3)) * int(rng.choice([8, 4, 2, 1])), c[1] + int(rng.integers(-2, 3)) * int(rng.choice([8, 4, 2, 1]))))   # on a telescope grid of the first step
            elif m == 2: out.append((int(rng.integers(-24, 25)), int(rng.integers(-16, 17))))
            else: out.append((t[0] // 4 + int(rng.integers(-6, 7)), t[1] // 4))
        if n:
            out[int(rng.integers(0, n))] = (t[0] // 4, t[1] // 4)
        return out

    def pu_off(pw, ph, cb):
        return int(rng.integers(0, cb // pw)) * pw, int(rng.integers(0, cb // ph)) * ph

    # A: every PU shape x positions x predictors; sign, filter set, lambda, list length and speed cycle
    k = 0
    for (pw, ph, cb) in shapes:
        for (cbx, cby) in positions(cb):
            for kind in ((0, 1, 2, 3, 4) if cb <= 32 else (0, 3, 4)):
                if bd > 8 and (k % 5) in (1, 3) and kind in (1, 2):
                    k += 1
                    continue
                sign, bip, lam = (k // 2) & 1, 0 if k % 7 == 3 else 1, LAMS[k % 3]
                speed = (0, 0, 0, 1, 0, 2, 0, 0)[k % 8]
                mvp = predictor(kind, sign, cbx, cby, cb)
                mvc = (mvp[0] + 6, mvp[1] - 9) if k % 5 == 4 else mvp
                n = (0, 1, 0, 5, 0, 2)[k % 6]
                pdx, pdy = pu_off(pw, ph, cb)
                add(cbx, cby, cb, pdx, pdy, pw, ph, mvc, mvp, sign, bip, speed, lam, near_list(n, sign, mvc), 0)
                k += 1
    # B: candidate lists of 0 / 1 / 5 / 13 (> kMeWideChunk) / 48 entries; 16x16 CBs take widesad, also inside the tie bands
    for rep in range(3 if bd == 8 else 1):
        for cb in (16, 16, 8, 32):
            for n in (0, 1, 5, 13, 48):
                for where in range(4):
                    sign, lam = (k >> 1) & 1, LAMS[k % 3]
                    xm, ym = W - cb, H - cb
                    cbx = int(rng.integers(0, xm // 8 + 1)) * 8
                    cby = (int(rng.integers(0, ym // 8 + 1)) * 8, BANDS[0][0] + 4, BANDS[1][0] + 4, BANDS[2][0] + 4)[where] if cb <= 16 else int(rng.integers(0, ym // 8 + 1)) * 8
                    kind = (3, 2, 1, 3)[k % 4]   # mostly off the true motion: the list holds it
                    mvp = predictor(kind, sign, cbx, cby, cb)
                    speed = (0, 1, 0, 2, 0)[k % 5]
                    pw, ph = ((cb, cb), (cb, cb), (cb, cb // 2), (cb // 2, cb))[k % 4] if rep else (cb, cb)
                    pdx, pdy = pu_off(pw, ph, cb)
                    add(cbx, cby, cb, pdx, pdy, pw, ph, mvp, mvp, sign, 1 if k % 6 else 0, speed, lam, near_list(n, sign, mvp), 0)
                    k += 1
    # C: HOR / VER / QUAD sets of one CB searched from one centre with the CB window staged (the later PUs take the first one's vector as predictor)
    for cb in ((8, 16, 32, 64) if bd == 8 else (8, 16, 32)):
        for (cbx, cby) in positions(cb)[:8 if bd == 8 else 4]:
            sign, lam, kind = k & 1, LAMS[k % 3], (0, 1, 3, 0, 4)[k % 5]
            mvc = predictor(kind, sign, cbx, cby, cb)
            cands = near_list((0, 2, 5)[k % 3], sign, mvc)
            speed = 1 if k % 9 == 8 else 0   # (the staged window is not used at encoder_speed > 0)
            h = cb // 2
            for (pdx, pdy, pw, ph) in ((0, 0, cb, h), (0, h, cb, h), (0, 0, h, cb), (h, 0, h, cb), (0, 0, h, h), (h, 0, h, h), (0, h, h, h), (h, h, h, h)):
                mvp = mvc if (pdx, pdy) == (0, 0) else true_mv(sign)
                add(cbx, cby, cb, pdx, pdy, pw, ph, mvc, mvp, sign, 1, speed, lam, cands, 1)
            k += 1
    # D: encoder_speed 1 and 2 (tk_me_fastsub.h; speed 1 with a 16x16 CB and bipred takes the widesad first ring)
    for rep in range(2 if bd == 8 else 1):
        for (pw, ph, cb) in SHAPES[1:] + (SHAPES_BIG[:2] if bd == 8 else []):
            for speed in (1, 2):
                for (cbx, cby) in positions(cb)[3::3]:
                    sign, lam, kind = k & 1, LAMS[k % 3], k % 4
                    mvp = predictor(kind, sign, cbx, cby, cb)
                    pdx, pdy = pu_off(pw, ph, cb)
                    add(cbx, cby, cb, pdx, pdy, pw, ph, mvp, mvp, sign, 0 if k % 5 == 2 else 1, speed, lam, near_list((1, 3, 0)[k % 3], sign, mvp), 0)
                    k += 1
    return items


def bi_items(bd, rng):
    items = []
    k = 0
    for rep in range(2 if bd == 8 else 1):
        for cb in (8, 16, 32, 64):
            for n in range(7):
                for where in range(4):
                    sign, lam = k & 1, LAMS[k % 3]
                    xm, ym = W - cb, H - cb
                    t = (-20, 12) if sign else (20, -12)
                    if where == 3:   # bottom / right blocks, centre far up / left (for ref0's sign): the second clip (1 - sign) changes the vector
                        cbx, cby = (xm, ym) if k % 3 == 0 else (int(rng.integers(0, xm // 8 + 1)) * 8, ym) if k % 3 == 1 else (xm, int(rng.integers(0, ym // 8 + 1)) * 8)
                        s = -1 if sign else 1
                        far = (-s * int(rng.integers(600, 1100)), -s * int(rng.integers(600, 1100)))
                        mvc = (far[0] if cbx == xm else t[0], far[1] if cby == ym else t[1])
                    else:
                        cbx, cby = (int(rng.integers(0, xm // 8 + 1)) * 8, int(rng.integers(0, ym // 8 + 1)) * 8) if where else ((0, 0), (xm, 0), (0, ym), (xm, ym))[k % 4]
                        mvc = (t, (t[0] + int(rng.integers(-9, 10)), t[1] + int(rng.integers(-9, 10))), (0, 0), (int(rng.integers(-80, 81)), int(rng.integers(-48, 49))))[k % 4]
                    mvp = (mvc[0] + 6, mvc[1] - 9) if k % 5 == 4 else mvc
                    # (motion_estimate_bi reads the list's full-pel entries as quarter-pel vectors)
                    cands = [(t[0] + int(rng.integers(-6, 7)), t[1] + int(rng.integers(-6, 7))) if c % 2 == 0 else (int(rng.integers(-40, 41)), int(rng.integers(-40, 41))) for c in range(n)]
                    if where == 3 and n:
                        cands[0] = (mvc[0] + int(rng.integers(-4, 5)), mvc[1] + int(rng.integers(-4, 5)))
                    items.append(([cbx, cby, cb, 0, 0, cb, cb, mvc[0], mvc[1], mvp[0], mvp[1], sign, 0 if k % 11 == 5 else 1, 0, n, 6 * len(items), 0], lam, cands + [SENTINEL] * (6 - n)))
                    k += 1
    return items


def main():
    from util import build_oracle_c
    O = build_oracle_c()
    libs = {8: C.CDLL(os.path.join(ROOT, 'oracle/_ref/libthorref.so')), 10: C.CDLL(os.path.join(ROOT, 'oracle/_ref/libthorref_hbd.so'))}
    out = {}
    for bd in (8, 10):
        L = libs[bd]
        me = getattr(L, 'ref_motion_estimate' + ('_hbd' if bd > 8 else ''))
        mebi = getattr(L, 'ref_motion_estimate_bi' + ('_hbd' if bd > 8 else ''))
        me.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double] + [C.c_int] * 7 + [C.c_void_p, C.c_int, C.c_int]
        mebi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double] + [C.c_int] * 7 + [C.c_void_p, C.c_int, C.c_int]
        T, S = (np.uint16, 2) if bd > 8 else (np.uint8, 1)
        cur, ref0, ref1 = frames(bd)
        out[f'f{bd}_cur'], out[f'f{bd}_ref'], out[f'f{bd}_ref1'] = cur, ref0, ref1
        (b0, a0), (b1, a1) = padded(ref0), padded(ref1)
        org = aligned((128 * 128,), T)
        rng = np.random.default_rng(80800 + bd)
        rep = Replay(O, bd, a0)
        par, lams, cand, res, cov = [], [], [], [], []
        for q, lam, cl in me_items(bd, rng):
            cbx, cby, cb, pdx, pdy, pw, ph = q[:7]
            assert 0 <= cbx and cbx + cb <= W and 0 <= cby and cby + cb <= H and pdx + pw <= cb and pdy + ph <= cb, q
            org[:cb * cb] = cur[cby:cby + cb, cbx:cbx + cb].reshape(-1)
            oa = org.ctypes.data + (pdy * cb + pdx) * S
            io = np.array([q[7], q[8], q[9], q[10], 0, 0], dtype=np.int16)
            ca = np.array(cl, dtype=np.int16).reshape(-1, 2)
            cost = me(oa, a0 + ((cby + pdy) * PITCH + cbx + pdx) * S, cb, PITCH, pw, ph, io.ctypes.data, lam, q[13], bd, q[11], W, H, cbx, cby, ca.ctypes.data if len(cl) else None, len(cl), q[12])
            st = rep.run(q, lam, cl, oa)
            fx, fy = st['opt']
            assert abs(int(io[4]) - fx) <= 3 and abs(int(io[5]) - fy) <= 3 and cost <= st['min'], ('full-pel replay disagrees with the reference', q, io.tolist(), cost, st)
            q[15] = len(cand)
            par.append(q); lams.append(lam); cand += cl; res.append((int(io[4]), int(io[5]), cost))
            cov.append((int(st['src'] == 'list'), int((int(io[4]) | int(io[5])) & 3 != 0), st['clipped'], st['ties']))
        par, cov = np.array(par, dtype=np.int32), np.array(cov, dtype=np.int32)
        n = len(par)
        share = {'list': (cov[:, 0] != 0).mean(), 'subpel': (cov[:, 1] != 0).mean(), 'clipped': (cov[:, 2] != 0).mean(), 'tie': (cov[:, 3] != 0).mean()}
        wide = int((((par[:, 2] == 16) & (par[:, 14] > 0)) | ((par[:, 2] == 16) & (par[:, 13] == 1) & (par[:, 12] == 1))).sum())
        print(f'bitdepth {bd}: {n} motion_estimate items; shares', {k: round(float(v), 3) for k, v in share.items()}, 'ties met:', int(cov[:, 3].sum()), 'widesad items:', wide,
              'speeds:', [int((par[:, 13] == s).sum()) for s in (0, 1, 2)], 'staged:', int(par[:, 16].sum()))
        assert all(v >= 0.05 for v in share.values()), share   # conditions on the fixture
        assert wide >= 100
        out[f'me{bd}_par'], out[f'me{bd}_lam'], out[f'me{bd}_cand'] = par, np.array(lams), np.array(cand, dtype=np.int16).reshape(-1, 2)
        out[f'me{bd}_out'], out[f'me{bd}_cov'] = np.array(res, dtype=np.int32), cov
        par, lams, cand, res, lists, clip2 = [], [], [], [], [], 0
        for q, lam, cl in bi_items(bd, rng):
            cbx, cby, cb = q[:3]
            org[:cb * cb] = cur[cby:cby + cb, cbx:cbx + cb].reshape(-1)
            io = np.array([q[7], q[8], q[9], q[10], 0, 0], dtype=np.int16)
            ca = np.array(cl, dtype=np.int16).reshape(6, 2).copy()
            o = (cby * PITCH + cbx) * S
            cost = mebi(org.ctypes.data, a0 + o, a1 + o, cb, PITCH, io.ctypes.data, lam, 0, bd, q[11], W, H, cbx, cby, ca.ctypes.data, q[14], q[12])
            c0 = (((q[7] + 2) >> 2) << 2, ((q[8] + 2) >> 2) << 2)
            m0 = clip_mv(c0[0], c0[1], cby, cbx, cb, q[11])
            clip2 += clip_mv(m0[0], m0[1], cby, cbx, cb, 1 - q[11]) != m0
            par.append(q); lams.append(lam); cand.append(cl); res.append((int(io[4]), int(io[5]), cost)); lists.append(ca)
        lists = np.array(lists, dtype=np.int16)
        assert not ((lists[:, :, 0] == SENTINEL[0]) & (lists[:, :, 1] == SENTINEL[1])).any()   # every slot the call did not own on entry was overwritten
        print(f'bitdepth {bd}: {len(par)} motion_estimate_bi items; second clip changes the centre in {clip2}')
        assert clip2 >= 0.05 * len(par)
        out[f'bi{bd}_par'], out[f'bi{bd}_lam'], out[f'bi{bd}_cand'] = np.array(par, dtype=np.int32), np.array(lams), np.array(cand, dtype=np.int16).reshape(-1, 2)
        out[f'bi{bd}_out'], out[f'bi{bd}_list'] = np.array(res, dtype=np.int32), lists
    p = os.path.join(ROOT, 'tests', 'golden', 'kat8.npz')
    np.savez_compressed(p, **out)
    print('kat8.npz:', os.path.getsize(p), 'bytes')


if __name__ == '__main__':
    main()
