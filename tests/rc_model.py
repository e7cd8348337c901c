"""Rate control restated (include/thor_hip.h: thor_hip_rate_control): the frame analysis in numpy and the controller in plain Python integers.
Nothing here is shared with thor_amd/csrc/tk_rc.h but the constants, which the header states."""
import numpy as np

RANGE = 8
STEP_Q16 = [round(65536 * 2 ** ((q - 4) / 6)) for q in range(52)]
INIT_FACTOR_Q16 = [296000, 217000, 216000, 188000, 174000, 174000]
QR_BASE, QR_I, QR_P, QR_B0, QR_B1, QR_B2, QR_B3, QR_B = range(8)


def half_plane(y):
    """(a + b + c + d + 2) >> 2 over the 2x2 quads of a luma plane."""
    y = y.astype(np.int64)
    return (y[0::2, 0::2] + y[0::2, 1::2] + y[1::2, 0::2] + y[1::2, 1::2] + 2) >> 2


def analyse(cur_half, prev_half=None):
    """sum_intra, sum_best, n_intra of a half-size plane against the previous one (None: inter = intra)."""
    h = cur_half.astype(np.int64)
    hh, hw = h.shape
    sums = [0, 0, 0]
    for y0 in range(0, hh, 8):
        for x0 in range(0, hw, 8):
            b = h[y0:y0 + 8, x0:x0 + 8]
            bh, bw = b.shape
            n = bw * bh
            intra = int(np.abs(b - (int(b.sum()) + n // 2) // n).sum())
            inter = intra
            if prev_half is not None:
                p = prev_half.astype(np.int64)
                inter = None
                for dy in range(-RANGE, RANGE + 1):
                    for dx in range(-RANGE, RANGE + 1):
                        if x0 + dx < 0 or x0 + dx + bw > hw or y0 + dy < 0 or y0 + dy + bh > hh:
                            continue
                        s = int(np.abs(b - p[y0 + dy:y0 + dy + bh, x0 + dx:x0 + dx + bw]).sum())
                        inter = s if inter is None or s < inter else inter
            sums[0] += intra
            sums[1] += min(intra, inter)
            sums[2] += intra < inter
    return sums


def analyse_luma(cur, prev=None):
    """The analysis of two consecutive luma planes: (sums, half-size plane of cur)."""
    h = half_plane(cur)
    return analyse(h, None if prev is None else half_plane(prev)), h


def rule_qp(p, rule, base):
    """The reference's per-frame QP from a base QP; p: the parameter set (mqp* as float32, dqp* as int)."""
    f32 = np.float32
    if rule == QR_I:
        q = base + p['dqpI']
    elif rule == QR_BASE:
        q = base
    else:
        k = {QR_P: 'P', QR_B0: 'B0', QR_B1: 'B1', QR_B2: 'B2', QR_B3: 'B3', QR_B: 'B'}[rule]
        q = int(f32(p['mqp' + k]) * f32(base)) + p['dqp' + k]
    return min(max(q, 0), 51)


def frame_class(frame_type, b_level):
    return 0 if frame_type == 0 else 1 if frame_type == 1 else 2 + min(b_level, 3)


def clamp_cost(cost):
    return min(max(cost, 1), 1 << 36)


def tdiv(a, b):
    return a // b if a >= 0 else -((-a) // b)


class Controller:
    def __init__(self, bitrate, frame_rate, buffer_ms=0, min_qp=0, max_qp=0, min_qp_i=0, max_qp_i=0, initial_qp=0, seq_qp=32):
        if min_qp == 0 and max_qp == 0:
            max_qp = 51
        if min_qp_i == 0 and max_qp_i == 0:
            max_qp_i = 51
        self.lim = (min_qp, max_qp, min_qp_i, max_qp_i)
        self.initial_qp = initial_qp or seq_qp
        self.T = max(1, int(float(bitrate) / float(np.float32(frame_rate))))
        self.B = max(1, bitrate * (buffer_ms or 1000) // 1000)
        self.F = 0
        self.overflows = 0
        self.frames = 0
        self.factor = [0] * 6
        self.avg = [0] * 6
        self.n = [0] * 6

    def budget(self, c):
        b = self.T
        if c == 0:
            b = self.T * 4
        elif self.n[c] > 0:
            mean = max(1, sum(self.n[k] * self.avg[k] for k in range(1, 6)) // sum(self.n[1:]))
            b = self.T * self.avg[c] // mean
        b -= tdiv(self.F, max(1, self.B // (2 * self.T)))
        return max(b, self.T // 8)

    def decide(self, c, cost, qp_of_base):
        """qp_of_base(b): the frame's QP at base QP b."""
        if self.frames == 0:
            return self.initial_qp
        lo, hi = self.lim[2:] if c == 0 else self.lim[:2]
        budget = self.budget(c)
        f = self.factor[c] if self.n[c] > 0 else INIT_FACTOR_Q16[c]
        for b in range(lo, hi):
            if f * clamp_cost(cost) // STEP_Q16[qp_of_base(b)] <= budget:
                return b
        return hi

    def update(self, c, cost, qp, bits):
        o = min(max(bits * STEP_Q16[qp] // clamp_cost(cost), 1), 1 << 26)
        self.factor[c] = (self.factor[c] + o) // 2 if self.n[c] > 0 else o
        self.avg[c] = (3 * self.avg[c] + bits) // 4 if self.n[c] > 0 else bits
        self.n[c] += 1
        if sum(self.n) >= 65536:
            self.n = [(k + 1) // 2 for k in self.n]
        self.F = max(self.F + bits - self.T, -self.B)
        self.overflows += self.F > self.B
        self.frames += 1


def parse_log(text):
    """The controller's log the host simulation writes (THOR_RC_LOG): one row per coded frame."""
    keys = ('stream', 'display', 'frame_type', 'frame_class', 'qp_rule', 'base_qp', 'qp', 'bits', 'sum_intra', 'sum_best', 'n_intra', 'fullness', 'overflows')
    return [dict(zip(keys, map(int, line.split()))) for line in text.splitlines() if line.strip()]


def replay(rows, params, **rc):
    """Feed the controller the analysis sums and bit counts of one stream's log; returns the (base_qp, qp, fullness, overflows) it yields per frame."""
    ctl = Controller(seq_qp=params['qp'], frame_rate=params['frame_rate'], **rc)
    out = []
    for r in rows:
        cost = r['sum_intra'] if r['frame_class'] == 0 else r['sum_best']
        base = ctl.decide(r['frame_class'], cost, lambda b: rule_qp(params, r['qp_rule'], b))
        qp = rule_qp(params, r['qp_rule'], base)
        ctl.update(r['frame_class'], cost, qp, r['bits'])
        out.append((base, qp, ctl.F, ctl.overflows))
    return out, ctl


def read_params(cfg_path, qp, frame_rate=30.0):
    """The QP hierarchy of a config file: the dqp* / mqp* options, with the reference's defaults."""
    p = {'qp': qp, 'frame_rate': frame_rate, 'dqpI': 0}
    for k in ('P', 'B', 'B0', 'B1', 'B2', 'B3'):
        p['dqp' + k], p['mqp' + k] = 0, 1.0
    for line in open(cfg_path):
        t = line.split(';')[0].split()
        if len(t) >= 2 and t[0][1:] in p:
            p[t[0][1:]] = float(t[1]) if t[0].startswith('-mqp') else int(t[1])
    return p


# Contents of the known-answer cases, by name: (cur, prev or None) luma planes of h x w samples at `depth`.
KAT_SHAPES = [(16, 16), (24, 40), (136, 72)]
KAT_CONTENTS = ['random', 'max', 'no_prev', 'identical', 'shift_8_m8', 'shift_9', 'max_stripes']


def kat_case(w, h, depth, content, seed=1):
    rng = np.random.default_rng(seed + 1000 * depth + w)
    maxv = (1 << depth) - 1
    T = np.uint8 if depth == 8 else np.uint16
    big = rng.integers(0, maxv + 1, size=(h + 64, w + 64)).astype(T)
    cur = big[32:32 + h, 32:32 + w].copy()
    if content == 'random':
        return cur, rng.integers(0, maxv + 1, size=(h, w)).astype(T)
    if content == 'max':
        return np.full((h, w), maxv, T), np.zeros((h, w), T)
    if content == 'max_stripes':
        # half-size columns alternate 0 and the maximum; the previous frame has the same stripes with a lower high value: at depth 12 a block's intra cost is
        # 131040 and its least inter cost (the zero vector) 32 * 2559 = 81888 - both beyond 16 bits, and truncated to 16 they compare the other way round
        col = (np.arange(w) // 2) % 2
        cur = np.broadcast_to(col * maxv, (h, w)).astype(T)
        return cur, np.broadcast_to(col * (maxv - (maxv * 5) // 8), (h, w)).astype(T)
    if content == 'no_prev':
        return cur, None
    if content == 'identical':
        return cur, cur.copy()
    # the previous frame holds the current content displaced by (dx, dy) HALF-size samples: prev(x + dx, y + dy) = cur(x, y)
    dx, dy = (8, -8) if content == 'shift_8_m8' else (9, 0)
    return cur, big[32 - 2 * dy:32 - 2 * dy + h, 32 - 2 * dx:32 - 2 * dx + w].copy()
