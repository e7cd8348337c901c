"""Key frames restated (include/thor_hip.h: thor_hip_scene_cut): the scene-cut rule in plain Python integers on the sums of rc_model.analyse_luma, the schedule
of frame types it yields for a low-delay stream, the cut clip of the tests and one run of a Thorenc-compatible front end with the -key_ options."""
import os
import subprocess
import tempfile

import numpy as np

import rc_model as rm
from util import ROOT

KEY_SCHEDULE, KEY_FORCED, KEY_SCENE_CUT = 0, 1, 2
MAX_REQUESTS = 64   # pending requests per stream (include/thor_hip.h)

# The cut clip: frames 0 .. 3 of make_clip(seed 7) followed by frames 0 .. 3 of make_clip(seed 11), 96 x 64, sigma 3.  With the numpy model the ratio
# sum_best / sum_intra is 93 % at the cut and 47 .. 75 % inside either scene (tests/golden/key_streams.json holds them; gen_keys.py asserts the margins):
# PERCENT lies at least 10 points above every frame inside a scene and at least 5 below the cut.
CUT_W, CUT_H, CUT_SEEDS, CUT_AT, CUT_SIGMA = 96, 64, (7, 11), 4, 3.0
PERCENT = 85


def cut_clip():
    """The eight frames of the cut clip as 4:2:0 planes, and as the bytes of a .yuv file."""
    from thor_amd import synth
    fr = [f for seed in CUT_SEEDS for f in synth.make_clip(CUT_W, CUT_H, CUT_AT, seed, CUT_SIGMA)]
    return fr, b''.join(p.tobytes() for f in fr for p in f)


def is_cut(percent, min_interval, had_prev, frame_num, last_intra, sum_intra, sum_best):
    """The rule: a P frame with these figures is promoted."""
    if percent <= 0 or not had_prev:
        return False
    if frame_num - last_intra < max(1, min_interval):
        return False
    return sum_intra > 0 and sum_best * 100 >= percent * sum_intra


def schedule(lumas, percent=0, min_interval=0, forced=(), intra_period=0):
    """Frame types (0 I, 1 P), reasons and analysis sums of a low-delay stream over the luma planes `lumas`: [(type, reason, [sum_intra, sum_best, n_intra])].
    The sums are zero when scene cuts are off (the frame is not analysed)."""
    out, last_intra = [], 0
    for n, y in enumerate(lumas):
        own = (n % intra_period == 0) if intra_period > 0 else n == 0
        ftype, reason = (0, KEY_SCHEDULE) if own else (0, KEY_FORCED) if n in forced else (1, KEY_SCHEDULE)
        sums = [0, 0, 0]
        if percent > 0:
            sums = [int(v) for v in rm.analyse_luma(y, lumas[n - 1] if n else None)[0]]
            if ftype == 1 and is_cut(percent, min_interval, n > 0, n, last_intra, sums[0], sums[1]):
                ftype, reason = 0, KEY_SCENE_CUT
        if ftype == 0:
            last_intra = n
        out.append((ftype, reason, sums))
    return out


def parse_log(text):
    """The key-frame log a front end writes (THOR_KEY_LOG): one row per coded frame."""
    keys = ('stream', 'display', 'frame_type', 'reason', 'sum_intra', 'sum_best', 'n_intra')
    return [dict(zip(keys, map(int, line.split()))) for line in text.splitlines() if line.strip()]


def run(binary, clip_bytes, w, h, n, qp=32, extra=(), env=None, streams=1, cfg='ldb_high_efficiency.cfg', check=True):
    """One run of a Thorenc-compatible front end: dict(bits=[...], rec=[...], report, key_log, rc_log, returncode, stderr)."""
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(clip_bytes)
        e = dict(os.environ, THOR_KEY_LOG=os.path.join(d, 'key.log'), THOR_RC_LOG=os.path.join(d, 'rc.log'), **(env or {}))
        cmd = [binary, '-cf', os.path.join(ROOT, 'configs', cfg), '-if', os.path.join(d, 'in.yuv'), '-width', str(w), '-height', str(h), '-qp', str(qp),
               '-n', str(n), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + (['-streams', str(streams)] if streams > 1 else []) + list(extra)
        r = subprocess.run(cmd, check=check, capture_output=True, text=True, env=e)
        names = [''] if streams == 1 else ['.%d' % s for s in range(streams)]

        def rd(name, mode='rb'):
            p = os.path.join(d, name)
            return open(p, mode).read() if os.path.exists(p) else ('' if mode == 'r' else b'')
        return dict(bits=[rd('o.bit' + s) for s in names], rec=[rd('o.yuv' + s) for s in names], report=r.stdout, key_log=rd('key.log', 'r'), rc_log=rd('rc.log', 'r'),
                    returncode=r.returncode, stderr=r.stderr)


def luma_planes(clip_bytes, w, h, n, dtype=np.uint8):
    a = np.frombuffer(clip_bytes, dtype=dtype)
    fsz = w * h * 3 // 2
    return [a[i * fsz:i * fsz + w * h].reshape(h, w) for i in range(n)]
