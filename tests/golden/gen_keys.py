#!/usr/bin/env python3
"""Records tests/golden/key_streams.json.
  ref    stream / reconstruction hashes of the reference encoder (oracle/_ref/Thorenc) with -intra_period: low-delay streams with I frames after frame 0, which
         -key_frames must reproduce byte for byte
  ratios sum_best / sum_intra (per cent, rounded down) of the cut clip of tests/key_model.py with the numpy model, and the assertion that they separate
  host   hashes and key-frame logs of the host simulation on the -key_ cases; the GPU tests compare the device against them
Run after build(); only this recorded output is committed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import key_model as km
import rc_model as rm
from util import REF_ENC, build_hostsim, golden_clip, md5

HBD = ['-bitdepth', '10', '-input_bitdepth', '10']
REF = {
    'period4': dict(clip='clip_192x128_6.yuv.gz', w=192, h=128, n=6, qp=32, extra=['-intra_period', '4'], keys='0,4'),
    'period3': dict(clip='clip_192x128_6.yuv.gz', w=192, h=128, n=6, qp=32, extra=['-intra_period', '3'], keys='3'),
    'period2_10bit': dict(clip='clip10_192x128_5.yuv.gz', w=192, h=128, n=5, qp=32, extra=['-intra_period', '2'] + HBD, keys='2,4', keys_extra=HBD),
}
HOST = {
    'key2_nocdef': dict(clip='clip_192x128_6.yuv.gz', w=192, h=128, n=6, qp=32, extra=['-cdef', '0', '-key_frames', '2']),
    'cut': dict(clip='cut', w=km.CUT_W, h=km.CUT_H, n=8, qp=32, extra=['-key_scenecut', str(km.PERCENT)]),
    'cut_rc': dict(clip='cut', w=km.CUT_W, h=km.CUT_H, n=8, qp=32, extra=['-key_scenecut', str(km.PERCENT), '-rc_bitrate', '60000']),
    'plain_cut_clip': dict(clip='cut', w=km.CUT_W, h=km.CUT_H, n=8, qp=32, extra=[]),
    'key5_cut_clip': dict(clip='cut', w=km.CUT_W, h=km.CUT_H, n=8, qp=32, extra=['-key_frames', '5']),
}


def clip_bytes(name):
    return km.cut_clip()[1] if name == 'cut' else golden_clip(name)


def cut_ratios():
    """Per frame of the cut clip (frame 0 has no predecessor): floor(100 * sum_best / sum_intra)."""
    y = [f[0] for f in km.cut_clip()[0]]
    out = []
    for n in range(1, len(y)):
        s = rm.analyse_luma(y[n], y[n - 1])[0]
        out.append(int(s[1]) * 100 // int(s[0]))
    return out


if __name__ == '__main__':
    out = {'ref': {}, 'host': {}}
    for name, c in REF.items():
        r = km.run(REF_ENC, clip_bytes(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'])
        out['ref'][name] = dict(c, bit_md5=md5(r['bits'][0]), bit_bytes=len(r['bits'][0]), rec_md5=md5(r['rec'][0]))
    ratios = cut_ratios()
    cut, within = ratios[km.CUT_AT - 1], ratios[:km.CUT_AT - 1] + ratios[km.CUT_AT:]
    assert max(within) + 10 <= km.PERCENT and cut >= km.PERCENT + 5, (ratios, km.PERCENT)
    out['ratios'] = dict(percent=km.PERCENT, cut_at=km.CUT_AT, per_frame_from_1=ratios)
    for name, c in HOST.items():
        r = km.run(build_hostsim(), clip_bytes(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'])
        out['host'][name] = dict(c, bit_md5=md5(r['bits'][0]), rec_md5=md5(r['rec'][0]), key_log=r['key_log'].splitlines(), rc_log=r['rc_log'].splitlines())
    json.dump(out, open(os.path.join(HERE, 'key_streams.json'), 'w'), indent=1)
    print('ratios', ratios)
