#!/usr/bin/env python3
"""Records tests/golden/tf_streams.json: stream / reconstruction hashes of the host simulation coding, WITHOUT the -tf_ options, the clip that the numpy model
(tests/tf_model.py) filtered.  The front ends with -tf_strength on the unfiltered clip must reproduce them: the host simulation in tests/test_tf.py, the device
in tests/test_gpu_tf.py.  Run after build(); only this recorded output is committed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import key_model as km
import tf_model as tm
from util import build_hostsim, golden_clip, md5

CASES = {
    'ldb_8bit': dict(clip='gen:64,64,8,21,6.0', w=64, h=64, n=8, qp=32, depth=8, cfg='ldb_high_efficiency.cfg', extra=[], strength=6, past=2, future=2),
    'ra_10bit': dict(clip='gen:64,64,9,23,6.0,10', w=64, h=64, n=9, qp=32, depth=10, cfg='ra_high_efficiency.cfg', extra=['-bitdepth', '10', '-input_bitdepth', '10'],
                     strength=6, past=2, future=2),
}

if __name__ == '__main__':
    out = {}
    for name, c in CASES.items():
        frames = tm.split_frames(golden_clip(c['clip']), c['w'], c['h'], c['n'], c['depth'])
        clip = tm.join_frames(tm.filter_clip(frames, c['depth'], c['strength'], c['past'], c['future']))
        r = km.run(build_hostsim(), clip, c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c['cfg'])
        out[name] = dict(c, bit_md5=md5(r['bits'][0]), bit_bytes=len(r['bits'][0]), rec_md5=md5(r['rec'][0]))
        print(name, out[name]['bit_bytes'], 'bytes')
    json.dump(out, open(os.path.join(HERE, 'tf_streams.json'), 'w'), indent=1)
