#!/usr/bin/env python3
"""Golden layout of the reference structures include/thor_abi.h restates: sizeof and the offsets of the members this path uses, measured by
a probe compiled against the reference headers -> tests/golden/abi_layout.json (tests/test_abi.py compares thor_abi.h with it).  Build
container only (needs the reference tree).
  python tests/golden/gen_abi.py REFERENCE_DIR"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = [('yuv_frame_t', 'thor_yuv_frame'), ('stream_t', 'thor_stream'), ('enc_params', 'thor_enc_params'), ('frame_info_t', 'thor_frame_info'),
         ('encoder_info_t', 'thor_encoder_info'), ('stream_pos_t', 'thor_stream_pos'), ('deblock_data_t', 'thor_deblock_data'), ('inter_pred_t', 'thor_inter_pred')]
MEMBERS = [('yuv_frame_t', 'stride_c'), ('yuv_frame_t', 'frame_num'), ('yuv_frame_t', 'pad_ver_c'),
           ('enc_params', 'early_skip_thr'), ('enc_params', 'mqpP'), ('enc_params', 'cdef'), ('enc_params', 'enable_bipred'), ('enc_params', 'cfl_inter'),
           ('enc_params', 'input_bitdepth'),
           ('frame_info_t', 'qp'), ('frame_info_t', 'ref_array'), ('frame_info_t', 'lambda'), ('frame_info_t', 'num_intra_modes'), ('frame_info_t', 'frame_num'),
           ('frame_info_t', 'prev_qp'),
           ('encoder_info_t', 'params'), ('encoder_info_t', 'orig'), ('encoder_info_t', 'ref'), ('encoder_info_t', 'stream'), ('encoder_info_t', 'width'),
           ('encoder_info_t', 'cdef_bits'), ('encoder_info_t', 'deblock_data'),
           ('deblock_data_t', 'mode'), ('deblock_data_t', 'size'), ('deblock_data_t', 'tb_split'), ('deblock_data_t', 'pb_part'), ('deblock_data_t', 'inter_pred'),
           ('deblock_data_t', 'inter_pred_arr'), ('inter_pred_t', 'ref_idx0'), ('inter_pred_t', 'bipred_flag')]
THOR = dict(PAIRS)
# key -> (C expression on the reference structures, the same quantity on the thor_abi.h structures); deblock_data_t.cbp (a cbp_t of y / u / v)
# is restated as the members cbp_y / cbp_u / cbp_v
CHECKS = ([(f'sizeof {r}', f'sizeof({r})', f'sizeof({t})') for r, t in PAIRS] +
          [(f'offset {r}.{m}', f'offsetof({r}, {m})', f'offsetof({THOR[r]}, {m})') for r, m in MEMBERS] +
          [('offset deblock_data_t.cbp', 'offsetof(deblock_data_t, cbp)', 'offsetof(thor_deblock_data, cbp_y)'),
           ('offset deblock_data_t.cbp.v', 'offsetof(deblock_data_t, cbp) + offsetof(cbp_t, v)', 'offsetof(thor_deblock_data, cbp_v)')])


def measure(header, include_dirs, side):
    """{key: value} of the CHECKS expressions of `side` (1: reference, 2: thor_abi.h), compiled with gcc after #include `header`."""
    lines = ''.join(f'  printf("%s %%zu\\n", (size_t)({c[side]}));\n' % c[0] for c in CHECKS)
    probe = f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void) {{\n{lines}  return 0; }}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'p.c'), 'w').write(probe)
        subprocess.check_call(['gcc', '-fcommon', '-std=c99'] + [x for i in include_dirs for x in ('-I', i)] + ['-o', os.path.join(d, 'p'), os.path.join(d, 'p.c')])
        out = subprocess.run([os.path.join(d, 'p')], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (l.rsplit(' ', 1) for l in out.splitlines())}


def measure_reference(ref):
    return measure('mainenc.h', [os.path.join(ref, 'common'), os.path.join(ref, 'enc')], 1)


if __name__ == '__main__':
    json.dump(measure_reference(sys.argv[1]), open(os.path.join(HERE, 'abi_layout.json'), 'w'), indent=1)
