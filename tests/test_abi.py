"""The C-ABI library loads and exports every function include/thor_hip.h declares (no compute calls:
this runs without a GPU), and thor_abi.h matches the reference structure layouts."""
import ctypes as C
import os
import re
from util import ROOT


def declared_functions():
    h = open(os.path.join(ROOT, 'include', 'thor_hip.h')).read()
    h = re.sub(r'/\*.*?\*/', '', h, flags=re.S)
    return sorted(set(re.findall(r'\b(thor_hip_\w+|encode_frame_\w+)\s*\(', h)))


def test_library_exports_every_declared_symbol():
    import thor_amd
    lib = thor_amd.lib()
    names = declared_functions()
    assert 'encode_frame_lbd' in names and 'thor_hip_encode_staged' in names and len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/thor_hip.h but not exported'


def test_params_from_config_matches_config_file():
    import thor_amd
    p = thor_amd.load_config(os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg'), width=1920, height=1080, qp=32)
    assert (p.max_num_ref, p.HQperiod, p.enable_bipred, p.enable_tb_split, p.enable_pb_split, p.intra_rdo) == (4, 12, 1, 1, 1, 1)
    assert abs(p.mqpP - 1.2) < 1e-6 and p.dqpI == -2 and p.cdef == 2 and p.encoder_speed == 0


def test_abi_layout_matches_reference_headers():
    """Every sizeof and every named member offset of thor_abi.h equals the reference's, as tests/golden/gen_abi.py recorded it from the
    reference headers."""
    import json
    from golden.gen_abi import measure
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'abi_layout.json')))
    got = measure('thor_abi.h', [os.path.join(ROOT, 'include')], 2)
    assert got == want, {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
