"""64x64 superblocks, -log2_sb_size 6 (-m "not gpu"): the parameter doors accept 6 and 7 and nothing else, and the host simulation of the
engine sources (tests/hostsim) reproduces the reference encoder's streams, reconstructions and report on the finer superblock grid
(tests/golden/gen_streams_sb64.py -> streams_sb64.json, gen_reports_sb64.py -> reports_sb64.json).  Where oracle/_ref holds the
reference binaries, the live reference agrees with the recorded hashes and its decoder reproduces the reconstruction of the CDEF-off
cases (with CDEF on it mis-parses tiny frames at either superblock size: tests/test_reference_golden.py)."""
import ctypes as C
import json
import os
import subprocess
import tempfile
import pytest
from util import ROOT, GOLD, REF_ENC, REF_DEC, golden_clip, build_hostsim, run_encoder, decode, md5

G = json.load(open(os.path.join(GOLD, 'streams_sb64.json')))
REPORTS = json.load(open(os.path.join(GOLD, 'reports_sb64.json')))
CFG = os.path.join(ROOT, 'configs', 'ldb_high_efficiency.cfg')
# the cases of the issue's table; the '_skip' chunks belong to the multi-stream GPU test and get one host run each as well
SMALL = sorted(G)
FOUR_WAVES = [n for n in SMALL if n.startswith(('208x120', '200x184'))]
NOCDEF = [n for n in SMALL if 'nocdef' in n]
_RUNS = {}


def hostsim_run(name, waves=1):
    """(bits, recon) of the host simulation on a case of streams_sb64.json: one run per case and build, shared by the tests."""
    if (name, waves) not in _RUNS:
        c = G[name]
        _RUNS[(name, waves)] = run_encoder(build_hostsim(waves=waves), golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c['cfg'])
    return _RUNS[(name, waves)]


def _set(p, name, value):
    import thor_amd
    return thor_amd.lib().thor_hip_params_set(C.byref(p), name.encode(), str(value).encode())


def test_goldens_are_the_cases_they_claim_to_be():
    assert len(SMALL) == 13 and len(NOCDEF) == 2 and len(FOUR_WAVES) == 5
    big = json.load(open(os.path.join(GOLD, 'streams_big_sb64.json')))
    for c in list(G.values()) + list(big.values()):
        e = c['extra']
        assert e[e.index('-log2_sb_size') + 1] == '6' and len(c['frames']) == c['n']
    # the streams differ from the 128x128 ones of the same command
    g128 = json.load(open(os.path.join(GOLD, 'streams.json')))
    for name in ('208x120_n4_q32', '192x128_n6_q32', '128x96_n9_q32_ra', '192x128_n4_q32_10bit', '192x128_n6_q32_ldb_low', '208x120_n4_q30_ldb_medium'):
        assert G[name + '_sb64']['bit_md5'] != g128[name]['bit_md5']


def test_params_set_sb_size_accepts_6_and_7_and_both_setters_refuse_5_and_8():
    """thor_hip_params_set itself keeps refusing "-log2_sb_size 6" with code 2 (tests/test_params.py holds it to that), so 64x64 is chosen
    through thor_hip_params_set_sb_size, which load_config(log2_sb_size=...) and tools/thorenc_hip call for this option."""
    import thor_amd
    L = thor_amd.lib()
    p = thor_amd.load_config(CFG, width=208, height=120, qp=32, f=30)
    assert p.log2_sb_size == 7                                   # the reference's default (enc/strings.c:299)
    assert L.thor_hip_params_set_sb_size(C.byref(p), 6) == 0 and p.log2_sb_size == 6
    assert L.thor_hip_params_set_sb_size(C.byref(p), 7) == 0 and p.log2_sb_size == 7
    assert _set(p, '-log2_sb_size', 7) == 0 and p.log2_sb_size == 7
    L.thor_hip_params_set_sb_size(C.byref(p), 6)
    for bad in (5, 8):
        assert _set(p, '-log2_sb_size', bad) == 2 and p.log2_sb_size == 6, bad           # known option, value not implemented
        assert L.thor_hip_params_set_sb_size(C.byref(p), bad) == 2 and p.log2_sb_size == 6, bad
    assert thor_amd.load_config(CFG, width=208, height=120, log2_sb_size=6).log2_sb_size == 6
    with pytest.raises(ValueError):
        thor_amd.load_config(CFG, log2_sb_size=8)


def test_params_from_config_round_trip(tmp_path):
    import thor_amd
    ok = tmp_path / 'sb64.cfg'
    ok.write_text('-max_num_ref 2\n-log2_sb_size 6 ; 64x64 superblocks\n')
    p = thor_amd.load_config(str(ok))
    assert (p.max_num_ref, p.log2_sb_size) == (2, 6)
    for bad in (5, 8):
        f = tmp_path / ('sb%d.cfg' % bad)
        f.write_text('-log2_sb_size %d\n' % bad)
        q = thor_amd.binding.ThorParams()
        assert thor_amd.lib().thor_hip_params_from_config(C.byref(q), str(f).encode()) == 2


def test_existing_field_offsets_hold():
    """The new field is the last one of thor_hip_params: every earlier field keeps its offset."""
    import thor_amd
    T = thor_amd.binding.ThorParams
    names = [f[0] for f in T._fields_]
    assert names[-1] == 'log2_sb_size' and names[-2] == 'max_clpf_strength'
    assert [getattr(T, n).offset for n in names] == [4 * i for i in range(len(names))] and C.sizeof(T) == 4 * len(names)


def test_open_refuses_5_and_8_before_it_touches_the_device():
    """thor_hip_open validates the parameters before it initialises HIP: NULL comes back on a machine without a GPU too, where any
    later step would have ended the process (the library has no CPU path)."""
    import thor_amd
    for bad in (5, 8):
        p = thor_amd.load_config(CFG, width=208, height=120, qp=32, f=30)
        p.log2_sb_size = bad
        assert not thor_amd.lib().thor_hip_open(C.byref(p), 1, 0), bad


@pytest.mark.parametrize('binary', ['hostsim', 'thorenc_hip'])
def test_command_line_exits_2_for_5_and_8(binary):
    exe = build_hostsim() if binary == 'hostsim' else os.path.join(ROOT, 'tools', 'thorenc_hip')
    for bad in ('5', '8'):
        r = subprocess.run([exe, '-cf', CFG, '-if', os.devnull, '-width', '208', '-height', '120', '-qp', '32', '-n', '1', '-log2_sb_size', bad],
                           capture_output=True, text=True)
        assert r.returncode == 2 and 'log2_sb_size' in r.stderr, (bad, r.returncode, r.stderr)


@pytest.mark.parametrize('name', SMALL)
def test_host_simulation_matches_reference_golden(name):
    bits, rec = hostsim_run(name)
    c = G[name]
    assert len(bits) == c['bit_bytes']
    assert md5(bits) == c['bit_md5'], 'bitstream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@pytest.mark.parametrize('name', FOUR_WAVES)
def test_four_wave_host_simulation_matches_reference_golden(name):
    """Four wavefronts per workgroup (OS threads): the fork/join block decision with 64x64 roots."""
    bits, rec = hostsim_run(name, waves=4)
    c = G[name]
    assert md5(bits) == c['bit_md5'] and md5(rec) == c['rec_md5']


def test_host_simulation_prints_the_reference_report():
    name = '208x120_n4_q32_sb64'
    c = G[name]
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(golden_clip(c['clip']))
        cmd = [build_hostsim(), '-cf', os.path.join(ROOT, 'configs', c['cfg']), '-if', os.path.join(d, 'in.yuv'), '-width', str(c['w']), '-height', str(c['h']),
               '-qp', str(c['qp']), '-n', str(c['n']), '-f', '30', '-of', os.path.join(d, 'o.bit'), '-rf', os.path.join(d, 'o.yuv')] + c['extra']
        out = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    rep = REPORTS[name]['report']
    assert out == rep
    assert [l.split()[:4] for l in rep.splitlines()[1:1 + c['n']]] == c['frames']


@pytest.mark.skipif(not os.path.exists(REF_ENC), reason='oracle/_ref/Thorenc not built')
@pytest.mark.parametrize('name', SMALL)
def test_live_reference_agrees_with_recorded_hashes(name):
    c = G[name]
    bits, rec = run_encoder(REF_ENC, golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c['cfg'])
    assert md5(bits) == c['bit_md5'] and md5(rec) == c['rec_md5'] and len(bits) == c['bit_bytes']


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason='oracle/_ref/Thordec not built')
@pytest.mark.parametrize('name', NOCDEF)
def test_reference_decoder_reproduces_the_reconstruction(name):
    bits, rec = hostsim_run(name)
    assert decode(bits) == rec
