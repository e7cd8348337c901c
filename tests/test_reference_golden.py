"""Pins the frame-level oracle: the reference encoder built by oracle/Makefile reproduces the committed
golden stream/recon hashes, decodes to its own reconstruction, and the 1-lane host simulation of the
engine sources (tests/hostsim) produces the identical stream and reconstruction."""
import os
import pytest
from util import (REF_ENC, REF_DEC, golden_streams, golden_clip, run_encoder, decode, md5, build_hostsim)

G = golden_streams()
needs_ref = pytest.mark.skipif(not os.path.exists(REF_ENC), reason='oracle/_ref not built (make -C oracle)')


@needs_ref
@pytest.mark.parametrize('name', sorted(G))
def test_reference_reproduces_golden_and_roundtrips(name):
    c = G[name]
    bits, rec = run_encoder(REF_ENC, golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c.get('cfg'))
    assert md5(bits) == c['bit_md5'] and md5(rec) == c['rec_md5']
    # the reference's own check.sh property (check.sh:54-75).  NB: with CDEF on, the reference encoder
    # can shrink cdef_bits when it back-patches the frame header (encode_frame.c:776-782) without moving
    # the payload, which its own decoder then mis-parses on tiny frames; the property is therefore only
    # asserted for the CDEF-off case here (and at 1080p in the GPU tests).
    if '-cdef' in c['extra']:
        assert decode(bits) == rec


@pytest.mark.parametrize('name', ['192x128_n3_q32', '208x120_n4_q32', '192x128_n3_q32_skip3', '192x128_n4_q44', '192x128_n4_q32_10bit',
                                  '128x96_n9_q32_ra', '192x128_n6_q30_ra_gop4', '192x128_n6_q36_ra_gop4_nointerp',
                                  '192x128_n5_q32_hdb16_gop4_10bit',
                                  '192x128_n6_q32_ldb_low', '208x120_n4_q30_ldb_medium', '208x120_n4_q38_ldb_medium_clpf',
                                  '192x128_n5_q34_ldb_low_10bit', 'cfg1_352x288_n30_q32_ldb_low',
                                  '192x128_n4_q32_12bit', '192x128_n5_q30_hdb16_gop4_12bit', '208x120_n4_q36_ldb_medium_clpf_12bit'])   # (the 26 / 27-frame LDB goldens: 4-wave simulation below and the GPU suite)
def test_engine_host_simulation_matches_golden(name):
    c = G[name]
    bits, rec = run_encoder(build_hostsim(), golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c.get('cfg'))
    assert md5(bits) == c['bit_md5'], 'stream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@pytest.mark.parametrize('name', ['192x128_n3_q32', '192x128_n6_q32_ldb_low', '208x120_n4_q30_ldb_medium'])
def test_engine_multi_lane_host_simulation_matches_golden(name):
    """The same engine sources with 8-lane teams (one OS thread per lane; ballots, shuffles, reductions and barriers go
    through a publish/read exchange, tests/hostsim/hostsim.cpp): exercises the lane-parallel logic - work distribution,
    reductions, ballot automata, uniformity assumptions (tk_uniform aborts if lanes disagree) - without a GPU."""
    c = G[name]
    bits, rec = run_encoder(build_hostsim(lanes=8), golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c.get('cfg'))
    assert md5(bits) == c['bit_md5'], 'stream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@pytest.mark.parametrize('name', ['192x128_n6_q32', '208x120_n4_q32', '128x96_n9_q32_ra', '192x128_n6_q30_ra_gop4', '192x128_n4_q32_10bit',
                                  '192x128_n5_q32_hdb16_gop4_10bit', '208x120_n4_q30_ldb_medium', '208x120_n26_q24_ldb', '192x128_n4_q32_12bit'])
def test_engine_multi_wave_host_simulation_matches_golden(name):
    """Workgroups of 4 wavefronts (one OS thread each): the block decision of the encoder_speed 0 operating points is
    spread over the waves through a work queue (tk_block_queue.h:mode_decision_par) - fork/join barriers, atomics on the shared
    state and key-based pruning run under real concurrency; the result must not depend on the interleaving."""
    c = G[name]
    for _ in range(2):
        bits, rec = run_encoder(build_hostsim(waves=4), golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c.get('cfg'))
        assert md5(bits) == c['bit_md5'], 'stream differs from the reference'
        assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@pytest.mark.parametrize('name', ['192x128_n6_q32', '128x96_n9_q32_ra', '208x120_n4_q30_ldb_medium'])
def test_engine_eight_wave_host_simulation_matches_golden(name):
    """Workgroups of EIGHT wavefronts - the width of the third build of the 8-bit kernel (thor_hip_wide.cpp, what the library launches for runs of very few
    streams): the work queue drained by eight waves, the bi-prediction phase's rows split eight ways, eight per-wave minima at the join."""
    c = G[name]
    bits, rec = run_encoder(build_hostsim(waves=8), golden_clip(c['clip']), c['w'], c['h'], c['n'], c['qp'], c['extra'], cfg=c.get('cfg'))
    assert md5(bits) == c['bit_md5'], 'stream differs from the reference'
    assert md5(rec) == c['rec_md5'], 'reconstruction differs from the reference'


@needs_ref
def test_sixteen_lane_teams_search_window_and_row_segments_vs_live_reference():
    """16-lane teams on a 64x64 clip (I + 2 P): with 16 lanes the PUs up to 16x16 take the side-by-side row-segment path of the
    full-pel evaluator and the LDS search window (candidate sets per lane group, in-window test by ballot, window reads of the
    sub-pel search), larger PUs the whole-team path - the lane mappings the 8-lane test above does not reach."""
    from thor_amd import synth
    clip = b''.join(p.tobytes() for fr in synth.make_clip(64, 64, 3, 11, 4.0) for p in fr)
    rb, rr = run_encoder(REF_ENC, clip, 64, 64, 3, 32)
    bits, rec = run_encoder(build_hostsim(lanes=16), clip, 64, 64, 3, 32)
    assert bits == rb and rec == rr


@needs_ref
def test_sixty_four_lane_teams_run_the_lane_per_candidate_search_vs_live_reference():
    """64-lane teams (the device's team size) on a 64x64 clip (I + 2 P; the second P frame searches two references and their bi-prediction): with 64 lanes the 8-bit PUs of up to
    32x32 samples take the lane-per-candidate search (tk_me_lanes.h: me_cand_fullpel / me_cand8_subpel) - the code the MI355X runs - inside a complete
    encode, on the CPU; stream and reconstruction must equal the live reference run.  (A whole small golden, 192x128 x 3 frames, was run this way once
    in round 5: profiles/r05_hostsim_l64.log - 64 OS threads per team make it too slow for the suite.)"""
    from thor_amd import synth
    clip = b''.join(p.tobytes() for fr in synth.make_clip(64, 64, 3, 13, 4.0) for p in fr)
    rb, rr = run_encoder(REF_ENC, clip, 64, 64, 3, 32)
    bits, rec = run_encoder(build_hostsim(lanes=64), clip, 64, 64, 3, 32)
    assert bits == rb and rec == rr


@needs_ref
def test_sixty_four_lane_teams_16bit_lane_per_candidate_search_vs_live_reference():
    """Round 6: the same on 10-bit samples - 64-lane teams take me_cand_fullpel<uint16_t> (v_sad_u16 on 16-byte segments, SAD >> 2) for the full-pel passes of
    PUs up to 32x32 inside a complete encode (I + 2 P, 64x64); stream and reconstruction must equal the live reference run (_hbd path)."""
    from thor_amd import synth
    clip = b''.join(p.tobytes() for fr in synth.make_clip(64, 64, 3, 17, 4.0, 10) for p in fr)
    ex = ['-bitdepth', '10', '-input_bitdepth', '10']
    rb, rr = run_encoder(REF_ENC, clip, 64, 64, 3, 32, ex)
    bits, rec = run_encoder(build_hostsim(lanes=64), clip, 64, 64, 3, 32, ex)
    assert bits == rb and rec == rr


@needs_ref
def test_multi_wave_host_simulation_416x240_four_references_vs_live_reference():
    """416x240 LDB_high_efficiency, I + 5 P (the last two P frames search 4 references): the regime bench.py times - lock-step
    bi-prediction search over 4 references with skipped repeat steps, duplicate-partition skipping, key-based pruning - in the
    4-wave host simulation against a live run of the reference."""
    clip = golden_clip('gen:416,240,6,2,2.0')
    rb, rr = run_encoder(REF_ENC, clip, 416, 240, 6, 32)
    bits, rec = run_encoder(build_hostsim(waves=4), clip, 416, 240, 6, 32)
    assert bits == rb and rec == rr


def _large_pan_clip(w, h, n, seed):
    """Smoothed random texture panned by 13 / 17 samples per frame in alternating directions: the motion vectors near the frame
    borders point outside the padded area (clip_mv acts), telescope grids move every step."""
    import numpy as np
    from numpy.lib.stride_tricks import sliding_window_view
    rng = np.random.default_rng(seed)
    sm = sliding_window_view(rng.integers(0, 256, size=(h + 400, w + 400)).astype(np.float64), (5, 5)).mean(axis=(2, 3))
    out = b''
    for f in range(n):
        dy, dx = 200 + 13 * f * (1 if f % 2 else -1), 200 - 17 * f
        Y = sm[dy:dy + h, dx:dx + w] + rng.normal(0, 2.0, size=(h, w))
        U = sm[dy:dy + h:2, dx:dx + w:2] * 0.5 + 64 + rng.normal(0, 1.0, size=(h // 2, w // 2))
        V = sm[dy + 1:dy + h:2, dx + 1:dx + w:2] * 0.5 + 64
        out += b''.join(np.clip(np.rint(p), 0, 255).astype(np.uint8).tobytes() for p in (Y, U, V))
    return out


@needs_ref
def test_large_pan_clipped_vectors_and_moving_search_grids_vs_live_reference():
    """Fast alternating pan at 192x128 (I + 4 P): vectors get clipped at the frame borders and every telescope step moves its
    centre - the cases the "no vector is evaluated twice" rule of the motion search (tk_me.h: on_grid) has to get right: grids
    whose centre sits on the rim of the previous one, clipped candidates, hexagon starts off the last grid's centre.  1-lane and
    4-wave host simulation against a live run of the reference."""
    clip = _large_pan_clip(192, 128, 5, 77)
    rb, rr = run_encoder(REF_ENC, clip, 192, 128, 5, 30)
    for sim in (build_hostsim(), build_hostsim(waves=4)):
        bits, rec = run_encoder(sim, clip, 192, 128, 5, 30)
        assert bits == rb and rec == rr


@needs_ref
def test_host_simulation_two_random_access_streams_equal_reference_chunks():
    """Two closed RA streams (hierarchical B + interpolated references, host-threaded interpolation) in lock step ==
    the reference run on each chunk with -skip/-n."""
    import subprocess, tempfile
    from util import ROOT
    clip = golden_clip('gen:128,96,18,5,2.5')
    cfg = os.path.join(ROOT, 'configs', 'ra_high_efficiency.cfg')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(clip)
        base = ['-cf', cfg, '-if', os.path.join(d, 'in.yuv'), '-width', '128', '-height', '96', '-qp', '32', '-f', '30', '-n', '9']
        subprocess.run([build_hostsim()] + base + ['-streams', '2', '-of', os.path.join(d, 'm.bit'), '-rf', os.path.join(d, 'm.yuv')],
                       check=True, stdout=subprocess.DEVNULL)
        for s in range(2):
            subprocess.run([REF_ENC] + base + ['-skip', str(9 * s), '-of', os.path.join(d, 'r.bit'), '-rf', os.path.join(d, 'r.yuv')],
                           check=True, stdout=subprocess.DEVNULL)
            assert open(os.path.join(d, 'r.bit'), 'rb').read() == open(os.path.join(d, f'm.bit.{s}'), 'rb').read(), s
            assert open(os.path.join(d, 'r.yuv'), 'rb').read() == open(os.path.join(d, f'm.yuv.{s}'), 'rb').read(), s


@needs_ref
@pytest.mark.parametrize('cfg_name,w,h,n,streams', [('ldb_high_efficiency.cfg', 384, 136, 3, 3), ('ra_high_efficiency.cfg', 128, 96, 9, 2)])
def test_host_simulation_staggered_stream_groups_equal_reference_chunks(cfg_name, w, h, n, streams):
    """Engine::encode_run - the streams in two groups half a frame apart, every launch of the superblock scheduler covering the second half of
    one group's frame (a range of anti-diagonals of the superblock grid) and the first half of the other's - against the reference run on each
    chunk with -skip/-n: 384x136 LDB (3 x 2 superblocks: five anti-diagonals, three streams = groups of 1 and 2) with 1-lane teams and with
    4-wave workgroups, and an RA chunk pair (B frames, interpolated references prepared per group)."""
    import subprocess, tempfile
    from util import ROOT
    clip = golden_clip('gen:%d,%d,%d,6,2.5' % (w, h, n * streams))
    cfg = os.path.join(ROOT, 'configs', cfg_name)
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'in.yuv'), 'wb').write(clip)
        base = ['-cf', cfg, '-if', os.path.join(d, 'in.yuv'), '-width', str(w), '-height', str(h), '-qp', '32', '-f', '30', '-n', str(n)]
        for s in range(streams):
            subprocess.run([REF_ENC] + base + ['-skip', str(n * s), '-of', os.path.join(d, f'r.bit.{s}'), '-rf', os.path.join(d, f'r.yuv.{s}')],
                           check=True, stdout=subprocess.DEVNULL)
        for sim in ((build_hostsim(), build_hostsim(waves=4)) if 'ldb' in cfg_name else (build_hostsim(),)):
            subprocess.run([sim] + base + ['-streams', str(streams), '-of', os.path.join(d, 'm.bit'), '-rf', os.path.join(d, 'm.yuv')],
                           check=True, stdout=subprocess.DEVNULL, env=dict(os.environ, THOR_STAGGER='1'))
            for s in range(streams):
                assert open(os.path.join(d, f'r.bit.{s}'), 'rb').read() == open(os.path.join(d, f'm.bit.{s}'), 'rb').read(), (sim, s)
                assert open(os.path.join(d, f'r.yuv.{s}'), 'rb').read() == open(os.path.join(d, f'm.yuv.{s}'), 'rb').read(), (sim, s)
