"""Helpers shared by the known-answer tests of the block syntax (tests/golden/kat9.npz; tests/test_kat_host.py on the host build, tests/test_gpu_kat.py on the
device): the fixture's strings as bit arrays, the engine's 32-bit words (word w = bits [32w, 32w + 32), first bit in the MSB) as bit arrays, item rows."""
import os
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K9 = np.load(os.path.join(ROOT, 'tests', 'golden', 'kat9.npz'))
NP = 57
CO_WORDS = 260       # 2 words of start offset + 256 coefficients x 31 bits at most, + canaries
BL_WORDS = 640       # gen_kat9.py keeps every block string below 20 000 bits
FILL = 0xA5C396E1    # what the buffers hold before the call


def strings(pre):
    """List of bit arrays (uint8 0 / 1) of the fixture's strings `pre`_len / `pre`_str."""
    ln, raw = K9[pre + '_len'], K9[pre + '_str']
    off = np.concatenate([[0], np.cumsum((ln + 7) // 8)])
    return [np.unpackbits(raw[off[i]:off[i + 1]])[:ln[i]] for i in range(len(ln))]


def word_bits(words):
    """(n, W) uint32 -> (n, 32 W) bits, MSB of word 0 first."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(w.astype('>u4').view(np.uint8).reshape(len(w), -1), axis=1)


def vlc_rows():
    r = np.zeros((len(K9['vlc_par']), NP), dtype=np.int32)
    r[:, 0] = 2; r[:, 2:4] = K9['vlc_par']; r[:, 9] = 8
    return r


def mv_rows():
    r = np.zeros((len(K9['mv_par']), NP), dtype=np.int32)
    r[:, 0] = 3; r[:, 9] = 8; r[:, 29:31] = K9['mv_par'][:, 0:2]; r[:, 15:17] = K9['mv_par'][:, 2:4]
    return r


def all_rows():
    """Every item of the block entry: the fixture's blocks and super-modes, then every VLC codeword, then every vector difference; with their strings and the
    head lengths (-1: not a block)."""
    rows = np.concatenate([K9['bl_par'], vlc_rows(), mv_rows()])
    want = strings('bl') + strings('vlc') + strings('mv')
    head = np.concatenate([K9['bl_head'], np.full(len(rows) - len(K9['bl_head']), -1, dtype=np.int32)])
    return np.ascontiguousarray(rows), want, head


def check_emitted(name, bits, pos, ovf, want, start=None, fill_bits=None):
    """Every item: final position = start + length, no overflow, the bits [start, start + length) equal the reference string, and (fill_bits given) the bits
    before `start` are what the buffer held.  Returns a list of failure descriptions."""
    bad = []
    for i, w in enumerate(want):
        s = 0 if start is None else int(start[i])
        if int(pos[i]) != s + len(w) or int(ovf[i]) != 0: bad.append(f'{name} item {i}: pos {int(pos[i])} ovf {int(ovf[i])}, want pos {s + len(w)}')
        elif not np.array_equal(bits[i, s:s + len(w)], w): bad.append(f'{name} item {i}: string differs at bit {int(np.flatnonzero(bits[i, s:s + len(w)] != w)[0])} of {len(w)}')
        elif fill_bits is not None and not np.array_equal(bits[i, :s], fill_bits[:s]): bad.append(f'{name} item {i}: bits before the start offset {s} changed')
    return bad


def check_block_out(out, rows, want, head, lanes_only=False):
    """The counted variants of every item of the block entry against the reference length (and head length)."""
    bad = []
    for i, w in enumerate(want):
        n, o, q = len(w), out[i], rows[i]
        big = q[0] == 0 and q[25] and q[9] >= 64
        exp = {1: -1 if big else n, 3: -1 if big else n}
        if q[0] == 0: exp.update({0: int(head[i]), 2: n, 4: n})
        for k, v in exp.items():
            if int(o[k]) != v: bad.append(f'item {i} (kind {q[0]} mode {q[17]} size {q[9]} tb_split {q[25]}): out[{k}] = {int(o[k])}, want {v}')
    return bad


# ---- two engine-only properties (no reference comparison: the reference's putbits is undefined from 32 bits) -----------------------------------------------------
def vlc_code(n, cn):
    """(len, code) of put_vlc's tables 0..6 (enc/putvlc.c:85-125)."""
    if n == 6:
        if cn == 0: return 2, 2
        cn, n = cn + 1, 2
    t = 1 << n
    if cn < 5 * t: return 1 + n + (cn >> n), t + (cn & (t - 1))
    code = cn - 5 * t + t
    return (5 - n) + 1 + 2 * (code.bit_length() - 1), code


def code_bits(n, cn):
    ln, code = vlc_code(n, cn)
    k = code.bit_length()
    return [0] * (ln - k) + [int(b) for b in bin(code)[2:]]


def long_codeword_cases():
    """Luma inter 8x8 blocks whose only coefficient (scan position 0, or 1 after a zero) has a level of 4097 .. 32767: par, coef, expected strings, longest
    codeword.  Position 0: level code of table 0, sign, the extra zero (table 1 after a level > 3), EOB.  Position 1: zero level, run code, level code (level - 2) * 2 + sign, zero, EOB."""
    par, coef, want, longest = [], [], [], 0
    for lvl, sign, at in [(l, s, a) for l in (4097, 4098, 8195, 16387, 16388, 20000, 32767) for s in (0, 1) for a in (0, 1)]:
        c = np.zeros(256, dtype=np.int16)
        c[at] = -lvl if sign else lvl        # scan positions 0 and 1 of an 8x8 block are coefficients 0 and 1
        if at == 0: w = code_bits(0, lvl) + [sign] + code_bits(1, 0) + code_bits(6, 2)     # the zero after a level > 3 takes table 1
        else: w = code_bits(0, 0) + code_bits(6, 5) + code_bits(0, (lvl - 2) * 2 + sign) + code_bits(0, 0) + code_bits(6, 2)
        longest = max(longest, vlc_code(0, lvl if at == 0 else (lvl - 2) * 2 + sign)[0])
        par.append((8, 0, (0, 5, 31)[len(par) % 3], CO_WORDS * 32)); coef.append(c); want.append(np.array(w, dtype=np.uint8))
    return np.array(par, dtype=np.int32), np.array(coef), want, longest


def check_long_codewords(run):
    """run(par, coef, buf_single, buf_team) -> (out, buf_single, buf_team)."""
    par, coef, want, longest = long_codeword_cases()
    assert longest > 32
    fill = np.full((len(par), CO_WORDS), FILL, dtype=np.uint32)
    out, b1, bt = run(par, coef, fill, fill.copy())
    bad = [f'item {i}: counted {out[i, :2].tolist()}, string has {len(w)} bits' for i, w in enumerate(want) if not (out[i, 0] == out[i, 1] == len(w))]
    bad += check_emitted('bs_coeff', word_bits(b1), out[:, 2], out[:, 3], want, par[:, 2])
    bad += check_emitted('bs_coeff_team', word_bits(bt), out[:, 4], out[:, 5], want, par[:, 2])
    assert not bad, '\n'.join(bad[:8])


def check_overflow(run):
    """Capacity one to three whole words short of the string's end: ovf set, pos still the full length, every word from the capacity on untouched."""
    ln = K9['co_len']
    sel = np.flatnonzero(ln >= 200)[::9]
    assert len(sel) >= 50
    par = np.zeros((len(sel), 4), dtype=np.int32)
    par[:, :2] = K9['co_par'][sel]; par[:, 2] = np.arange(len(sel)) % 40
    par[:, 3] = 32 * ((par[:, 2] + ln[sel]) // 32 - 1 - np.arange(len(sel)) % 3)
    assert (par[:, 3] < par[:, 2] + ln[sel]).all() and (par[:, 3] > 64).all()
    fill = np.full((len(sel), CO_WORDS), FILL, dtype=np.uint32)
    out, b1, bt = run(par, np.ascontiguousarray(K9['co_coef'][sel]), fill, fill.copy())
    bad = []
    for i in range(len(sel)):
        for name, buf, o in (('bs_coeff', b1, out[i, 2:4]), ('bs_coeff_team', bt, out[i, 4:6])):
            if o[1] != 1 or o[0] != par[i, 2] + ln[sel[i]]: bad.append(f'{name} item {i}: pos {o[0]} ovf {o[1]}, want pos {par[i, 2] + ln[sel[i]]} ovf 1')
            elif (buf[i, par[i, 3] // 32:] != FILL).any(): bad.append(f'{name} item {i}: a word past the capacity of {par[i, 3]} bits changed')
    assert not bad, '\n'.join(bad[:8])
