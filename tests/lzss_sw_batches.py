"""The batches of tests/test_gpu_lzss_sw_batch.py and tests/test_gpu_lzss_sw_batch_decode.py, and what the host specification says of
them: per text the stream M.encode(tokens) of tests/models/lzss_sw.py, the tokens from M.parse for small texts and from the host parse
tdc_lzss_sw_factors for larger ones.  encode_fast() builds the fields of M.encode with numpy (tests/test_lzss_sw_batch_cli.py holds the
two against each other); expected() is cached, so the two test files compute every reference once.

Tile = 4096 text positions, the match kernel's unit (lzss_sw_batch.hip)."""
import functools

import numpy as np

import tudocomp_amd as T
from tests.models import lzss_sw as M
from tests.models.lzss_coders import _np_code, bits_for

TILE = 4096
CODER_ID = {"ascii": T.CODER_ASCII, "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
WINDOWS, THRESHOLDS = (1, 3, 16, 4096), (0, 3)


def small(data, w):
    """texts that go through M.parse (about n * min(n, w) candidates); the others through tdc_lzss_sw_factors"""
    return len(data) * min(len(data), w) <= 20000


def material(n, seed, sigma=3):
    """n bytes over `sigma` letters: matches everywhere, at every window"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, sigma, size=n, dtype=np.uint8) + ord("a")).tobytes()


def cut(data, lengths):
    """consecutive pieces of `data` of the given lengths"""
    out, p = [], 0
    for ln in lengths:
        out.append(data[p:p + ln])
        p += ln
    assert p <= len(data)
    return out


@functools.lru_cache(maxsize=None)
def batch(name):
    """a list of texts"""
    if name == "tile_edges":                      # borders at positions 4095, 4096, 4097, 8191, 8192, 8193, 12289 and 16386
        return cut(material(5 * TILE, 1), [4095, 1, 1, 4094, 1, 1, 4096, 4097, 100])
    if name == "three_tiles":                     # a text of three tiles between texts of 1 - 3 bytes
        return cut(material(4 * TILE, 2, 2), [2, 3 * TILE + 5, 1, 3, 700, 2])
    if name == "tiny":                            # 5000 texts of 0 .. 7 bytes in a row: more than a thousand texts in one tile
        rng = np.random.default_rng(3)
        return cut(material(8 * 5000, 4, 2), rng.integers(0, 8, size=5000).tolist())
    if name == "empties":                         # empty texts first, last and in runs -- one run longer than a tile's staged borders
        data = material(3 * TILE, 5)
        return [b"", b"", b""] + cut(data, [10]) + [b""] + cut(data[10:], [300]) + [b""] * 4 + cut(data[310:], [5000]) + [b""] * 3000 \
            + cut(data[5310:], [TILE, 7]) + [b"", b""]
    if name == "only_empties":
        return [b""] * 5
    if name == "copies":                          # the same 300 bytes three times: no source in front of a text's start
        return [material(300, 6)] * 3
    if name == "lookahead":                       # ...abcabc | abc...: the last factor of the first text must not grow into the second
        return [b"xyzxyzzabcabc", b"abcabcabcq", b"abc"]
    if name == "widths":                          # 40 texts of 300 bytes: local positions pass 2, 4, ..., 256, the global ones do not
        return cut(material(40 * 300, 7, 2), [300] * 40)
    if name == "truncation":                      # window 3, bit: the lengths 4 and 5 of "aaaaaaaa" do not fit 2 bits
        return [b"abcabdab", b"aaaaaaaa", b"bcdbcebc"]
    if name == "one":
        return [material(3 * TILE + 17, 8)]
    if name == "english":                         # 512 pieces of gen_english, lengths drawn from 0 .. 40000 (small ones more often)
        rng = np.random.default_rng(9)
        lengths = (40000 * rng.random(512) ** 4).astype(np.int64)
        lengths[[0, 17, 511]] = 0
        lengths[5] = 40000
        data = T.gen_english(int(lengths.sum()), 42).tobytes()
        return cut(data, lengths.tolist())
    raise ValueError(name)


def window_batch(w):
    """texts of w - 1, w, w + 1, 2w - 1, 2w, 2w + 1 bytes back to back: the look-ahead rule changes at n >= 2w, per text"""
    lengths = [w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1]
    return cut(material(sum(lengths), 10 + w, 2), lengths)


def tokens_of(data, w, t):
    """the token list of M.parse, from the host parse for longer texts"""
    if small(data, w):
        return M.parse(data, w, t)
    pos, src, ln = T.lzss_sw_factors(data, w, t)
    toks, p = [], 0
    for q, s, j in zip(pos.tolist(), src.tolist(), ln.tolist()):
        toks.extend((i, None, data[i]) for i in range(p, q))
        toks.append((q, s, j))
        p = q + j
    toks.extend((i, None, data[i]) for i in range(p, len(data)))
    return toks


def encode_fast(data, factors, coder, w):
    """M.encode(tokens, coder, w) for the tokens that the factor list (pos, src, len arrays, sorted by pos) and the literals in
    between make, with numpy"""
    text = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(text)
    pos, src, ln = (np.asarray(a, dtype=np.int64) for a in factors)
    covered = np.zeros(n + 1, dtype=np.int64)
    np.add.at(covered, pos, 1)
    np.add.at(covered, pos + ln, -1)
    lit = np.flatnonzero(np.cumsum(covered)[:n] == 0)
    if coder == "ascii":
        parts = [(int(p), b"0" + bytes([int(text[p])])) for p in lit.tolist()]
        parts += [(int(p), b"1%d:%d:" % (p - s, j)) for p, s, j in zip(pos.tolist(), src.tolist(), ln.tolist())]
        body = b"".join(x for _, x in sorted(parts))
        return body + b"\x00"                                      # (whole bytes: the terminator is a byte of its own)
    keys, vals, wid = [], [], []

    def add(at, order, vw):
        keys.append(np.asarray(at, dtype=np.int64) * 4 + order)
        vals.append(np.asarray(vw[0], dtype=np.uint64))
        wid.append(np.asarray(vw[1], dtype=np.int64))

    add(lit, 0, (np.zeros(len(lit), dtype=np.uint64), np.ones(len(lit), dtype=np.int64)))
    add(pos, 0, (np.ones(len(pos), dtype=np.uint64), np.ones(len(pos), dtype=np.int64)))
    add(lit, 1, _np_code(text[lit], coder, 8))
    if coder == "bit":
        dw = np.array([bits_for(p) for p in pos.tolist()], dtype=np.int64)
        add(pos, 1, ((pos - src).astype(np.uint64) & ((np.uint64(1) << dw.astype(np.uint64)) - np.uint64(1)), dw))
        lw = bits_for(w)
        add(pos, 2, (ln.astype(np.uint64) & np.uint64((1 << lw) - 1), np.full(len(pos), lw, dtype=np.int64)))
    else:
        add(pos, 1, _np_code(pos - src, coder))
        add(pos, 2, _np_code(ln, coder))
    keys, vals, wid = np.concatenate(keys), np.concatenate(vals), np.concatenate(wid)
    order = np.argsort(keys, kind="stable")
    vals, wid = vals[order], wid[order]
    first = np.cumsum(wid) - wid
    total = int(wid.sum())
    idx = np.repeat(np.arange(len(wid)), wid)
    shift = (wid[idx] - 1 - (np.arange(total) - first[idx])).astype(np.uint64)
    bits = ((vals[idx] >> shift) & np.uint64(1)).astype(np.uint8)
    u = total % 8
    out = bytearray(np.packbits(bits).tobytes())
    if u == 0:
        out.append(0)
    elif u <= 5:
        out[-1] |= u
    else:
        out.append(u)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _expected_text(data, w, t):
    """{coder: (status, stream)} of one text: what the single call returns for it"""
    if small(data, w):
        toks = M.parse(data, w, t)
        trunc = any(j >> bits_for(w) for _, s, j in toks if s is not None)
        return {coder: (ERR_UNSUPPORTED, b"") if coder == "bit" and trunc else (0, M.encode(toks, coder, w)) for coder in M.CODERS}
    f = T.lzss_sw_factors(data, w, t)
    trunc = bool((f[2] >> bits_for(w)).any())
    return {coder: (ERR_UNSUPPORTED, b"") if coder == "bit" and trunc else (0, encode_fast(data, f, coder, w)) for coder in M.CODERS}


def expected(texts, w, t, coder):
    """([status], [stream]) of a batch"""
    per = [_expected_text(x, w, t)[coder] for x in texts]
    return [s for s, _ in per], [x for _, x in per]

