"""Batches for the lzw / lz78 batch calls (tudocomp_amd/csrc/lz_batch.hip) and what they must yield, from code that is not under test:
tests/models/lzw.py, the oracle's lz78 and the host parses tdc_lzw_factors / tdc_lz78_factors.  Every batch is named for the fork of the
parse kernel it reaches; tests/test_lz_batch_cli.py checks on the CPU that it does, tests/test_gpu_lz_batch.py runs it."""
import functools
import json
import os

import numpy as np

import tudocomp_amd as T
from oracle import oracle as O
from tests import coder_borders as CB
from tests.models import lzw as M
from tests.models import lz78_decode as D

ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -4, -5, -6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXT_CAP = (1 << 25) - 256                      # the longest text of a batch (include/tdc_gpu.h)
LZW_CODERS = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA}
# code counts at which lzw(coder=bit) changes its width (code k takes bits_for(k + 256) bits), and the field coder's tile borders
LZW_COUNTS = tuple(sorted(set(CB.LZW_COUNTS + (255, 256, 257, 767, 768, 769, 1791, 1792, 1793, 3839, 3840, 3841))))


def rnd(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8).tobytes()


def english(n, seed):
    return T.gen_english(n, seed).tobytes()


def lzw_lengths(codes):
    """phrase lengths of an lzw code list: entry 256 + j is phrase j and one more byte"""
    lens = np.ones(len(codes), dtype=np.int64)
    for k, c in enumerate(codes):
        if c >= 256:
            lens[k] = lens[int(c) - 256] + 1
    return lens


@functools.lru_cache(maxsize=None)
def kats(which):
    if which == "lzw":
        rows = json.load(open(os.path.join(GOLDEN, "lzw_kats.json")))["lzw_codes"]
        return tuple((bytes.fromhex(r["input_hex"]), tuple(r["codes"])) for r in rows)
    rows = json.load(open(os.path.join(GOLDEN, "reference_kats.json")))["lz78_factors"]
    return tuple((bytes.fromhex(r["input_hex"]), tuple(tuple(p) for p in r["pairs"])) for r in rows)


def _depth(n):
    return [b"xy", b"a" * n, b"q"]


def _capacity(sigma):
    """2^j - 1, 2^j, 2^j + 1 bytes: 2 (n + 1) lies on both sides of a power of two, the table doubles between the first two"""
    return [rnd((1 << j) + d, sigma, 100 * j + d + sigma) for j in (10, 11, 12) for d in (-1, 0, 1)]


def _width_borders():
    base = rnd(16 << 10, 256, 4097)
    codes = T.lzw_factors(base)
    assert len(codes) > max(LZW_COUNTS)
    return [x for _, x in CB.phrase_prefixes(base, lzw_lengths(codes), LZW_COUNTS)]


def _tiny5000():
    rng = np.random.default_rng(5000)
    lens = rng.integers(3, 41, 5000)
    return [rng.integers(97, 101, int(n), dtype=np.uint8).tobytes() for n in lens]


def _mixed():
    return [b"", rnd(1025, 2, 1), rnd(300, 256, 2), b"a" * 2211, b"ab" * 300, english(1500, 3), b"", b"\x00" * 200, rnd(700, 4, 4)]


_BATCHES = {
    "count0": lambda: [],
    "empties": lambda: [b""] * 3 + [b"abcabcabc"] + [b""] * 4 + [b"the cat sat on the mat"] + [b""] * 2,
    "only_empties": lambda: [b""] * 5,
    "one_two_bytes": lambda: [b"a", b"ab", b"aa", b"\x00", b"\xff", b"\x00\x00", b"\xff\xff", b"\x7f\x7f", b"\x80", b"\x00\xff", b"z"],
    "depth_2210": lambda: _depth(2210),          # lz78 phrases of a^n are 1, 2, 3, ... bytes long: the 66th starts the second depth turn
    "depth_2211": lambda: _depth(2211),          # ... and ends the text exactly
    "depth_2212": lambda: _depth(2212),
    "depth_5000": lambda: _depth(5000),          # depths above 64: one continuation turn; lzw: KwKwK all the way
    "depth_9000": lambda: _depth(9000),          # depths above 128: two
    "abab": lambda: [b"ab" * 700, b"c", b"ab" * 3000, b"ba" * 33],
    "ends": lambda: [b"abcabd", b"abcab", b"aab", b"aaba", b"aabaa", b"abababab", b"ababababa"],
    "leftover_7f_80": lambda: [b"hello world", b"\x7f\x7f", b"hello again", b"\x80\x80", b"and again", b"ab\x80ab\x80", b"ab\xffab"],
    "bytes_00_ff": lambda: [b"\x00" * 300, b"\xff" * 301, rnd(2000, 2, 7).replace(b"\x01", b"\xff"), b"\x00" * 2211, b"\xff" * 2212],
    "lzw_kats": lambda: [x for x, _ in kats("lzw")],
    "lz78_kats": lambda: [x for x, _ in kats("lz78")],
    "capacity_sigma2": lambda: _capacity(2),
    "capacity_sigma256": lambda: _capacity(256),
    "width_borders": _width_borders,
    "tiny5000": _tiny5000,
    "one_mib": lambda: [english(4096, 11), english(1 << 20, 12), english(4096, 13)],
    "identical64": lambda: [english(2048, 64)] * 64,
    "mixed": _mixed,
}
NAMES = tuple(_BATCHES)


@functools.lru_cache(maxsize=None)
def batch(name):
    return tuple(_BATCHES[name]())


# ---- what a text must yield ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lzw_codes(x):
    """the codes of text x: the model's parse; for long texts the host parse"""
    if len(x) <= 1 << 16:
        return np.array(M.parse(x), dtype=np.uint32)
    return T.lzw_factors(x)


@functools.lru_cache(maxsize=None)
def lzw_stream(x, coder):
    codes = lzw_codes(x)
    return M.encode(codes.tolist(), coder) if len(codes) < 4096 else M.encode_fast(codes, coder)


@functools.lru_cache(maxsize=None)
def lz78_pairs(x):
    ids, chars = O.lz78_factors(x)
    return ids, bytes(chars)


@functools.lru_cache(maxsize=None)
def lz78_status(x):
    """-6 where the single call refuses x: the text ends inside the dictionary -- its last pair names a node that exists, so it
    repeats an earlier pair -- on a byte >= 0x80"""
    ids, chars = lz78_pairs(x)
    if len(ids) == 0 or chars[-1] < 0x80:
        return 0
    pairs = list(zip(ids.tolist(), chars))
    return ERR_UNSUPPORTED if pairs[-1] in set(pairs[:-1]) else 0


@functools.lru_cache(maxsize=None)
def lz78_stream(x):
    return b"" if lz78_status(x) else O.lz78_gamma_compress(x)


@functools.lru_cache(maxsize=None)
def lzw_decode(stream, coder):
    return T.lzw_decode(stream, LZW_CODERS[coder])


@functools.lru_cache(maxsize=None)
def lz78_decode(stream):
    """the host loop of LZ78Compressor::decompress"""
    return D.sequential_decode(stream)


# ---- the bounds, restated ----------------------------------------------------------------------------------------------------------------
def stream_len(bits):
    return bits // 8 + (1 if bits % 8 <= 5 else 2)


def text_bound(n, algo, coder):
    """n items, every field at its widest for a text of n bytes, and the terminator; rounded up to 8"""
    if algo == "lz78":
        bits = n * (2 * M.bits_for(n) + 1 + 17)
    elif coder == "bit":
        bits = M.offset(n)
    else:
        bits = n * (2 * M.bits_for(n + 255) + 1)
    return (stream_len(bits) + 7) // 8 * 8
