"""CPU tests of the lzss batch interface (no GPU): the three symbols, tdc_gpu_lzss_sw_batch_bound against the single bounds, the argument
refusals that are decided before the context is looked at, and the numpy encoder of tests/lzss_sw_batches.py against the model's."""
import ctypes

import numpy as np
import pytest

import tudocomp_amd as T
from tests import lzss_sw_batches as B
from tests.models import lzss_sw as M

ERR_ARG, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -4, -6
NAMES = ("tdc_gpu_lzss_sw_compress_batch", "tdc_gpu_lzss_sw_batch_bound", "tdc_gpu_lzss_sw_decompress_batch")


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_facade():
    lib = T._native.load()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
    assert lib.tdc_gpu_lzss_sw_compress_batch.argtypes is not None and lib.tdc_gpu_lzss_sw_decompress_batch.argtypes is not None
    assert lib.tdc_gpu_lzss_sw_batch_bound.restype is ctypes.c_size_t
    for name in ("lzss_sw_compress_batch", "lzss_sw_compress_batch_into", "lzss_sw_decompress_batch", "lzss_sw_decompress_batch_into",
                 "lzss_sw_batch_bound"):
        assert hasattr(T.Context, name)
    assert hasattr(T.LZSSSlidingWindowCompressor, "compress_batch") and hasattr(T.LZSSSlidingWindowCompressor, "decompress_batch")


def test_bound_is_the_sum_of_the_rounded_single_bounds():
    lengths = [0, 1, 7, 8, 0, 0, 300, 4095, 4096, 4097, 70001, 0]
    for coder in B.CODER_ID.values():
        for w in (1, 3, 16, 4096):
            want = sum((T.lzss_sw_bound(n, w, coder) + 7) // 8 * 8 for n in lengths)
            assert T.lzss_sw_batch_bound(lengths, w, coder) == want > 0
    assert T.lzss_sw_batch_bound([], 16, T.CODER_BIT) == 0                                  # no text: no byte
    assert T.lzss_sw_batch_bound([0], 16, T.CODER_BIT) == 8                                 # the terminator, rounded up


def test_bound_is_zero_where_the_single_bound_is():
    for w, coder in ((0, T.CODER_BIT), (4097, T.CODER_BIT), (16, T.CODER_HUFF), (16, T.CODER_ARITH), (16, 99)):
        assert T.lzss_sw_bound(100, w, coder) == 0
        assert T.lzss_sw_batch_bound([100, 5], w, coder) == 0
    L = T._native.load()
    assert L.tdc_gpu_lzss_sw_batch_bound(None, 1, 16, T.CODER_BIT) == 0
    assert L.tdc_gpu_lzss_sw_batch_bound(ptr(np.array([1, 5], dtype=np.uint64)), 1, 16, T.CODER_BIT) == 0          # in_off[0] != 0
    assert L.tdc_gpu_lzss_sw_batch_bound(ptr(np.array([0, 5, 3], dtype=np.uint64)), 2, 16, T.CODER_BIT) == 0       # decreasing
    assert L.tdc_gpu_lzss_sw_batch_bound(ptr(np.array([0, 1 << 31, 0xFFFFFFFF], dtype=np.uint64)), 2, 16, T.CODER_GAMMA) == 0   # 2^32 - 1 bytes
    assert L.tdc_gpu_lzss_sw_batch_bound(ptr(np.array([0, 1 << 31, 0xFFFFFFFE], dtype=np.uint64)), 2, 16, T.CODER_GAMMA) > 0


def compress_status(in_off, window=16, coder=T.CODER_BIT, null=()):
    """the status of tdc_gpu_lzss_sw_compress_batch without a context (NULL): what the arguments alone decide comes first"""
    L = T._native.load()
    off = np.asarray(in_off, dtype=np.uint64)
    count = len(off) - 1
    text, out = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    out_off, out_len, status = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.int32)
    arg = {"in": ptr(text), "in_off": ptr(off), "out": ptr(out), "out_off": ptr(out_off), "out_len": ptr(out_len), "status": ptr(status)}
    for name in null:
        arg[name] = None
    return L.tdc_gpu_lzss_sw_compress_batch(None, arg["in"], arg["in_off"], count, window, 3, coder, arg["out"], 64, arg["out_off"],
                                            arg["out_len"], arg["status"], None)


def test_compress_refusals_that_need_no_device():
    good = [0, 5, 5, 20]
    for name in ("in", "in_off", "out", "out_off", "out_len", "status"):
        assert compress_status(good, null=(name,)) == ERR_ARG, name
    assert compress_status([0, 5, 4, 20]) == ERR_ARG                                        # a decreasing in_off
    assert compress_status([1, 5, 5, 20]) == ERR_ARG                                        # in_off[0] != 0
    assert compress_status(good, window=0) == ERR_ARG
    assert compress_status(good, window=4097) == ERR_UNSUPPORTED
    for coder in (T.CODER_HUFF, T.CODER_ARITH, T.CODER_SLE, 99):
        assert compress_status(good, coder=coder) == ERR_UNSUPPORTED
    assert compress_status([0, 1 << 31, 0xFFFFFFFF]) == ERR_TOO_LARGE                       # by the offsets alone: nothing is read
    assert compress_status(good) == ERR_ARG                                                 # all is well but the context: NULL


def test_decompress_refusals_that_need_no_device():
    L = T._native.load()
    blob = np.zeros(64, dtype=np.uint8)
    s_off, s_len = np.array([0, 8], dtype=np.uint64), np.array([3, 3], dtype=np.uint64)
    out_off, status = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.int32)

    def call(coder=T.CODER_GAMMA, window=16, **null):
        a = {"blob": ptr(blob), "s_off": ptr(s_off), "s_len": ptr(s_len), "out_off": ptr(out_off), "status": ptr(status)}
        a.update(null)
        return L.tdc_gpu_lzss_sw_decompress_batch(None, a["blob"], a["s_off"], a["s_len"], 2, coder, window, None, 0, a["out_off"], a["status"], None)

    for name in ("blob", "s_off", "s_len", "out_off", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    for coder in (T.CODER_ASCII, T.CODER_HUFF, T.CODER_ARITH, 99):                          # ascii: as on the single call's device path
        assert call(coder=coder) == ERR_UNSUPPORTED
    assert call(coder=T.CODER_BIT, window=0) == ERR_ARG
    assert call(coder=T.CODER_GAMMA, window=0) == ERR_ARG == call()                         # only bit reads the window; then the NULL context


def test_the_numpy_encoder_is_the_models():
    for data, w, t in M.sweep(20261020, 400):
        toks = M.parse(data, w, t)
        f = [tok for tok in toks if tok[1] is not None]
        fac = tuple(np.array([x[i] for x in f], dtype=np.int64) for i in range(3))
        for coder in M.CODERS:
            if coder == "bit" and M.truncates(data, w, t):
                continue
            assert B.encode_fast(data, fac, coder, w) == M.encode(toks, coder, w), (data, w, t, coder)
    for n, w in ((8000, 3), (3000, 16)):                                                    # (not small: through the host parse)
        data = B.material(n, 1)
        assert not B.small(data, w) and B.tokens_of(data, w, 3) == M.parse(data, w, 3)


def test_the_batches_hold_what_they_promise():
    ends = np.cumsum([len(x) for x in B.batch("tile_edges")])
    assert {4095, 4096, 4097, 8191, 8192, 8193} <= set(ends.tolist()) and {0, 1, 4095} <= set((ends % B.TILE).tolist())
    lens = [len(x) for x in B.batch("three_tiles")]
    assert max(lens) > 3 * B.TILE and lens[0] <= 3 and lens[2] <= 3 and lens[3] <= 3
    tiny = B.batch("tiny")
    assert len(tiny) == 5000 and set(len(x) for x in tiny) == set(range(8)) and sum(len(x) for x in tiny) < 5 * B.TILE
    e = B.batch("empties")
    assert e[0] == e[-1] == b"" and sum(1 for x in e if not x) > 3000
    eng = B.batch("english")
    assert len(eng) == 512 and max(len(x) for x in eng) == 40000 and min(len(x) for x in eng) == 0 and sum(len(x) for x in eng) <= 10_000_000
    assert M.truncates(B.batch("truncation")[1], 3, 3) and not M.truncates(B.batch("truncation")[0], 3, 3) and not M.truncates(B.batch("truncation")[2], 3, 3)
