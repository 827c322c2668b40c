"""CPU tests of the lzw / lz78 batch interface (no GPU): the five symbols, the refusals that are decided before the context is looked
at, the two bounds against their formula and against the model's streams, the facades, and that the batches of tests/lz_batches.py
reach the forks they are named for."""
import ctypes

import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batches as B
from tests.models import lzw as M

ERR_ARG, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -4, -6
NAMES = ("tdc_gpu_lzw_compress_batch", "tdc_gpu_lzw_batch_bound", "tdc_gpu_lz78_compress_batch", "tdc_gpu_lz78_batch_bound",
         "tdc_gpu_lz_parse_batch")
TAKEN = {"lzw": (T.CODER_BIT, T.CODER_GAMMA), "lz78": (T.CODER_GAMMA,)}
ALL_CODERS = (T.CODER_HUFF, T.CODER_GAMMA, T.CODER_ARITH, T.CODER_ASCII, T.CODER_SLE, T.CODER_BIT, T.CODER_DELTA, 99)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_facades():
    lib = T._native.load()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.tdc_gpu_lzw_batch_bound.restype is ctypes.c_size_t and lib.tdc_gpu_lz78_batch_bound.restype is ctypes.c_size_t
    for name in ("lzw_compress_batch", "lzw_compress_batch_into", "lz78_compress_batch", "lz78_compress_batch_into", "lz_parse_batch"):
        assert hasattr(T.Context, name)
    assert callable(T.lzw_batch_bound) and callable(T.lz78_batch_bound)
    assert callable(T.LZWCompressor(None).compress_batch) and callable(T.LZ78Compressor(None).compress_batch)
    assert "lz_batch_hash_bits" not in T.option_names()                                     # an option of the context, not enumerated


def bound(algo, lengths, coder):
    return (T.lzw_batch_bound if algo == "lzw" else T.lz78_batch_bound)(lengths, coder)


def test_bounds_are_their_formula():
    lengths = [0, 1, 2, 7, 8, 0, 0, 255, 256, 257, 300, 767, 768, 769, 4095, 4096, 4097, 70001, B.TEXT_CAP, B.TEXT_CAP + 1, 0]
    for algo, coder, name in (("lzw", T.CODER_BIT, "bit"), ("lzw", T.CODER_GAMMA, "gamma"), ("lz78", T.CODER_GAMMA, "gamma")):
        assert bound(algo, lengths, coder) == sum(B.text_bound(n, algo, name) for n in lengths) > 0
        for n in lengths:
            assert bound(algo, [n], coder) == B.text_bound(n, algo, name)
        assert bound(algo, [], coder) == 0                                                  # no text: no byte
        assert bound(algo, [0], coder) == 8                                                 # the terminator, rounded up


def test_bounds_are_zero_where_the_call_refuses():
    L = T._native.load()
    for algo in ("lzw", "lz78"):
        f = getattr(L, "tdc_gpu_%s_batch_bound" % algo)
        for coder in ALL_CODERS:
            assert (bound(algo, [100, 5], coder) > 0) == (coder in TAKEN[algo]), (algo, coder)
        g = T.CODER_GAMMA
        assert f(None, 1, g) == 0
        assert f(ptr(np.array([1, 5], dtype=np.uint64)), 1, g) == 0                         # in_off[0] != 0
        assert f(ptr(np.array([0, 5, 3], dtype=np.uint64)), 2, g) == 0                      # decreasing
        assert f(ptr(np.array([0, 1 << 31, 0xFFFFFFFF], dtype=np.uint64)), 2, g) == 0       # 2^32 - 1 bytes
        assert f(ptr(np.array([0, 1 << 31, 0xFFFFFFFE], dtype=np.uint64)), 2, g) > 0


def test_bounds_hold_the_models_streams():
    rng = np.random.default_rng(20261020)
    for n in (0, 1, 2, 3, 9, 100, 255, 256, 257, 1000, 3000):
        for _ in range(3):
            x = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            for name, coder in B.LZW_CODERS.items():
                assert len(M.compress(x, name)) <= bound("lzw", [n], coder)
            if not B.lz78_status(x):
                assert len(B.lz78_stream(x)) <= bound("lz78", [n], T.CODER_GAMMA)
    for x in B.batch("depth_9000") + B.batch("width_borders")[-3:]:                          # few long phrases; many short ones
        assert len(B.lzw_stream(x, "bit")) <= bound("lzw", [len(x)], T.CODER_BIT)
        assert len(B.lzw_stream(x, "gamma")) <= bound("lzw", [len(x)], T.CODER_GAMMA)
        assert len(B.lz78_stream(x)) <= bound("lz78", [len(x)], T.CODER_GAMMA)


def compress_status(algo, in_off, coder=T.CODER_GAMMA, null=()):
    """the status of a compress batch call without a context (NULL): what the arguments alone decide comes first"""
    L = T._native.load()
    off = np.asarray(in_off, dtype=np.uint64)
    count = len(off) - 1
    text, out = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    out_off, out_len, status = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.int32)
    arg = {"in": ptr(text), "in_off": ptr(off), "out": ptr(out), "out_off": ptr(out_off), "out_len": ptr(out_len), "status": ptr(status)}
    for name in null:
        arg[name] = None
    return getattr(L, "tdc_gpu_%s_compress_batch" % algo)(None, arg["in"], arg["in_off"], count, coder, arg["out"], 64, arg["out_off"],
                                                          arg["out_len"], arg["status"], None)


@pytest.mark.parametrize("algo", ("lzw", "lz78"))
def test_compress_refusals_that_need_no_device(algo):
    good = [0, 5, 5, 20]
    for name in ("in", "in_off", "out", "out_off", "out_len", "status"):
        assert compress_status(algo, good, null=(name,)) == ERR_ARG, name
    assert compress_status(algo, [0, 5, 4, 20]) == ERR_ARG                                  # a decreasing in_off
    assert compress_status(algo, [1, 5, 5, 20]) == ERR_ARG                                  # in_off[0] != 0
    for coder in ALL_CODERS:
        assert compress_status(algo, good, coder=coder) == (ERR_ARG if coder in TAKEN[algo] else ERR_UNSUPPORTED), coder
    assert compress_status(algo, [1, 5, 5, 20], coder=T.CODER_HUFF) == ERR_UNSUPPORTED      # the coder before the offsets, as the lzss batch
    assert compress_status(algo, [0, 1 << 31, 0xFFFFFFFF]) == ERR_TOO_LARGE                 # by the offsets alone: nothing is read
    assert compress_status(algo, good) == ERR_ARG                                           # all is well but the context: NULL


def test_parse_refusals_that_need_no_device():
    L = T._native.load()
    text, items, chars = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint8)
    item_off, status = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.int32)

    def call(offsets, lzw, null=None):
        off = np.asarray(offsets, dtype=np.uint64)
        a = {"in": ptr(text), "in_off": ptr(off), "items": ptr(items), "chars": ptr(chars), "item_off": ptr(item_off), "status": ptr(status)}
        if null:
            a[null] = None
        return L.tdc_gpu_lz_parse_batch(None, a["in"], a["in_off"], len(off) - 1, lzw, a["items"], a["chars"], a["item_off"], a["status"])

    good = [0, 5, 5, 20]
    for lzw in (0, 1):
        for name in ("in", "in_off", "items", "item_off", "status"):
            assert call(good, lzw, name) == ERR_ARG, name
        assert call([0, 5, 4, 20], lzw) == ERR_ARG and call([1, 5, 5, 20], lzw) == ERR_ARG
        assert call([0, 1 << 31, 0xFFFFFFFF], lzw) == ERR_TOO_LARGE
        assert call(good, lzw) == ERR_ARG                                                   # the NULL context
    assert call(good, 0, "chars") == ERR_ARG                                             # lz78 needs its chars


def test_the_batches_hold_what_they_promise():
    assert B.batch("count0") == ()
    e = B.batch("empties")
    assert e[0] == e[-1] == b"" and e[4] == b"" and sum(1 for x in e if x) == 2
    for n in (2210, 2211, 2212, 5000, 9000):                                                # phrase lengths 1, 2, 3, ...: above 64 from the 65th on
        ids, chars = B.lz78_pairs(B.batch("depth_%d" % n)[1])
        assert ids.tolist()[:65] == list(range(65)) and set(chars) == {ord("a")}
    assert len(B.lz78_pairs(b"a" * 2211)[0]) == 66 and len(B.lz78_pairs(b"a" * 2212)[0]) == 67       # 2211 ends with its 66th phrase
    assert len(B.lz78_pairs(b"a" * 9000)[0]) > 129                                          # depths above 128
    codes = B.lzw_codes(b"a" * 5000)
    assert (codes[1:-1] == 255 + np.arange(1, len(codes) - 1)).all() and len(codes) > 66     # KwKwK at every step, beyond depth 64
    status = [B.lz78_status(x) for x in B.batch("leftover_7f_80")]
    assert status == [0, 0, 0, ERR_UNSUPPORTED, 0, ERR_UNSUPPORTED, 0]
    assert B.lz78_pairs(b"\x7f\x7f")[0].tolist() == [0, 0]                                  # the left-over pair repeats the first
    for x, want in B.kats("lzw"):
        assert B.lzw_codes(x).tolist() == list(want)
    for x, want in B.kats("lz78"):
        ids, chars = B.lz78_pairs(x)
        assert tuple(zip(ids.tolist(), chars)) == want
    assert len(B.kats("lzw")) == 8
    for sigma in (2, 256):                                                                  # the table of 2^j - 1 bytes is half that of 2^j
        lens = [len(x) for x in B.batch("capacity_sigma%d" % sigma)]
        assert lens == [1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
    assert tuple(len(B.lzw_codes(x)) for x in B.batch("width_borders")) == B.LZW_COUNTS
    assert {5, 6, 255, 256, 257, 767, 768, 769, 2047, 2048, 2049, 4097} <= set(B.LZW_COUNTS)
    tiny = B.batch("tiny5000")
    assert len(tiny) == 5000 and min(len(x) for x in tiny) == 3 and max(len(x) for x in tiny) == 40
    assert [len(x) for x in B.batch("one_mib")] == [4096, 1 << 20, 4096]
    same = B.batch("identical64")
    assert len(same) == 64 and len(set(same)) == 1
    assert max(len(x) for x in B.batch("mixed")) <= 2211 and b"" in B.batch("mixed")
    for name in B.NAMES:                                                                    # every accepted stream decodes, on the host
        for x in B.batch(name)[:12]:
            if len(x) <= 10000:
                assert B.lzw_decode(B.lzw_stream(x, "bit"), "bit") == x and B.lzw_decode(B.lzw_stream(x, "gamma"), "gamma") == x
                if not B.lz78_status(x):
                    assert B.lz78_decode(B.lz78_stream(x)) == x
