"""CPU tests of the interface of repair's batch decoder (no GPU): the symbol, the facades, the argument refusals that are decided before
the context is looked at -- in their documented order, the NULL context last --, and the expectations
tests/test_gpu_repair_batch_decode.py relies on, checked against the models and the host loop."""
import ctypes

import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batches as LB
from tests import many_texts as MT
from tests import repair_batch_decode_cases as C
from tests.models import repair as M
from tests.models import repair_batch_decode as B

NAME = "tdc_gpu_repair_decompress_batch"


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host(stream, coder):
    """(status, text) of the host loop tdc_repair_decode on one stream"""
    try:
        return 0, T.repair_decode(stream, C.CODER_ID[coder])
    except T.TdcGpuError as e:
        return e.status, b""


def test_symbol_and_facades():
    lib = T._native.load()
    assert NAME in T.SYMBOLS and hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes is not None and len(getattr(lib, NAME).argtypes) == 11
    assert hasattr(T.Context, "repair_decompress_batch") and hasattr(T.Context, "repair_decompress_batch_into")
    assert hasattr(T.RePairCompressor, "decompress_batch")


def test_refusals_that_need_no_device():
    fn = getattr(T._native.load(), NAME)
    blob = np.zeros(64, dtype=np.uint8)
    s_off, s_len = np.array([0, 8], dtype=np.uint64), np.array([3, 3], dtype=np.uint64)
    out_off, status = np.full(3, 7, dtype=np.uint64), np.full(2, 7, dtype=np.int32)
    out = np.full(32, 0xA5, dtype=np.uint8)

    def call(coder=T.CODER_GAMMA, count=2, **other):
        a = {"blob": ptr(blob), "s_off": ptr(s_off), "s_len": ptr(s_len), "out_off": ptr(out_off), "status": ptr(status)}
        a.update(other)
        return fn(None, a["blob"], a["s_off"], a["s_len"], count, coder, ptr(out), out.size, a["out_off"], a["status"], None)

    for arg in ("blob", "s_off", "s_len", "out_off", "status"):
        assert call(**{arg: None}) == C.ERR_ARG, arg
    for coder in (T.CODER_HUFF, T.CODER_ASCII, T.CODER_ARITH, T.CODER_SLE, 99, -1):
        assert call(coder=coder) == C.ERR_UNSUPPORTED, coder
        assert call(coder=coder, s_off=None, out_off=None) == C.ERR_UNSUPPORTED              # the coder comes first
    wrap = np.array([3, 0xFFFFFFFFFFFFFFFE], dtype=np.uint64)                 # a stream whose end overflows
    assert call(s_off=ptr(wrap)) == C.ERR_ARG
    assert call(s_off=ptr(wrap), coder=T.CODER_ASCII) == C.ERR_UNSUPPORTED
    empty = np.array([0, 0], dtype=np.uint64)                                 # no blob is fine where no stream has a byte
    assert call(blob=None, s_len=ptr(empty)) == C.ERR_ARG == call()           # ... so both end at the NULL context
    assert call(count=0, s_off=None, s_len=None, status=None) == C.ERR_ARG    # count = 0 needs out_off alone; then the NULL context
    assert call(count=0, out_off=None) == C.ERR_ARG
    for coder in C.CODER_ID.values():
        assert call(coder=coder) == C.ERR_ARG                                 # accepted: the NULL context, last
    assert (out == 0xA5).all() and (out_off == 7).all() and (status == 7).all()   # nothing was written on the way


@pytest.mark.parametrize("coder", C.CODERS)
def test_round_trip_streams_decode_to_their_texts(coder):
    for name in ("mixed", "ends", "one_two_bytes", "empties", "only_empties", "abab", "bytes_00_ff", "depth_2211", "width_borders"):
        for x in LB.batch(name):
            s = C.stream_of(x, coder)
            assert host(s, coder) == (0, x) == B.expected(s, coder)[:2], name
    for s, x in zip(C.known(coder), C.KNOWN):
        assert host(s, coder) == (0, x)


@pytest.mark.parametrize("coder", C.CODERS)
def test_foreign_grammars_and_long_streams(coder):
    for nr in C.RULE_COUNTS:
        s, x = C.foreign_stream(nr, coder)
        assert len(M.parse(s, coder)[0]) == nr and host(s, coder) == (0, x)
    for s, x in C.long_streams(coder):
        assert len(s) > 5 * 1024 and host(s, coder) == (0, x)
    assert B.expected(C.long_streams(coder)[1][0], coder)[:2] == (0, C.long_streams(coder)[1][1])


@pytest.mark.parametrize("coder", C.CODERS)
def test_minimal_and_own_stream_cases(coder):
    for s, want in C.minimal(coder):
        assert host(s, coder)[0] == want == B.expected(s, coder)[0]
    assert host(C.minimal(coder)[1][0], coder) == (0, b"")
    streams, status, texts = C.own_stream_batch(coder)
    for s, v, x in zip(streams, status, texts):
        assert host(s, coder) == (v, x) == B.expected(s, coder)[:2]
    assert B.decode_batch(streams, coder)[1:3] == (texts, status)


@pytest.mark.parametrize("coder", C.CODERS)
def test_damaged_expectations(coder):
    """the expected verdicts are the host loop's, but for the streams the model excepts -- computed from the stream: the first token the
    walk does not read crosses a cap, and the host loop does not refuse the stream"""
    streams, status, texts, excepted = C.damaged(coder)
    assert len(streams) == C.DAMAGED[coder] + 2
    assert excepted <= C.EXCEPTED_MOST * len(streams) and (coder != "bit" or excepted == 0)
    differ = 0
    for s, v, x in zip(streams, status, texts):
        h = host(s, coder)
        if h != (v, x):
            assert v == C.ERR_ARG and x == b"" and h[0] != C.ERR_ARG and B.expected(s, coder)[2]
            differ += 1
    assert differ == excepted
    assert set(status) >= {0, C.ERR_ARG}


@pytest.mark.parametrize("coder", C.CODERS)
def test_depth_cases(coder):
    streams, texts, at_d, below = C.depth_batch(coder)
    for s, x in zip(streams, texts):
        assert host(s, coder) == (0, x)                                       # the host loop has no cap
    assert [B.expected(s, coder, C.DEPTH)[0] for s in streams] == at_d
    assert [B.expected(s, coder, C.DEPTH - 1)[0] for s in streams] == below
    assert max(B.heights(M.parse(streams[3], coder)[0])) == C.DEPTH           # the deep rule that nothing names


@pytest.mark.parametrize("coder", C.CODERS)
def test_claims(coder):
    assert host(C.doubling(30, [30, 30], coder), coder)[0] == C.ERR_TOO_LARGE
    assert host(C.bad_and_large(coder), coder)[0] == C.ERR_ARG
    assert B.expected(C.doubling(30, [30], coder), coder, decode=False)[0] == 0
    rules, start = M.parse(C.doubling(30, [30], coder), coder)
    assert M.expansion_lengths(rules)[30] == 2**31 and start == [256 + 30]
    for top in (C.MOVE_TOP - 1, C.MOVE_TOP):
        s = C.doubling(top, [top], coder)
        rules, start = M.parse(s, coder)
        assert len(s) <= 64 and M.expansion_lengths(rules)[top] == 2 << top and start == [256 + top]
    assert B.expected(C.doubling(9, [9], coder), coder)[:2] == (0, b"a" * 1024)


def test_two_bit_tokens():
    s = C.two_bit_tokens(1000)
    assert len(s) == (35 + 2000) // 8 + 1 and host(s, "gamma") == (0, b"ab" * 1000) == B.expected(s, "gamma")[:2]
    big = C.two_bit_tokens(1 << 20)
    assert 4 * (len(big) - 8) <= (1 << 20) + 2 <= 4 * len(big)                # four tokens per stream byte


def test_many_streams_pool():
    for coder in ("bit", "gamma"):
        streams = MT.repair_streams(coder)
        for j in (0, 1, 5, 40, len(MT.pool()) - 1):
            assert host(streams[j].tobytes(), coder) == (0, MT.texts()[j])
        assert sum(1 for v in C.damaged(coder)[1] if v) >= 7
    assert MT.TRIPS3 > 2 * MT.CAP16 and MT.CAP16 == 1 << 16


def test_cpp_facade_compiles(tmp_path):
    """tdc_amd::RePairCompressor::decompress_batch hands the C call to lz_decompress_batch: taking its address makes the compiler
    instantiate that (no device is needed to compile it)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "facade.cpp"
    src.write_text('#include "tdc_amd.hpp"\n'
                   "using tdc_amd::bytes;\n"
                   "void (tdc_amd::RePairCompressor::*batch)(const std::vector<bytes>&, std::vector<bytes>&, std::vector<int32_t>&) =\n"
                   "    &tdc_amd::RePairCompressor::decompress_batch;\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "facade.o"),
                           "-I", os.path.join(root, "tudocomp_amd", "host"), "-I", os.path.join(root, "include")])
