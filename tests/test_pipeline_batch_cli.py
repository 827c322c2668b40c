"""CPU tests of the batch pipeline interface (no GPU): the two symbols, the methods and facades, the option that is not enumerated, the
refusals that are decided before the context is looked at, in their documented order, and the bound."""
import ctypes
import os
import re
import subprocess

import numpy as np

import tudocomp_amd as T

ERR_ARG, ERR_NO_SENTINEL, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -3, -4, -6
NAMES = ("tdc_gpu_pipeline_compress_batch", "tdc_gpu_pipeline_batch_bound")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 20
BWTZIP = [T.STAGE_BWT, (T.STAGE_RLE, 0), T.STAGE_MTF, T.STAGE_HUFF]
BYTES3 = [(T.STAGE_RLE, 0), T.STAGE_MTF, T.STAGE_HUFF]


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_methods_and_options():
    lib = T._native.load()
    hdr = open(os.path.join(ROOT, "include", "tdc_gpu.h")).read()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bint tdc_gpu_pipeline_compress_batch\(", hdr) and re.search(r"\bsize_t tdc_gpu_pipeline_batch_bound\(", hdr)
    assert len(lib.tdc_gpu_pipeline_compress_batch.argtypes) == 12 and len(lib.tdc_gpu_pipeline_batch_bound.argtypes) == 4
    for name in ("pipeline_compress_batch", "pipeline_compress_batch_into", "pipeline_batch_bound"):
        assert callable(getattr(T.Context, name))
    assert callable(T.pipeline_batch_bound)
    for facade in (T.ChainCompressor(None, "bwt:rle:mtf:encode(huff)"), T.RunLengthEncoder(None), T.MTFCompressor(None), T.LiteralEncoder(None)):
        assert callable(facade.compress_batch)
    assert "pipe_batch_threads" not in T.option_names()                                      # an option of the context, not enumerated


def call(stages, offsets, null=(), nstages=None):
    """the status of the batch call without a context (NULL): what the arguments alone decide comes first"""
    L = T._native.load()
    arr, k = T._stages(stages)
    off = np.asarray(offsets, dtype=np.uint64)
    count = len(off) - 1
    data, out = np.zeros(64, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    out_off, out_len = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64)
    status = np.zeros(count + 1, dtype=np.int32)
    arg = {"in": ptr(data), "in_off": ptr(off), "out": ptr(out), "out_off": ptr(out_off), "out_len": ptr(out_len), "status": ptr(status)}
    for n in null:
        arg[n] = None
    return L.tdc_gpu_pipeline_compress_batch(None, arr, k if nstages is None else nstages, arg["in"], arg["in_off"], count, arg["out"], 256,
                                             arg["out_off"], arg["out_len"], arg["status"], None)


def test_refusals_that_need_no_device_in_their_order():
    good = [0, 5, 5, 20]
    huge = [0, 1 << 31, 0xFFFFFFFF]                                                          # above 2^32 - 2 in all, by the offsets alone
    bwt_behind = [(T.STAGE_RLE, 0), T.STAGE_BWT]
    sle = [T.STAGE_MTF, (T.STAGE_SLE, 3)]
    nine = [T.STAGE_MTF] * 9
    # 1: NULL pointers and offsets -- before every other reason
    for null in ("in", "in_off", "out_off", "out_len", "status"):
        assert call(BWTZIP, good, null=(null,)) == ERR_ARG, null
        assert call(bwt_behind, huge, null=(null,)) == ERR_ARG, null
    assert call(BWTZIP, [1, 5, 5, 20]) == ERR_ARG                                            # in_off[0] != 0
    assert call(BWTZIP, [0, 5, 4, 20]) == ERR_ARG                                            # a decreasing in_off
    assert call(bwt_behind, [1, 5, 5, 20]) == ERR_ARG and call(sle, [0, 5, 4, 20]) == ERR_ARG
    # 2: the stage list, as the single call judges it
    assert call(bwt_behind, good) == ERR_NO_SENTINEL
    assert call(bwt_behind + [(T.STAGE_SLE, 3)], huge) == ERR_NO_SENTINEL
    assert call([], good) == ERR_ARG and call(BWTZIP, good, nstages=0) == ERR_ARG
    assert call(nine, good) == ERR_ARG and call(nine, huge) == ERR_ARG
    assert call([(T.STAGE_RLE, (1 << 62) + 1)], good) == ERR_ARG and call([7], good) == ERR_ARG
    # 3: encode(sle) has no batch form
    assert call(sle, good) == ERR_UNSUPPORTED and call(sle, huge) == ERR_UNSUPPORTED
    assert call([(T.STAGE_SLE, 3)], [0]) == ERR_UNSUPPORTED
    # 4: the size in all, from offsets with no buffer behind them
    for stages in (BWTZIP, BYTES3, [T.STAGE_MTF]):
        assert call(stages, huge) == ERR_TOO_LARGE
        assert call(stages, [0, 1 << 31, 0xFFFFFFFE]) == ERR_ARG                             # 2^32 - 2 passes: the context is next
    # 5: all is well but the context: NULL
    for stages in (BWTZIP, BYTES3, [T.STAGE_HUFF]):
        assert call(stages, good) == ERR_ARG
        assert call(stages, [0]) == ERR_ARG                                                  # count = 0 needs a context too
        assert call(stages, [0, 0, 0], null=("in",)) == ERR_ARG                              # no bytes need no `in` -- the context again
        assert call(stages, good, null=("out",)) == ERR_ARG                                  # a NULL `out` is the sizes pass, not an argument error


def test_bound():
    lengths = [0, 1, 7, 8, 9, 4096, 65537, CAP]
    for stages in (BWTZIP, BYTES3, [(T.STAGE_RLE, 200)], [T.STAGE_MTF], [T.STAGE_HUFF], [T.STAGE_BWT]):
        want = sum(-(-T.pipeline_bound(stages, n) // 8) * 8 for n in lengths)
        assert want > 0 and T.pipeline_batch_bound(stages, lengths) == want
        assert T.pipeline_batch_bound(stages, lengths + [CAP + 1]) == want                   # a text above the cap contributes 0
        assert T.pipeline_batch_bound(stages, [CAP + 1, 5]) == -(-T.pipeline_bound(stages, 5) // 8) * 8
        assert T.pipeline_batch_bound(stages, []) == 0
    assert T.pipeline_batch_bound([T.STAGE_MTF, (T.STAGE_SLE, 3)], lengths) == 0
    assert T.pipeline_batch_bound([T.STAGE_MTF, T.STAGE_BWT], lengths) == 0 and T.pipeline_batch_bound([], lengths) == 0
    # refused offsets, through the C call (pipeline_batch_bound builds its own ascending ones)
    L = T._native.load()
    arr, k = T._stages(BYTES3)
    for off in ([1, 5, 20], [0, 5, 4], [0, 1 << 31, 0xFFFFFFFF]):
        a = np.asarray(off, dtype=np.uint64)
        assert L.tdc_gpu_pipeline_batch_bound(arr, k, ptr(a), len(a) - 1) == 0
    assert L.tdc_gpu_pipeline_batch_bound(arr, k, None, 0) == 0


def test_cpp_facade_compiles(tmp_path):
    """tdc_amd::ChainCompressor::compress_batch has the signature of the other facades' compress_batch, and the facades built on it
    inherit it; taking the address makes the compiler check the call of the C ABI (no device is needed to compile it)"""
    src = tmp_path / "facade.cpp"
    src.write_text('#include "tdc_amd.hpp"\n'
                   "using tdc_amd::bytes;\n"
                   "typedef void (tdc_amd::ChainCompressor::*batch_fn)(const std::vector<bytes>&, std::vector<bytes>&, std::vector<int32_t>&);\n"
                   "batch_fn chain = &tdc_amd::ChainCompressor::compress_batch;\n"
                   "typedef void (tdc_amd::RePairCompressor::*repair_fn)(const std::vector<bytes>&, std::vector<bytes>&, std::vector<int32_t>&);\n"
                   "repair_fn same = &tdc_amd::RePairCompressor::compress_batch;\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "facade.o"),
                           "-I", os.path.join(ROOT, "tudocomp_amd", "host"), "-I", os.path.join(ROOT, "include")])
