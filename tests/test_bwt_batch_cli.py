"""CPU tests of the bwt batch interface (no GPU): the three symbols, the methods and facades, the two options that are not enumerated,
and the refusals that are decided before the context is looked at, in their order."""
import ctypes
import os
import re
import subprocess

import numpy as np

import tudocomp_amd as T

ERR_ARG, ERR_TOO_LARGE = -2, -4
NAMES = ("tdc_gpu_bwt_compress_batch", "tdc_gpu_bwt_decompress_batch", "tdc_gpu_suffix_array_batch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_methods_and_options():
    lib = T._native.load()
    hdr = open(os.path.join(ROOT, "include", "tdc_gpu.h")).read()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, hdr)
    assert len(lib.tdc_gpu_bwt_compress_batch.argtypes) == len(lib.tdc_gpu_bwt_decompress_batch.argtypes) == 8
    assert len(lib.tdc_gpu_suffix_array_batch.argtypes) == 6
    assert re.search(r"#define BWT_BATCH_TEXT_CAP \(\(size_t\)1 << 20\)", hdr)
    for name in ("bwt_compress_batch", "bwt_compress_batch_into", "bwt_decompress_batch", "bwt_decompress_batch_into", "suffix_array_batch"):
        assert callable(getattr(T.Context, name))
    facade = T.BWTCompressor(None)
    assert callable(facade.compress_batch) and callable(facade.decompress_batch)
    for name in ("bwt_batch_sample", "bwt_batch_steps"):                                    # options of the context, not enumerated
        assert name not in T.option_names()


def call(name, offsets, null=(), overlap=False):
    """the status of a batch call without a context (NULL): what the arguments alone decide comes first"""
    L = T._native.load()
    off = np.asarray(offsets, dtype=np.uint64)
    count = len(off) - 1
    data, out = np.zeros(64, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    status = np.zeros(count + 1, dtype=np.int32)
    arg = {"in": ptr(data), "off": ptr(off), "out": ptr(data[8:]) if overlap else ptr(out), "status": ptr(status)}
    for n in null:
        arg[n] = None
    if name == "tdc_gpu_suffix_array_batch":
        return L.tdc_gpu_suffix_array_batch(None, arg["in"], arg["off"], count, arg["out"], arg["status"])
    return getattr(L, name)(None, arg["in"], arg["off"], count, arg["out"], 256, arg["status"], None)


def test_refusals_that_need_no_device():
    good = [0, 5, 5, 20]
    for name in NAMES:
        for null in ("in", "off", "status"):
            assert call(name, good, null=(null,)) == ERR_ARG, (name, null)
        assert call(name, [0, 5, 4, 20]) == ERR_ARG                                         # a decreasing off
        assert call(name, [1, 5, 5, 20]) == ERR_ARG                                         # off[0] != 0
        assert call(name, good, overlap=True) == ERR_ARG                                    # out inside in
        assert call(name, good) == ERR_ARG                                                  # all is well but the context: NULL
        assert call(name, [0]) == ERR_ARG                                                   # count = 0 needs a context too
        assert call(name, [0, 0, 0], null=("in",)) == ERR_ARG                               # no bytes need no `in` -- the context again
    # the order: 1 NULL arguments and bad offsets, 2 the size in all (by the offsets alone: nothing is read), 3 the NULL context
    for name in NAMES[::2]:                                                                 # forward: 2^32 - 2 bytes in all at the most
        assert call(name, [0, 1 << 31, 0xFFFFFFFF], null=("status",)) == ERR_ARG
        assert call(name, [0, 1 << 31, 0xFFFFFFFF]) == ERR_TOO_LARGE
        assert call(name, [0, 1 << 31, 0xFFFFFFFE]) == ERR_ARG
    inv = "tdc_gpu_bwt_decompress_batch"                                                    # inverse: below 2^31 - 1
    assert call(inv, [0, 1 << 30, 0x7FFFFFFF], null=("status",)) == ERR_ARG
    assert call(inv, [0, 1 << 30, 0x7FFFFFFF]) == ERR_TOO_LARGE
    assert call(inv, [0, 1 << 30, 0x7FFFFFFE]) == ERR_ARG
    assert call(inv, [3, 1 << 30, 0x7FFFFFFF]) == ERR_ARG                                   # a bad offset comes before the size


def test_cpp_facade_compiles(tmp_path):
    """tdc_amd::BWTCompressor::compress_batch / decompress_batch have the signature of the RePairCompressor ones; taking their addresses
    makes the compiler instantiate the shared call (no device is needed to compile it)"""
    src = tmp_path / "facade.cpp"
    src.write_text('#include "tdc_amd.hpp"\n'
                   "using tdc_amd::bytes;\n"
                   "typedef void (tdc_amd::BWTCompressor::*batch_fn)(const std::vector<bytes>&, std::vector<bytes>&, std::vector<int32_t>&);\n"
                   "batch_fn fwd = &tdc_amd::BWTCompressor::compress_batch, inv = &tdc_amd::BWTCompressor::decompress_batch;\n"
                   "typedef void (tdc_amd::RePairCompressor::*repair_fn)(const std::vector<bytes>&, std::vector<bytes>&, std::vector<int32_t>&);\n"
                   "repair_fn same = &tdc_amd::RePairCompressor::compress_batch;\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "facade.o"),
                           "-I", os.path.join(ROOT, "tudocomp_amd", "host"), "-I", os.path.join(ROOT, "include")])
