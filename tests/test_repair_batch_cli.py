"""CPU tests of the repair batch interface (no GPU): the three symbols, the facades, the refusals that are decided before the context is
looked at and their order, the bound against its formula and against the model's streams, and that the batches of
tests/repair_batches.py hold what their names promise."""
import ctypes

import numpy as np
import pytest

import tudocomp_amd as T
from tests import repair_batches as B
from tests.models import repair as M

ERR_ARG, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -4, -6
NAMES = ("tdc_gpu_repair_compress_batch", "tdc_gpu_repair_batch_bound", "tdc_gpu_repair_grammar_batch")
TAKEN = tuple(B.CID.values())
ALL_CODERS = (T.CODER_HUFF, T.CODER_GAMMA, T.CODER_ARITH, T.CODER_ASCII, T.CODER_SLE, T.CODER_BIT, T.CODER_DELTA, 99)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_facades():
    lib = T._native.load()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert len(lib.tdc_gpu_repair_compress_batch.argtypes) == 12 and len(lib.tdc_gpu_repair_grammar_batch.argtypes) == 10
    assert lib.tdc_gpu_repair_compress_batch.argtypes[4] is ctypes.c_uint64               # max_rules
    assert lib.tdc_gpu_repair_batch_bound.restype is ctypes.c_size_t
    for name in ("repair_compress_batch", "repair_compress_batch_into", "repair_grammar_batch", "repair_batch_bound"):
        assert hasattr(T.Context, name)
    assert callable(T.repair_batch_bound)
    assert callable(T.RePairCompressor(None, coder="gamma", max_rules=64).compress_batch)
    for name in ("repair_batch_rounds", "repair_batch_table"):                             # options of the context, not enumerated
        assert name not in T.option_names()


LENGTHS = [0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 70001, 1 << 24, (1 << 24) + 1]


def test_bound_is_its_formula():
    for name, coder in B.CID.items():
        assert T.repair_batch_bound(LENGTHS, coder) == sum(B.text_bound(n, name) for n in LENGTHS) > 0
        for n in LENGTHS:
            assert T.repair_batch_bound([n], coder) == B.text_bound(n, name) == (T.repair_bound(n, coder) + 7) // 8 * 8
        assert T.repair_batch_bound([], coder) == 0                                         # no text: no byte


def test_bound_is_zero_where_the_call_refuses():
    f = T._native.load().tdc_gpu_repair_batch_bound
    for coder in ALL_CODERS:
        assert (T.repair_batch_bound([100, 5], coder) > 0) == (coder in TAKEN), coder
    g = T.CODER_GAMMA
    assert f(None, 1, g) == 0
    assert f(ptr(np.array([1, 5], dtype=np.uint64)), 1, g) == 0                             # in_off[0] != 0
    assert f(ptr(np.array([0, 5, 3], dtype=np.uint64)), 2, g) == 0                          # decreasing
    assert f(ptr(np.array([0, 1 << 31, 0xFFFFFFFF], dtype=np.uint64)), 2, g) == 0           # 2^32 - 1 bytes
    assert f(ptr(np.array([0, 1 << 30, 1 << 31], dtype=np.uint64)), 2, g) > 0


def test_bound_holds_the_models_streams():
    rng = np.random.default_rng(20261021)
    texts = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 2, 3, 9, 100, 255, 256, 257, 1000, 3000) for _ in range(2)]
    texts += [b"a" * 3000, b"ab" * 1500, B.tie_text(), B.english(3000, 3), B.dna(2999, 4), B.rnd(3000, 16, 5), bytes(range(256)) * 11]
    for x in texts:
        for name, coder in B.CID.items():
            assert len(M.compress(x, name)) <= T.repair_batch_bound([len(x)], coder), (len(x), name)


def compress_status(in_off, coder=T.CODER_BIT, null=()):
    """the status of a compress batch call without a context (NULL): what the arguments alone decide comes first"""
    L = T._native.load()
    off = np.asarray(in_off, dtype=np.uint64)
    count = len(off) - 1
    text, out = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    out_off, out_len, status = np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.uint64), np.zeros(count + 1, dtype=np.int32)
    arg = {"in": ptr(text), "in_off": ptr(off), "out": ptr(out), "out_off": ptr(out_off), "out_len": ptr(out_len), "status": ptr(status)}
    for name in null:
        arg[name] = None
    return L.tdc_gpu_repair_compress_batch(None, arg["in"], arg["in_off"], count, 0, coder, arg["out"], 64, arg["out_off"], arg["out_len"],
                                           arg["status"], None)


def test_compress_refusals_that_need_no_device():
    good = [0, 5, 5, 20]
    for name in ("in", "in_off", "out", "out_off", "out_len", "status"):
        assert compress_status(good, null=(name,)) == ERR_ARG, name
    assert compress_status([0, 5, 4, 20]) == ERR_ARG                                        # a decreasing in_off
    assert compress_status([1, 5, 5, 20]) == ERR_ARG                                        # in_off[0] != 0
    for coder in ALL_CODERS:
        assert compress_status(good, coder=coder) == (ERR_ARG if coder in TAKEN else ERR_UNSUPPORTED), coder
    # the order: 1 the coder, 2 NULL arguments and bad offsets, 3 the size in all, 4 the NULL context
    assert compress_status([1, 5, 5, 20], coder=T.CODER_HUFF) == ERR_UNSUPPORTED
    assert compress_status(good, coder=T.CODER_HUFF, null=("out",)) == ERR_UNSUPPORTED
    assert compress_status([0, 1 << 31, 0xFFFFFFFF], null=("status",)) == ERR_ARG
    assert compress_status([0, 1 << 31, 0xFFFFFFFF]) == ERR_TOO_LARGE                       # by the offsets alone: nothing is read
    assert compress_status([0, 1 << 31, 0xFFFFFFFE]) == ERR_ARG                             # all is well but the context: NULL
    assert compress_status(good) == ERR_ARG
    assert compress_status([0]) == ERR_ARG                                                  # count = 0 needs a context too


def test_grammar_refusals_that_need_no_device():
    L = T._native.load()
    text, rules, start = np.zeros(64, dtype=np.uint8), np.zeros(64, dtype=np.uint64), np.zeros(64, dtype=np.uint32)
    rule_off, start_off, status = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.int32)

    def call(offsets, null=None):
        off = np.asarray(offsets, dtype=np.uint64)
        a = {"in": ptr(text), "in_off": ptr(off), "rules": ptr(rules), "rule_off": ptr(rule_off), "start": ptr(start),
             "start_off": ptr(start_off), "status": ptr(status)}
        if null:
            a[null] = None
        return L.tdc_gpu_repair_grammar_batch(None, a["in"], a["in_off"], len(off) - 1, 0, a["rules"], a["rule_off"], a["start"],
                                              a["start_off"], a["status"])

    good = [0, 5, 5, 20]
    for name in ("in", "in_off", "rules", "rule_off", "start", "start_off", "status"):
        assert call(good, name) == ERR_ARG, name
    assert call([0, 5, 4, 20]) == ERR_ARG and call([1, 5, 5, 20]) == ERR_ARG
    assert call([0, 1 << 31, 0xFFFFFFFF]) == ERR_TOO_LARGE
    assert call(good) == ERR_ARG                                                            # the NULL context


def test_the_batches_hold_what_they_promise():
    assert B.batch("count0") == () and len(B.batch("count1")) == 1
    assert set(B.batch("only_empties")) == {b""}
    ab = B.batch("no_pair_across")
    assert len(ab) == 50 and all(len(B.host(x)[0]) == 0 for x in ab) and len(B.host(b"".join(ab))[0]) > 0
    assert b"".join(ab).count(b"ab") - 1 == 49                                              # the concatenation repeats (a, b) 49 times
    nxt = B.batch("a_next_to_a")
    assert any(x.endswith(b"a") and y.startswith(b"a") for x, y in zip(nxt, nxt[1:]))
    split = [x for x in B.batch("split_runs") if x != b"ba"]
    assert [len(x) + len(y) for x, y in zip(split[::2], split[1::2])] == list(B.RUNS) and set(b"".join(split)) == {ord("a")}
    assert {1, 2, 69, 70, 255, 256, 257, 1023, 1024, 1025} <= set(B.RUNS)
    same = B.batch("same_at_three_places")
    where = [k for k, x in enumerate(same) if x == same[0]]
    assert len(where) == 3 and len({(same[k - 1], same[k + 1]) for k in where[1:]}) == 2 and where[0] == 0
    small = B.batch("smallest")
    assert [len(x) for x in small[1::2]] == [0, 1, 2, 3, 0, 1, 2, 3, 2, 3] and min(len(x) for x in small[::2]) >= 400
    lens = {len(x) for x in B.batch("forks")}
    assert {B.WORKGROUP - 1, B.WORKGROUP, B.WORKGROUP + 1, B.CHUNK - 1, B.CHUNK, B.CHUNK + 1, 2 * B.CHUNK - 1, 2 * B.CHUNK, 2 * B.CHUNK + 1} <= lens
    squares = [x for x in B.batch("forks") if len(B.host(x)[0]) and int(B.host(x)[0][0]) == (97 << 32 | 97)]
    assert len(squares) >= 20                                                               # rule 0 is (a, a): the chunked mark runs
    assert {x.index(b"aa") % 2 for x in squares} == {0, 1}                                  # runs from even and odd positions
    las = B.batch("long_among_short")
    assert len(las) == 201 and sorted(len(x) for x in las)[-2:][1] == 70001 and sorted(len(x) for x in las)[-2] < 400
    assert las[77] == max(las, key=len)
    r300 = B.batch("random300")
    assert len(r300) == 300 and max(len(x) for x in r300) <= 3000 and min(len(x) for x in r300) < 20
    assert len(set(r300[1])) <= 4 and len(set(r300[2])) <= 16 and len(set(r300[0])) > 16    # english, dna, 16 symbols
    for x, rules, start in B.kat_cases():                                                   # the host loop on the hand-derived cases
        assert B.as_model(*B.host(x)) == ([tuple(r) for r in rules], list(start))
    known = B.batch("known")
    assert B.tie_text() in known and b"a" * 65536 in known and b"ab" * 4097 + b"a" in known
    for mr in (1, 64, 512):                                                                 # texts that need fewer rules than the cap
        counts = [len(B.host(x, mr)[0]) for x in B.batch("capped")]
        assert max(counts) == mr and 0 in counts
        assert any(0 < c < mr for c in counts) or mr == 1
    for name in B.NAMES:                                                                    # every stream decodes, on the host
        for x in B.batch(name)[:8]:
            if len(x) <= 5000:
                for coder, cid in B.CID.items():
                    assert T.repair_decode(B.stream(x, coder), cid) == x


def test_cpp_facade_compiles(tmp_path):
    """tdc_amd::RePairCompressor::compress_batch adapts the batch call, whose max_rules the lz batches lack, to lz_compress_batch: taking
    its address makes the compiler instantiate that adapter (no device is needed to compile it)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "facade.cpp"
    src.write_text('#include "tdc_amd.hpp"\n'
                   "using tdc_amd::bytes;\n"
                   "void (tdc_amd::RePairCompressor::*batch)(const std::vector<bytes>&, std::vector<bytes>&, std::vector<int32_t>&) =\n"
                   "    &tdc_amd::RePairCompressor::compress_batch;\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-o", str(tmp_path / "facade.o"),
                           "-I", os.path.join(root, "tudocomp_amd", "host"), "-I", os.path.join(root, "include")])
