"""GPU tests of repair (tdc_gpu_repair_grammar, tdc_gpu_repair_compress{,_into}; repair.hip and the shared field coder, field_coder.hpp): the
device grammar -- rules and start sequence, exactly -- against the host loop tdc_repair_grammar (which tests/test_repair_cli.py holds
against the model), the device streams byte for byte against the model's coders (tests/models/repair.py), every stream back through
tdc_repair_decode.  Every case runs twice: with the digram table kept up to date by the rounds' deltas, and with option
repair_recount = 1, which recounts it in every round."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests.coder_borders import repair_borders
from tests.models import repair as M
from tests.util import load_json

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CID = {"ascii": T.CODER_ASCII, "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}


@pytest.fixture(scope="module", params=["deltas", "recount"])
def dev(request):
    with T.Context(0) as ctx:
        if request.param == "recount":
            ctx.set_option("repair_recount", 1)
        yield ctx


@functools.lru_cache(maxsize=None)
def host(data, max_rules=0):
    """the specification, computed once per case: (rules, start) of tdc_repair_grammar"""
    r, s = T.repair_grammar(data, max_rules)
    r.setflags(write=False)
    s.setflags(write=False)
    return r, s


def as_model(rules, start):
    return [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in rules], [int(x) for x in start]


def check(ctx, data, max_rules=0):
    want_r, want_s = host(data, max_rules)
    r, s, st = ctx.repair_grammar(data, max_rules)
    assert np.array_equal(r, want_r) and np.array_equal(s, want_s), (len(data), data[:24], max_rules)
    assert st["rules"] == len(r) and st["replaced"] == len(data) - len(s) and st["n"] == len(data)
    if max_rules:
        assert len(r) <= max_rules
    return st


@functools.lru_cache(maxsize=None)
def english(n):
    return T.gen_english(n, 42).tobytes()


@functools.lru_cache(maxsize=None)
def dna(n):
    return T.gen_dna(n, 7).tobytes()


@functools.lru_cache(maxsize=None)
def binary16k():
    rng = np.random.default_rng(3)
    block = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    return (block + b"\x00\xff" * 700 + block[::-1] + b"\x00" * 333 + block + b"\xff" * 555 + english(6000))[:16384]


@functools.lru_cache(maxsize=None)
def tie_text():
    """every two-letter word over 16 letters, twice, shuffled: hundreds of pairs that count the same"""
    letters = b"abcdefghijklmnop"
    words = [bytes((x, y)) for x in letters for y in letters] * 2
    order = np.random.default_rng(16).permutation(len(words))
    return b"".join(words[i] for i in order)


RUNS = list(range(1, 71)) + [255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537]


def test_runs(dev):
    for k in RUNS:
        st = check(dev, b"a" * k)
        assert st["tie_rounds"] == 0
    r, s, _ = dev.repair_grammar(b"aaa")
    assert as_model(r, s) == ([(97, 97)], [256, 97])                # left-greedy: the count was 2, one pair goes


def test_runs_inside_a_text(dev):
    for k in (2, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049):
        check(dev, b"xy" * 3 + b"a" * k + b"yx" * 3 + b"a" * (k + 1) + b"b")


def test_hand_derived_grammars(dev):
    for c in load_json("repair_kats.json")["cases"]:
        r, s, _ = dev.repair_grammar(c["text"].encode())
        assert as_model(r, s) == ([tuple(x) for x in c["rules"]], c["start"]), c["text"]
        check(dev, c["text"].encode())


def test_ties(dev):
    st = check(dev, tie_text())
    assert st["tie_rounds"] > 0
    for mr in (1, 2, 7):
        check(dev, tie_text(), mr)
    check(dev, tie_text() + tie_text()[::-1])


def test_adjacent_pairs(dev):
    for k in (1, 2, 3, 4, 5, 6, 7, 100, 1000, 4097):
        check(dev, b"ab" * k)
        check(dev, b"ab" * k + b"a")
        check(dev, b"b" + b"ab" * k)


@pytest.mark.parametrize("name", ["english", "dna", "binary"])
def test_full_grammars(dev, name):
    data = {"english": lambda: english(64 << 10), "dna": lambda: dna(64 << 10), "binary": binary16k}[name]()
    if name == "binary":
        assert len(data) == 16384 and 0 in data and 255 in data
    st = check(dev, data)
    assert st["rules"] > 100 and st["tie_rounds"] > 0
    print("%s: %d rules, %d replaced, %d tie rounds, %d rebuilds, %.1f ms" % (name, st["rules"], st["replaced"], st["tie_rounds"],
                                                                             st["rebuilds"], st["ms_factorize"]))


@pytest.mark.parametrize("max_rules", [1, 64, 512])
def test_capped(dev, max_rules):
    st = check(dev, english(1 << 20), max_rules)
    assert st["rules"] == max_rules


def test_small_table_is_rebuilt():
    data = english(64 << 10)
    with T.Context(0) as ctx:
        ctx.set_option("repair_table_bits", 8)
        st = check(ctx, data)
        assert st["rebuilds"] > 0
        st = check(ctx, tie_text())
        assert st["tie_rounds"] > 0


@pytest.mark.parametrize("coder", M.CODERS)
def test_compress(dev, coder):
    cases = ((english(64 << 10), 0), (english(64 << 10), 100), (binary16k(), 0), (b"a" * 1000, 0), (tie_text(), 0))
    # and field counts on the tile borders of the coder (tests/coder_borders.py; the counts are asserted in tests/test_repair_model.py)
    for data, mr in cases + tuple((t, mr) for t, mr, _ in repair_borders()):
        want = M.encode(*as_model(*host(data, mr)), coder)
        got, st = dev.repair_compress(data, mr, CID[coder])
        assert got == want, (len(data), mr, coder)
        assert T.repair_decode(got, CID[coder]) == data
        assert dev.repair_decompress(got, CID[coder]) == data
        bound = T.repair_bound(len(data), CID[coder])
        assert 0 < len(got) <= bound
        assert st["out_len"] == len(got) and st["rules"] == len(host(data, mr)[0]) and st["n"] == len(data)
        out = np.full(bound, 0xA5, dtype=np.uint8)
        n, _ = dev.repair_compress_into(data, len(data), out, mr, CID[coder])
        assert out[:n].tobytes() == want and (out[n:] == 0xA5).all()


@pytest.mark.parametrize("coder", M.CODERS)
def test_smallest_inputs(dev, coder):
    for data in (b"", b"q", b"qq", b"qr", b"\x00", b"\xff\xff"):
        want = M.encode(*M.grammar(data), coder)
        got, st = dev.repair_compress(data, 0, CID[coder])
        assert got == want and T.repair_decode(got, CID[coder]) == data
        assert st["rules"] == 0 and st["replaced"] == 0
        r, s, _ = dev.repair_grammar(data)
        assert len(r) == 0 and s.tolist() == list(data)
        assert len(got) <= T.repair_bound(len(data), CID[coder])


def test_into_and_the_short_buffer(dev):
    data = english(20000)
    want, _ = dev.repair_compress(data, 0, T.CODER_GAMMA)
    short = np.full(len(want) - 1, 0xA5, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        dev.repair_compress_into(data, len(data), short, 0, T.CODER_GAMMA)
    assert e.value.status == ERR_OOM and e.value.required == len(want) and (short == 0xA5).all()
    back = np.full(len(data) - 1, 0xA5, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        dev.repair_decompress_into(want, back, T.CODER_GAMMA)
    assert e.value.status == ERR_OOM and e.value.required == len(data) and (back == 0xA5).all()
    back = np.zeros(len(data) + 5, dtype=np.uint8)
    assert dev.repair_decompress_into(want, back, T.CODER_GAMMA) == len(data) and back[:len(data)].tobytes() == data
    check(dev, data)                                                # a valid call after the refusals


def test_refused_arguments(dev):
    data = b"abcabcabc"
    for coder in (T.CODER_HUFF, T.CODER_ARITH, T.CODER_SLE, 99):
        with pytest.raises(T.TdcGpuError) as e:
            dev.repair_compress(data, 0, coder)
        assert e.value.status == ERR_UNSUPPORTED
        assert T.repair_bound(100, coder) == 0
        check(dev, data)
    L = T._native.load()
    n = ctypes.c_size_t()
    a = np.frombuffer(data, dtype=np.uint8)
    assert L.tdc_gpu_repair_compress(dev._h, a.ctypes.data, len(a), 0, T.CODER_BIT, None, ctypes.byref(n), None) == ERR_ARG
    assert L.tdc_gpu_repair_compress(dev._h, None, 5, 0, T.CODER_BIT, None, ctypes.byref(n), None) == ERR_ARG
    assert L.tdc_gpu_repair_grammar(dev._h, a.ctypes.data, len(a), 0, None, None, None, None, None) == ERR_ARG
    assert L.tdc_gpu_repair_grammar(dev._h, a.ctypes.data, (1 << 30) + 1, 0, None, None, None, None, None) == ERR_TOO_LARGE
    assert T.repair_bound((1 << 30) + 1, T.CODER_BIT) == 0
    check(dev, data)


def test_facade_and_command_line(dev, tmp_path):
    data = english(30000) + b"\x00\xff" + b"a" * 300
    z = T.RePairCompressor(dev, coder="ascii", max_rules=50)
    s = z.compress(data)
    assert s == M.encode(*as_model(*host(data, 50)), "ascii") and z.decompress(s) == data and z.last_stats["rules"] == 50
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    src = tmp_path / "in.txt"
    src.write_bytes(data)
    for algo, mr, coder in (("repair", 0, "bit"), ("repair(coder=gamma,max_rules=1000)", 1000, "gamma")):
        packed, back = tmp_path / "p.tdc", tmp_path / "p.out"
        r = subprocess.run([TDC, "-a", algo, "-f", "-o", str(packed), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert packed.read_bytes() == algo.encode() + b"%" + M.encode(*as_model(*host(data, mr)), coder)
        r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(packed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data
