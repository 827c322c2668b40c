"""CPU tests of the interface of the repair device decoder (no GPU): the exported symbols and the Context methods, the entry points
without a context, the `tdc` registry line, the facade, which keeps the host loop for dec="host", and the damaged streams of the GPU
test, none of which announces a large text."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests import repair_damage as D
from tests.models import repair as M
from tests.models.lzss_coders import Malformed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
ERR_ARG = -2


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def test_symbols_and_context_methods():
    lib = T._native.load()
    for name in ("tdc_gpu_repair_decompress", "tdc_gpu_repair_decompress_into", "tdc_gpu_repair_decompress_stats"):
        assert name in T.SYMBOLS and hasattr(lib, name)
    for name in ("repair_decompress", "repair_decompress_into", "repair_decompress_stats", "repair_decompress_stats_into"):
        assert hasattr(T.Context, name)
    assert "len_rounds" in dict(T._native.Stats._fields_)        # the field reserved0 has a name; the struct keeps its size
    assert ctypes.sizeof(T._native.Stats) == 376 and T._native.Stats.len_rounds.offset == 332 and T._native.Stats.rules.offset == 336


def test_null_context_is_refused():
    lib = T._native.load()
    s = np.frombuffer(M.encode([(97, 98)], [M.SIGMA], "bit"), dtype=np.uint8)
    sp = s.ctypes.data_as(ctypes.c_void_p)
    out, n, buf = ctypes.c_void_p(), ctypes.c_size_t(), np.zeros(8, dtype=np.uint8)
    bp = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.tdc_gpu_repair_decompress(None, sp, s.size, T.CODER_BIT, ctypes.byref(out), ctypes.byref(n)) == ERR_ARG
    assert lib.tdc_gpu_repair_decompress_into(None, sp, s.size, T.CODER_BIT, bp, buf.size, ctypes.byref(n)) == ERR_ARG
    assert lib.tdc_gpu_repair_decompress_stats(None, sp, s.size, T.CODER_BIT, bp, buf.size, ctypes.byref(n), None) == ERR_ARG
    assert not buf.any()


def test_registry_lists_the_device_decoder():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "repair(coder=bit | gamma | delta, dec=gpu)" in r.stdout
    assert "repair(coder=bit | ascii | gamma | delta, max_rules=0)" in r.stdout


def test_facade_keeps_the_host_loop():
    data = b"tobeornottobeortobeornot" * 40
    for coder in M.CODERS:
        s = M.compress(data, coder)
        assert T.RePairCompressor(None, coder).decompress(s) == data                         # the default
        assert T.RePairCompressor(None, coder, dec="host").decompress(s) == data
    with pytest.raises(RuntimeError, match="dec=gpu needs a context"):
        T.RePairCompressor(None, "bit", dec="gpu").decompress(M.encode([], [97], "bit"))
    with pytest.raises(RuntimeError, match="repair: dec must be host or gpu"):
        T.RePairCompressor(None, "bit", dec="scan")


def test_tdc_decodes_a_dec_gpu_header_of_coder_host(tmp_path):
    """the header is written as given, and `dec=host` in it needs no device"""
    src, packed, back = tmp_path / "in", tmp_path / "p.tdc", tmp_path / "p.out"
    data = b"abracadabra" * 50
    packed.write_bytes(b"repair(coder=gamma,dec=host)%" + M.compress(data, "gamma"))
    r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(packed)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == data


@pytest.mark.parametrize("coder", D.CODERS)
def test_damaged_streams_stay_small(coder):
    ok = 0
    for name, s in D.damaged_streams(coder):
        try:
            rules, start = M.parse(s, coder)
        except Malformed:
            continue
        ln = M.expansion_lengths(rules)
        assert sum(1 if x < M.SIGMA else ln[x - M.SIGMA] for x in start) <= 1 << 21, name
        ok += 1
    assert ok >= 3 and len(D.damaged_streams(coder)) > 1000
    for name, s, data in D.good_streams(coder):
        assert T.repair_decode(s, {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}[coder]) == data
