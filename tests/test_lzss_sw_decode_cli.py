"""CPU tests of the interface of the lzss device decoder (no GPU): the exported symbols and the Context methods, the `tdc` registry line,
and the facade, which keeps the host loop for dec="host"."""
import os
import subprocess

import pytest

import tudocomp_amd as T
from tests.models import lzss_sw as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def test_symbols_and_context_methods():
    lib = T._native.load()
    for name in ("tdc_gpu_lzss_sw_decompress", "tdc_gpu_lzss_sw_decompress_into"):
        assert name in T.SYMBOLS and hasattr(lib, name)
    for name in ("lzss_sw_decompress", "lzss_sw_decompress_into"):
        assert hasattr(T.Context, name)


def test_registry_lists_the_device_decoder():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "lzss(coder=bit | gamma | delta, dec=gpu)" in r.stdout
    assert "lzss(coder=bit | ascii | gamma | delta, window=16, threshold=3)" in r.stdout


def test_facade_keeps_the_host_loop():
    data = b"tobeornottobeortobeornot" * 40
    for coder in M.CODERS:
        s = M.encode(M.parse(data, 64, 2), coder, 64)
        assert T.LZSSSlidingWindowCompressor(None, coder=coder, window=64, threshold=2).decompress(s) == data     # the default
        assert T.LZSSSlidingWindowCompressor(None, coder=coder, window=64, threshold=2, dec="host").decompress(s) == data
    with pytest.raises(RuntimeError, match="dec=gpu needs a context"):
        T.LZSSSlidingWindowCompressor(None, coder="bit", dec="gpu").decompress(M.encode([(0, None, 97)], "bit", 16))
    with pytest.raises(RuntimeError, match="dec"):
        T.LZSSSlidingWindowCompressor(None, coder="bit", dec="scan")
