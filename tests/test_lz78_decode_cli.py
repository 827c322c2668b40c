"""CPU tests of the lz78 decode interface around the device decoder: the C ABI exports it, the `tdc` registry lists and accepts
lz78(coder=gamma,dec=gpu), and without dec=gpu `tdc -d` keeps the host loop (no GPU needed)."""
import os
import subprocess

import pytest

import tudocomp_amd as T
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def test_symbols_exported():
    lib = T._native.load()
    for name in ("tdc_gpu_lz78_decompress", "tdc_gpu_lz78_decompress_into"):
        assert name in T.SYMBOLS and hasattr(lib, name)
    assert hasattr(T.Context, "lz78_decompress") and hasattr(T.Context, "lz78_decompress_into")
    assert hasattr(T.LZ78Compressor, "decompress")


def test_registry_lists_dec_gpu():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0 and "lz78(coder=gamma, dec=gpu)" in r.stdout


def test_plain_header_keeps_the_host_loop(tmp_path):
    data = T.gen_english(20000, 21).tobytes()
    f = tmp_path / "p.tdc"
    f.write_bytes(b"lz78(coder=gamma)%" + O.lz78_gamma_compress(data))
    out = tmp_path / "p.out"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data
