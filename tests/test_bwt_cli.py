"""CPU tests of the bwt interface around the device code: the C ABI exports it, the `tdc` registry lists `bwt`, `tdc -d` inverts a
transform with the facade's host loop (no GPU needed), and chains stay refused."""
import os
import subprocess

import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests.models import bwt as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
NAMES = ("tdc_gpu_bwt_compress", "tdc_gpu_bwt_compress_into", "tdc_gpu_bwt_decompress", "tdc_gpu_bwt_decompress_into",
         "tdc_gpu_bwt_inverse_stage")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def test_symbols_exported():
    lib = T._native.load()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
    for m in ("bwt_compress", "bwt_compress_into", "bwt_decompress", "bwt_decompress_into", "bwt_inverse_stage"):
        assert hasattr(T.Context, m)
    assert hasattr(T.BWTCompressor, "compress") and hasattr(T.BWTCompressor, "decompress")
    assert "bwt_log" in T.option_names()


def test_registry_lists_bwt():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    lines = [ln.split("[")[0].strip() for ln in r.stdout.splitlines()]
    assert "bwt" in lines and "bwt(dec=gpu)" in lines


@pytest.mark.parametrize("header", [b"bwt%", b"bwt(textds=textds(sa=divsufsort))%"])
def test_host_inverse_without_a_gpu(tmp_path, header):
    data = b"\x00\xffab\xff\xfe\x00" * 50 + T.gen_english(5000, 3).tobytes() + bytes(range(256))
    text = T.escape(data)
    assert b"\xff" in text
    f = tmp_path / "p.tdc"
    f.write_bytes(header + M.bwt_from_sa(text, O.suffix_array(text)))
    out = tmp_path / "p.out"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data


def test_chains_stay_refused(tmp_path):
    src = tmp_path / "in.txt"
    src.write_bytes(b"abracadabra")
    r = subprocess.run([TDC, "-a", "bwt:rle:mtf:encode(huff)", "-o", str(tmp_path / "o"), str(src)], capture_output=True, text=True)
    assert r.returncode == 1
    assert not (tmp_path / "o").exists()
