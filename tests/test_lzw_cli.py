"""CPU tests of the lzw interface: the C ABI exports it, the `tdc` registry lists and accepts lzw(coder=bit | gamma), refuses other
coders and dictionary limits, and `tdc -d` decodes model-made files through the host loop (no GPU needed)."""
import os
import subprocess

import pytest

import tudocomp_amd as T
from tests.models import lzw as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def test_symbols_exported():
    lib = T._native.load()
    for name in ("tdc_gpu_lzw_compress", "tdc_gpu_lzw_decompress", "tdc_gpu_lzw_decompress_into", "tdc_lzw_factors", "tdc_lzw_decode"):
        assert name in T.SYMBOLS and hasattr(lib, name)
    for name in ("lzw_compress", "lzw_decompress", "lzw_decompress_into"):
        assert hasattr(T.Context, name)
    assert T.CODER_BIT == 5


def test_registry_lists_lzw():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    for name in ("lzw(coder=bit)", "lzw(coder=gamma)", "lzw(coder=bit, dec=gpu)", "lzw(coder=gamma, dec=gpu)"):
        assert name in r.stdout


@pytest.mark.parametrize("header,coder", [("lzw(coder=bit)", "bit"), ("lzw(coder=gamma)", "gamma"), ("lzw", "bit"),
                                          ("lzw(coder=bit,lz78trie=ternary)", "bit"), ("lzw(gamma, binary)", "gamma")])
def test_tdc_d_decodes_model_files_on_the_host(tmp_path, header, coder):
    data = T.gen_english(20000, 21).tobytes() + b"\x00\xff" + b"a" * 300
    f = tmp_path / "p.tdc"
    f.write_bytes(header.encode() + b"%" + M.compress(data, coder))
    out = tmp_path / "p.out"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data


def test_tdc_d_refuses_a_bad_code(tmp_path):
    f = tmp_path / "bad.tdc"
    f.write_bytes(b"lzw(coder=bit)%" + M.encode([97, 300], "bit"))
    r = subprocess.run([TDC, "-d", "-o", str(tmp_path / "bad.out"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and "invalid compressed code" in r.stderr


@pytest.mark.parametrize("algo", ["lzw(coder=huff)", "lzw(coder=delta)", "lzw(coder=ascii)"])
def test_other_coders_are_refused(tmp_path, algo):
    f = tmp_path / "in.txt"
    f.write_bytes(b"abc")
    r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "o.tdc"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and "No implementation found" in r.stderr
    with pytest.raises(RuntimeError, match="No implementation found"):
        T.LZWCompressor(None, coder=algo[10:-1])


def test_dict_size_is_refused_by_name(tmp_path):
    f = tmp_path / "in.txt"
    f.write_bytes(b"abc")
    r = subprocess.run([TDC, "-a", "lzw(dict_size=4096)", "-o", str(tmp_path / "o.tdc"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and "dict_size" in r.stderr
    with pytest.raises(RuntimeError, match="dict_size"):
        T.LZWCompressor(None, dict_size=4096)
    T.LZWCompressor(None, dict_size=0)


def test_facade_host_loop():
    data = b"tobeornottobeortobeornot" * 40
    for coder in ("bit", "gamma"):
        assert T.LZWCompressor(None, coder=coder).decompress(M.compress(data, coder)) == data
