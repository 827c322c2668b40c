"""CPU tests of the lzss_lcp coder interface: the C ABI exports it, the `tdc` registry lists the coders and refuses the others, and
`tdc -d` decodes model-made files through the host loop (no GPU needed) under every spelling of the header."""
import os
import subprocess

import pytest

import tudocomp_amd as T
from tests import lzss_damage as D
from tests.models import lzss_coders as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def test_symbols_exported():
    lib = T._native.load()
    for name in ("tdc_gpu_lzss_lcp_compress", "tdc_gpu_lzss_lcp_compress_into", "tdc_gpu_lzss_lcp_bound", "tdc_gpu_lzss_lcp_decompress",
                 "tdc_gpu_lzss_lcp_decompress_into", "tdc_lzss_decode"):
        assert name in T.SYMBOLS and hasattr(lib, name)
    for name in ("lzss_lcp_compress", "lzss_lcp_compress_into", "lzss_lcp_decompress", "lzss_lcp_decompress_into", "lzss_lcp_bound"):
        assert hasattr(T.Context, name)
    assert T.CODER_DELTA == 6 and T.CODER_BIT == 5
    n = 1000
    assert T.lzss_lcp_bound(n, T.CODER_BIT) >= 8 * n and T.lzss_lcp_bound(n, T.CODER_GAMMA) >= 9 * n
    assert T.lzss_lcp_bound(n, T.CODER_DELTA) >= 6 * n and T.lzss_lcp_bound(n, T.CODER_ASCII) >= 24 * n
    assert T.lzss_lcp_bound(n, T.CODER_SLE) == 0 and T.lzss_lcp_bound(n, T.CODER_ARITH) == 0


def test_registry_lists_the_coders():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    for name in ("lzss_lcp(coder=huff, threshold=3)", "lzss_lcp(coder=bit | gamma | delta | ascii, threshold=3)",
                 "lzss_lcp(coder=huff | bit | gamma | delta, dec=gpu)"):
        assert name in r.stdout


@pytest.mark.parametrize("header,coder", [("lzss_lcp(coder=bit)", "bit"), ("lzss_lcp(bit)", "bit"), ("lzss_lcp(coder=delta,threshold=5)", "delta"),
                                          ("lzss_lcp(coder=gamma)", "gamma"), ("lzss_lcp(gamma, textds, 3)", "gamma")])
def test_tdc_d_decodes_model_files_on_the_host(tmp_path, header, coder):
    data = D.TEXT[:-1]
    f = tmp_path / "p.tdc"
    f.write_bytes(header.encode() + b"%" + M.encode(D.TEXT, D.factors(), coder))
    out = tmp_path / "p.out"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data


@pytest.mark.parametrize("coder", M.CODERS)
def test_tdc_d_refuses_a_damaged_stream(tmp_path, coder):
    name, s = D.damaged_streams(coder)[-2]
    assert name == "src+len>n"
    f = tmp_path / "bad.tdc"
    f.write_bytes(("lzss_lcp(coder=%s)%%" % coder).encode() + s)
    out = tmp_path / "bad.out"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and "corrupt stream" in r.stderr and not out.exists()


@pytest.mark.parametrize("algo", ["lzss_lcp(coder=sle)", "lzss_lcp(coder=arithmetic)", "lzss_lcp(coder=nosuch)", "lzss_lcp"])
def test_other_coders_are_refused(tmp_path, algo):
    f = tmp_path / "in.txt"
    f.write_bytes(b"abc")
    r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "o.tdc"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and "No implementation found" in r.stderr
    if "=" in algo:
        with pytest.raises(RuntimeError, match="No implementation found"):
            T.LZSSLCPCompressor(None, coder=algo[15:-1])


def test_facade_host_loop():
    for coder in M.CODERS:
        z = T.LZSSLCPCompressor(None, coder=coder, threshold=5)
        assert z.decompress(M.encode(D.TEXT, D.factors(), coder)) == D.TEXT[:-1]
    with pytest.raises(RuntimeError, match="dec must be"):
        T.LZSSLCPCompressor(None, dec="scan")
