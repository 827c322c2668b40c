"""CPU tests of the interface around rle, mtf and encode(huff): the C ABI exports and the Python binding, the `tdc` registry, and
`tdc -d` on streams the model / the oracle made (host decoders, no GPU needed).  Chains stay off the command line."""
import os
import subprocess

import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests.models import bwtzip as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
NAMES = ("tdc_gpu_pipeline_bound", "tdc_gpu_pipeline_compress", "tdc_gpu_pipeline_compress_into", "tdc_gpu_pipeline_decompress",
         "tdc_gpu_pipeline_decompress_into", "tdc_rle_decode", "tdc_mtf_decode", "tdc_huff_decode_literals")


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def test_symbols_exported_and_bound():
    lib = T._native.load()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
    for m in ("pipeline_compress", "pipeline_compress_into", "pipeline_decompress", "pipeline_decompress_into"):
        assert hasattr(T.Context, m)
    for cls in (T.RunLengthEncoder, T.MTFCompressor, T.LiteralEncoder, T.ChainCompressor):
        assert hasattr(cls, "compress") and hasattr(cls, "decompress")
    assert (T.STAGE_BWT, T.STAGE_RLE, T.STAGE_MTF, T.STAGE_HUFF) == (0, 1, 2, 3)
    assert "pipe_log" in T.option_names()


def test_pipeline_bound_and_chain_parser():
    assert T.pipeline_bound([T.STAGE_MTF], 1000) == 1000
    assert T.pipeline_bound([(T.STAGE_RLE, 0)], 1000) == 1999 and T.pipeline_bound([(T.STAGE_RLE, 200)], 1000) == 2998
    assert T.pipeline_bound([T.STAGE_BWT, (T.STAGE_RLE, 0), T.STAGE_MTF, T.STAGE_HUFF], 1000) >= 1999
    for bad in ([], [T.STAGE_MTF] * 9, [9], [T.STAGE_MTF, T.STAGE_BWT]):
        assert T.pipeline_bound(bad, 1000) == 0
    assert T.pipeline_bound([(T.STAGE_RLE, 0)], (1 << 32) - 2) == 0          # the worst case passes 2^32 - 2 bytes
    assert T.parse_chain("bwt:rle:mtf:encode(huff)") == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert T.parse_chain("rle(offset=7):mtf") == [(1, 7), (2, 0)]
    with pytest.raises(RuntimeError):
        T.parse_chain("bwt:lz4")


def test_registry_lists_the_three_and_no_chain():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    names = [ln.split("[")[0].strip() for ln in r.stdout.splitlines()[1:]]
    for want in ("rle", "rle(offset=0)", "mtf", "encode(huff)"):
        assert want in names
    assert not [n for n in names if ":" in n]


DATA = b"\x00\xffab\xff\xfe\x00" * 50 + T.gen_english(5000, 3).tobytes() + bytes(range(256)) * 3 + b"a" * 300 + b"\x80" * 7 + b"\xff\xff"


@pytest.mark.parametrize("algo,payload", [("rle", M.rle_encode(DATA)), ("rle(offset=3)", M.rle_encode(DATA, 3)), ("mtf", M.mtf_encode(DATA)),
                                          ("encode(huff)", O.huff_encode_literals(DATA))], ids=["rle", "rle-offset", "mtf", "huff"])
def test_host_decoders_without_a_gpu(tmp_path, algo, payload):
    f, out = tmp_path / "p.tdc", tmp_path / "p.out"
    f.write_bytes(algo.encode() + b"%" + payload)
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == DATA


def test_malformed_streams_and_chains_are_refused(tmp_path):
    f = tmp_path / "p.tdc"
    for blob in (b"rle%aa", b"encode(huff)%", b"rle:mtf%abc", b"encode(huff):mtf%abc"):
        f.write_bytes(blob)
        r = subprocess.run([TDC, "-d", "-o", str(tmp_path / "o"), str(f)], capture_output=True, text=True)
        assert r.returncode == 1 and not (tmp_path / "o").exists(), blob
    src = tmp_path / "in.txt"
    src.write_bytes(b"abracadabra")
    for algo in ("rle:mtf", "encode(huff):mtf", "bwt:rle:mtf:encode(huff)"):
        r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "o"), str(src)], capture_output=True, text=True)
        assert r.returncode == 1 and not (tmp_path / "o").exists(), algo
