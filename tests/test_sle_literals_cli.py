"""CPU tests of the interface around encode(sle): the host loop tdc_sle_decode against the model on good and on
damaged streams, the Python binding and the chain parser, the `tdc` registry, and `tdc -d` on files the model wrote (no GPU needed)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests.models import sle_literals as M
from tests.models.sle_decode import BitWriter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
KMERS = (1, 2, 3, 4, 7)


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def texts():
    rng = np.random.default_rng(11)
    out = [b"", b"a", b"ab", b"abc" * 700, b"abcdefg" * 301, b"\xff" * 50, bytes(range(256)) * 3, T.gen_english(6000, 3).tobytes(),
           T.gen_dna(5000, 4).tobytes()]
    for d in (2, 8, 9, 17, 33, 65, 129, 256):
        out.append(rng.integers(0, d, 2000, dtype=np.int64).astype(np.uint8).tobytes())
    return out


def host(stream, k):
    """(status, bytes) of tdc_sle_decode"""
    try:
        return 0, T.sle_decode_literals(stream, k)
    except T.TdcGpuError as e:
        return e.status, None


def model(stream, k):
    try:
        return 0, M.decode(stream, k)
    except M.Malformed:
        return -2, None


def test_symbol_exported_and_bound():
    assert "tdc_sle_decode" in T.SYMBOLS and hasattr(T._native.load(), "tdc_sle_decode")
    assert T.STAGE_SLE == 4 and callable(T.sle_decode_literals)


@pytest.mark.parametrize("k", KMERS)
def test_host_loop_equals_the_model(k):
    for data in texts():
        z = M.encode(data, k)
        assert host(z, k) == (0, data), (k, data[:8])
    assert host(M.encode(b"abcabc", 3), 0) == (0, b"abcabc")                    # kmer 0 means 3
    assert host(b"\x00\x00", 8)[0] == -2                                        # TDC_GPU_ERR_ARG


@pytest.mark.parametrize("k", (1, 3, 7))
def test_host_loop_refuses_what_the_model_refuses(k):
    rng = random.Random(k)
    seen = set()
    for data in (b"abracadabra" * 9, texts()[7][:400], texts()[-1][:300], texts()[-3][:300]):
        z = M.encode(data, k)
        damaged = [z[:i] for i in range(len(z))] if len(z) < 400 else [z[:i] for i in range(0, len(z), 7)]
        for _ in range(150):
            i = rng.randrange(len(z) * 8)
            damaged.append(z[:i >> 3] + bytes([z[i >> 3] ^ (0x80 >> (i & 7))]) + z[(i >> 3) + 1:])
        for s in damaged:
            want = model(s, k)
            assert host(s, k) == want, (k, s.hex())
            seen.add(want[0])
    assert seen == {0, -2}
    # each refusal by name
    w = BitWriter(); w.compressed_int(1025)
    assert host(w.finish(), k)[0] == -2                                         # sigma > 1024
    w = BitWriter(); w.compressed_int(2); w.compressed_int(0x61)
    assert host(w.finish(), k)[0] == -2                                         # the ranking runs off the end
    w = BitWriter(); w.compressed_int(1); w.compressed_int(0x161)
    assert host(w.finish(), k)[0] == -2                                         # neither a byte nor a k-mer
    if k < 7:
        w = BitWriter(); w.compressed_int(1); w.compressed_int(M.MARK | (1 << (8 * k)))
        assert host(w.finish(), k)[0] == -2                                     # a k-mer of another kmer
    w = BitWriter(); M.header_bits(w, [0x61, 0x62, 0x63]); w.write(3, 2)
    assert host(w.finish(), k)[0] == -2                                         # rank 3 >= sigma 3
    w = BitWriter(); M.header_bits(w, list(range(17))); w.write(1, 1); w.write(16, 5); w.write(1, 1); w.write(0, 2)
    assert host(w.finish(), k)[0] == -2                                         # a code cut off by the end
    assert host(b"", k)[0] == -2


def test_out_null_measures_and_short_buffers_are_refused():
    L = T._native.load()
    data = T.gen_english(3000, 5).tobytes()
    z = np.frombuffer(M.encode(data, 3), dtype=np.uint8)
    n = ctypes.c_size_t()
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert L.tdc_sle_decode(p, len(z), 3, None, 0, ctypes.byref(n)) == 0 and n.value == len(data)
    out = np.zeros(len(data), dtype=np.uint8)
    assert L.tdc_sle_decode(p, len(z), 3, out.ctypes.data_as(ctypes.c_void_p), len(data), ctypes.byref(n)) == 0 and out.tobytes() == data
    short = np.zeros(100, dtype=np.uint8)
    assert L.tdc_sle_decode(p, len(z), 3, short.ctypes.data_as(ctypes.c_void_p), 100, ctypes.byref(n)) == -2 and n.value == len(data)
    assert short.tobytes() == data[:100]
    assert L.tdc_sle_decode(p, len(z), 3, None, 0, None) == -2


def test_chain_parser_bound_and_facades():
    assert T.parse_chain("encode(sle)") == [(4, 3)]
    assert T.parse_chain("encode(sle(kmer=2))") == [(4, 2)] and T.parse_chain("encode(coder=sle(kmer=7))") == [(4, 7)]
    assert T.parse_chain("bwt:rle:mtf:encode(sle)") == [(0, 0), (1, 0), (2, 0), (4, 3)]
    for bad in ("encode(sle(kmer=0))", "encode(sle(kmer=8))", "encode(coder=sle(kmer=-1))"):
        with pytest.raises(RuntimeError, match="kmer"):
            T.parse_chain(bad)
    for other in ("encode(bit)", "encode(gamma)", "encode(coder=ascii)", "encode(sle(k=3))"):
        with pytest.raises(RuntimeError, match="No implementation"):
            T.parse_chain(other)
    # 13 bits per byte, 1024 ranking entries of ten bytes, sigma and the terminator
    assert T.pipeline_bound([T.STAGE_SLE], 0) == 2 + 10240 + 2
    assert T.pipeline_bound([(T.STAGE_SLE, 7)], 1000) == 1625 + 2 + 10240 + 2
    assert T.pipeline_bound([(T.STAGE_SLE, 8)], 1000) == 0 and T.pipeline_bound([5], 1000) == 0
    assert T.pipeline_bound([T.STAGE_SLE], (1 << 32) - 2) == 0
    for data in texts():
        for k in (1, 3):
            assert len(M.encode(data, k)) <= T.pipeline_bound([(T.STAGE_SLE, k)], len(data))
    c = T.LiteralEncoder(None, coder="sle")
    assert c.stages == [(4, 3)] and T.LiteralEncoder(None, coder="sle", kmer=5, dec="host").stages == [(4, 5)]
    z = M.encode(b"hello hello hello", 5)
    assert T.LiteralEncoder(None, coder="sle", kmer=5, dec="host").decompress(z) == b"hello hello hello"
    assert T.LiteralEncoder(None).stages == [(3, 0)]
    with pytest.raises(RuntimeError):
        T.LiteralEncoder(None, coder="bit")
    with pytest.raises(RuntimeError, match="kmer"):
        T.LiteralEncoder(None, coder="sle", kmer=9)


def test_registry_lists_encode_sle():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    names = [ln.split("[")[0].strip() for ln in r.stdout.splitlines()[1:]]
    assert "encode(sle)" in names and "encode(sle(kmer=3))" in names and "encode(huff)" in names
    assert not [n for n in names if ":" in n]


DATA = b"\x00\xffab\xff\xfe\x00" * 50 + T.gen_english(5000, 3).tobytes() + bytes(range(256)) * 3 + b"abc" * 300 + b"\xff\xff"


@pytest.mark.parametrize("algo,k", [("encode(sle(kmer=1))", 1), ("encode(sle)", 3), ("encode(coder=sle(kmer=7))", 7)], ids=["k1", "default", "k7"])
def test_tdc_decompresses_model_files_without_a_gpu(tmp_path, algo, k):
    f, out = tmp_path / "p.tdc", tmp_path / "p.out"
    f.write_bytes(algo.encode() + b"%" + M.encode(DATA, k))                  # the kmer comes from the file's header
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == DATA


def test_tdc_refuses_bad_kmers_other_coders_chains_and_damage(tmp_path):
    f = tmp_path / "p.tdc"
    src = tmp_path / "in.txt"
    src.write_bytes(b"abracadabra")
    for algo in ("encode(sle(kmer=8))", "encode(sle(kmer=0))"):
        r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "o"), str(src)], capture_output=True, text=True)
        assert r.returncode == 1 and "kmer" in r.stderr and not (tmp_path / "o").exists(), algo
        f.write_bytes(algo.encode() + b"%" + M.encode(b"abc", 3))
        r = subprocess.run([TDC, "-d", "-o", str(tmp_path / "o"), str(f)], capture_output=True, text=True)
        assert r.returncode == 1 and "kmer" in r.stderr and not (tmp_path / "o").exists(), algo
    for algo in ("encode(bit)", "encode(gamma)", "rle:encode(sle)", "bwt:rle:mtf:encode(sle)"):
        r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "o"), str(src)], capture_output=True, text=True)
        assert r.returncode == 1 and "No implementation" in r.stderr and not (tmp_path / "o").exists(), algo
    z = M.encode(DATA, 3)
    for blob in (b"encode(sle)%", b"encode(sle)%" + z[:100], b"encode(sle):mtf%" + z, b"encode(sle(kmer=2))%" + z[:40]):
        f.write_bytes(blob)
        r = subprocess.run([TDC, "-d", "-o", str(tmp_path / "o"), str(f)], capture_output=True, text=True)
        assert r.returncode == 1 and not (tmp_path / "o").exists(), blob[:24]
