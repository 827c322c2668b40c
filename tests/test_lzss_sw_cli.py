"""CPU tests of the lzss interface (no GPU): the host parse tdc_lzss_sw_factors and the host decoder tdc_lzss_sw_decode against the model
(tests/models/lzss_sw.py) on good and damaged streams, the refusals by name, and the `tdc` command line -- -d of model-made files, the
refused spellings, -l."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests.models import lzss_sw as M
from tests.models.lzss_coders import terminate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CODER_ID = {"ascii": T.CODER_ASCII, "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
ERR_ARG, ERR_TOO_LARGE, ERR_UNSUPPORTED = -2, -4, -6


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def host_factors(data, w, t):
    p, s, l = T.lzss_sw_factors(data, w, t)
    return list(zip(p.tolist(), s.tolist(), l.tolist()))


def host_decode(stream, coder, w):
    """(status, text) of tdc_lzss_sw_decode"""
    try:
        return 0, T.lzss_sw_decode(stream, CODER_ID[coder], w)
    except T.TdcGpuError as e:
        return e.status, None


def model_decode(stream, coder, w):
    try:
        return 0, M.decode(stream, coder, w)
    except M.Malformed:
        return ERR_ARG, None
    except M.TooLarge:
        return ERR_TOO_LARGE, None


def test_symbols_and_facade():
    lib = T._native.load()
    for name in ("tdc_gpu_lzss_sw_compress", "tdc_gpu_lzss_sw_compress_into", "tdc_gpu_lzss_sw_bound", "tdc_gpu_lzss_sw_factorize",
                 "tdc_lzss_sw_factors", "tdc_lzss_sw_decode"):
        assert name in T.SYMBOLS and hasattr(lib, name)
    for name in ("lzss_sw_compress", "lzss_sw_compress_into", "lzss_sw_factorize", "lzss_sw_bound"):
        assert hasattr(T.Context, name)


def test_host_parse_equals_the_model():
    for data, w, t in M.sweep(20261019, 4000):
        assert host_factors(data, w, t) == M.factors(data, w, t), (data, w, t)
    assert host_factors(b"", 16, 3) == []
    assert host_factors(b"abxabyab", 16, 2)[-1] == (6, 0, 2)                    # of two equally long matches the farther one


def test_host_decode_equals_the_model_on_good_streams():
    for data, w, t in M.sweep(5, 1500):
        toks = M.parse(data, w, t)
        for coder in M.CODERS:
            s = M.encode(toks, coder, w)
            assert host_decode(s, coder, w) == model_decode(s, coder, w), (data, w, t, coder)
            if not (coder == "bit" and M.truncates(data, w, t)):
                assert host_decode(s, coder, w) == (0, data)


def test_bound_covers_the_model_streams():
    for data, w, t in M.sweep(11, 700):
        toks = M.parse(data, w, t)
        for coder in M.CODERS:
            assert len(M.encode(toks, coder, w)) <= T.lzss_sw_bound(len(data), w, CODER_ID[coder]), (data, w, t, coder)
    assert T.lzss_sw_bound(100, 16, T.CODER_HUFF) == 0 and T.lzss_sw_bound(100, 0, T.CODER_BIT) == 0
    assert T.lzss_sw_bound(100, 4097, T.CODER_BIT) == 0 and T.lzss_sw_bound(100, 4096, T.CODER_BIT) > 0


@pytest.mark.parametrize("coder", M.CODERS)
def test_refusals_by_name(coder):
    enc = lambda toks, w=16: M.encode(toks, coder, w)
    assert host_decode(enc([(0, None, 97), (1, 1, 2)]), coder, 16)[0] == ERR_ARG                 # distance 0
    if coder != "bit":                                                                            # (bit: bits_for(1) = 1 bit holds 0 or 1)
        assert host_decode(enc([(0, None, 97), (1, -1, 2)]), coder, 16)[0] == ERR_ARG            # distance 2 above a text of 1
    assert host_decode(enc([(0, 0, 3)]), coder, 16)[0] == ERR_ARG                                 # a factor in front of any text
    bits = M.encode_bits([(0, None, 97), (1, 0, 5), (6, None, 98)], coder, 16)
    for cut in (1, 3, 7):                                                                         # the last token cut off
        s = terminate(bits[:-cut])
        assert model_decode(s, coder, 16)[0] == ERR_ARG
        assert host_decode(s, coder, 16)[0] == ERR_ARG
    assert host_decode(enc([(0, None, 97), (1, 0, 0), (1, None, 98)]), coder, 16) == (0, b"ab")  # length 0 decodes to nothing
    if coder != "bit":                                                                            # (bit: 5 bits hold at most 31)
        big = enc([(0, None, 97), (1, 0, M.TEXT_MAX)])                                            # 1 + (2^32 - 2) bytes
        assert host_decode(big, coder, 16)[0] == ERR_TOO_LARGE == model_decode(big, coder, 16)[0]


def test_prefixes_the_field_readers_refuse():
    assert host_decode(terminate("1" + "0" * 70 + "1"), "gamma", 16)[0] == ERR_ARG               # a unary prefix above 64
    assert host_decode(terminate("1" + "0000"), "gamma", 16)[0] == ERR_ARG                       # ... that runs into the end
    assert host_decode(terminate("1" + "0000000" + "1" + "1111111" + "0" * 20), "delta", 16)[0] == ERR_ARG    # a delta width of 127
    assert host_decode(terminate("00110001" + "01100001"), "ascii", 16)[0] == ERR_ARG            # '1' 'a': an integer expected


def test_other_arguments():
    L = T._native.load()
    n = ctypes.c_size_t()
    assert L.tdc_lzss_sw_decode(None, 0, T.CODER_HUFF, 16, None, 0, ctypes.byref(n)) == ERR_UNSUPPORTED
    assert L.tdc_lzss_sw_decode(None, 0, T.CODER_BIT, 0, None, 0, ctypes.byref(n)) == ERR_ARG
    assert L.tdc_lzss_sw_decode(None, 0, T.CODER_GAMMA, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert L.tdc_lzss_sw_decode(None, 0, T.CODER_BIT, 16, None, 0, None) == ERR_ARG
    s = np.frombuffer(M.encode(M.parse(b"abcabcabc", 16, 3), "bit", 16), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint8)
    assert L.tdc_lzss_sw_decode(s.ctypes.data, len(s), T.CODER_BIT, 16, out.ctypes.data, 4, ctypes.byref(n)) == ERR_ARG and n.value == 9
    assert not out.any()                                                                          # a buffer too small is left alone
    with pytest.raises(T.TdcGpuError):
        T.lzss_sw_factors(b"abc", 0, 3)
    assert T.lzss_sw_factors(b"abcabcabc", 100000, 3)[2].tolist() == [6]                          # the host takes any window


@pytest.mark.parametrize("coder", M.CODERS)
def test_damaged_streams_get_the_models_verdict(coder):
    w = 16
    s = M.encode(M.parse(b"abcabcabcxabcabb", w, 3), coder, w)
    damaged = [s[:k] for k in range(len(s))]                                                      # every truncation
    damaged += [s[:i] + bytes([s[i] ^ (1 << b)]) + s[i + 1:] for i in range(len(s)) for b in range(8)]    # every single bit
    verdicts = set()
    for d in damaged:
        got, want = host_decode(d, coder, w), model_decode(d, coder, w)
        assert got == want, (d.hex(), got, want)
        verdicts.add(want[0])
    assert {0, ERR_ARG} <= verdicts


HEADERS = [("lzss(coder=%s)", 16, 3), ("lzss(coder=%s,window=64,threshold=2)", 64, 2), ("lzss(coder=%s, window=3)", 3, 3),
           ("lzss(%s, 8, 1)", 8, 1)]


@pytest.mark.parametrize("coder", M.CODERS)
@pytest.mark.parametrize("header,w,t", HEADERS)
def test_tdc_d_decodes_model_files(tmp_path, coder, header, w, t):
    data = T.gen_english(3000, 21).tobytes() + b"\x00\xff" + b"a" * 300 + b"abc" * 50
    if coder == "bit" and M.truncates(data, w, t):
        data = T.gen_english(3000, 21).tobytes() + b"\x00\xff"
        assert not M.truncates(data, w, t)
    f = tmp_path / "p.tdc"
    f.write_bytes((header % coder).encode() + b"%" + M.encode(M.parse(data, w, t), coder, w))
    out = tmp_path / "p.out"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data


def test_tdc_d_refuses_a_bad_distance(tmp_path):
    f = tmp_path / "bad.tdc"
    f.write_bytes(b"lzss(coder=gamma)%" + M.encode([(0, None, 97), (1, -4, 3)], "gamma", 16))
    r = subprocess.run([TDC, "-d", "-o", str(tmp_path / "bad.out"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and "corrupt stream" in r.stderr


@pytest.mark.parametrize("algo,word", [("lzss", "No implementation found"), ("lzss(coder=huff)", "No implementation found"),
                                       ("lzss(coder=sle)", "No implementation found"), ("lzss(coder=arithmetic)", "No implementation found"),
                                       ("lzss(coder=bit,window=0)", "window"), ("lzss(coder=bit,window=4097)", "window")])
def test_refused_spellings(tmp_path, algo, word):
    f = tmp_path / "in.txt"
    f.write_bytes(b"abc")
    r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "o.tdc"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and word in r.stderr
    assert not (tmp_path / "o.tdc").exists()


def test_python_facade_refusals_and_host_loop():
    for coder in (None, "huff", "sle", "arithmetic"):
        with pytest.raises(RuntimeError, match="No implementation found"):
            T.LZSSSlidingWindowCompressor(None, coder=coder)
    for w in (0, 4097):
        with pytest.raises(RuntimeError, match="window"):
            T.LZSSSlidingWindowCompressor(None, coder="bit", window=w)
    data = b"tobeornottobeortobeornot" * 40
    for coder in M.CODERS:
        z = T.LZSSSlidingWindowCompressor(None, coder=coder, window=64, threshold=2)
        assert z.decompress(M.encode(M.parse(data, 64, 2), coder, 64)) == data


def test_registry_lists_lzss():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "lzss(coder=bit | ascii | gamma | delta, window=16, threshold=3)" in r.stdout
