"""GPU tests of lzw(coder=bit | gamma) (tdc_gpu_lzw_compress, tdc_gpu_lzw_decompress{,_into}; lzw.hip, lz78_decode.hip): the device
coder byte for byte against the model (tests/models/lzw.py), the device decoder (option dec_parse = 2: every stream) back to the
text -- exact code counts at the width steps, KwKwK chains, many segments, the caller's buffer --, what it refuses, a differential run
against the host loop on damaged streams, and the facade / `tdc` round trips."""
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import tudocomp_amd as T
from tests import corpus
from tests.coder_borders import LZW_COUNTS, phrase_prefixes, two_letters_64k
from tests.lzw_damage import base_stream, damaged_streams
from tests.models import lzw as M

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CODERS = ("bit", "gamma")
CID = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA}


@pytest.fixture(scope="module")
def dev():
    """every stream on the device, whatever its size"""
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        yield ctx


@functools.lru_cache(maxsize=None)
def _big(name):
    """(text, model code list): computed once, shared by the coders and by both directions"""
    if name == "english":
        data = T.gen_english(2 << 20, 31).tobytes()
    elif name == "dna":
        data = T.gen_dna(1 << 20, 32).tobytes()
    elif name == "random":
        data = np.random.default_rng(33).integers(0, 256, 300000, dtype=np.uint8).tobytes()
    elif name == "a^2^21":
        data = b"a" * (1 << 21)
    else:
        data = b"ab" * (1 << 20)
    return data, tuple(M.parse(data))


BIG = ("english", "dna", "random", "a^2^21", "ab^2^20")


def _small_inputs():
    return list(corpus.small_corpus()) + list(corpus.random_small(60, 99)) + [("aa", b"aa"), ("one", b"q"), ("empty2", b"")]


def _check_both_ways(ctx, data, stream, coder):
    got, st = ctx.lzw_decompress(stream, CID[coder])
    assert got == data
    out = np.full(len(data) + 3, 0xA5, dtype=np.uint8)
    n, _ = ctx.lzw_decompress_into(stream, out, CID[coder])
    assert n == len(data) and out[:n].tobytes() == data and (out[n:] == 0xA5).all()
    return st


@pytest.mark.parametrize("coder", CODERS)
def test_compress_small_inputs(dev, coder):
    for name, data in _small_inputs():
        want = M.compress(data, coder)
        got, st = dev.lzw_compress(data, CID[coder])
        assert got == want, name
        assert st["factors"] == len(M.parse(data))
        st = _check_both_ways(dev, data, want, coder)
        assert st["device_parse"] == (1 if data else 0), name           # (the empty stream holds no code: nothing to parse)


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("name", BIG)
def test_compress_and_decompress_large(dev, name, coder):
    data, codes = _big(name)
    if name == "random":
        assert len(codes) > 65280                                        # crosses the 16 -> 17 bit width
    want = M.encode_fast(codes, coder)
    got, st = dev.lzw_compress(data, CID[coder])
    assert st["factors"] == len(codes)
    assert got == want
    dst = _check_both_ways(dev, data, want, coder)
    assert dst["codes"] == len(codes) and dst["device_parse"] == 1
    if name == "a^2^21":                                                 # every code but the last is KwKwK: the chain is the code list
        assert all(c == 255 + k for k, c in enumerate(codes[1:-1], 1))
        assert dst["rounds"] >= 3


@pytest.mark.parametrize("coder", CODERS)
def test_exact_code_counts(dev, coder):
    """Any sequence of codes below 256 is a valid stream.  The counts sit on the width steps of the bit coder (256 codes of 9 bits, 512
    of 10, 1024 of 11, ..., 65 280 codes below 17 bits) and the tile edges of both packers; 4000 codes hold 9-bit and 11-bit codes at
    every bit offset mod 64 (9 and 11 are odd), so a code crosses a 64-bit word boundary at every residue."""
    rng = np.random.default_rng(7)
    for z in (1, 255, 256, 257, 767, 768, 769, 2047, 2048, 2049, 4000, 65279, 65280, 65281):
        codes = rng.integers(0, 256, z, dtype=np.int64)
        stream = M.encode_fast(codes, coder) if z > 300 else M.encode(codes.tolist(), coder)
        data = codes.astype(np.uint8).tobytes()
        got, st = dev.lzw_decompress(stream, CID[coder])
        assert st["codes"] == z and got == data, z
    for z in (767, 768, 769, 2049, 65281):                              # and through the packer: a text of z distinct-pair-free phrases
        codes = [int(c) for c in rng.integers(0, 256, z)]
        assert dev.lzw_compress(bytes(codes), CID[coder])[0] == M.compress(bytes(codes), coder)
    # Code counts on both sides of the gamma coder's tile border (2048 items, 8 per thread) and streams on both sides of the terminator
    # rule, for both coders: tests/coder_borders.py, held against the model in tests/test_lzw_model.py
    text = two_letters_64k()
    for k, prefix in phrase_prefixes(text, M.phrase_lengths(np.asarray(M.parse(text)))[0], LZW_COUNTS):
        got, st = dev.lzw_compress(prefix, CID[coder])
        assert st["factors"] == k == len(M.parse(prefix))
        assert got == M.compress(prefix, coder), k
        assert dev.lzw_decompress(got, CID[coder])[0] == prefix


def test_gamma_many_segments():
    data, codes = _big("dna")
    stream = M.encode_fast(codes, "gamma")
    with T.Context(0, options={"dec_parse": 2, "dec_seg": 4096}) as ctx:
        got, _ = ctx.lzw_decompress(stream, T.CODER_GAMMA)
    assert len(stream) * 8 // 4096 >= 300
    assert got == data


@pytest.mark.parametrize("coder", CODERS)
def test_deep_chain(dev, coder):
    """97, 256, 257, ...: code k names the entry made one step earlier, so the chain of links is as deep as the stream has codes and
    phrase k is a^(k + 1).  A chain of depth d costs d (d + 1) / 2 bytes of text, so the format's 2^32 - 2 bytes allow no chain deeper
    than 92 681 (a 10^5 deep one would be a text of 5.0e9 bytes); 46 340 codes decode to 2^30 bytes here."""
    z = 46340
    codes = np.concatenate(([97], 256 + np.arange(z - 1)))
    n = z * (z + 1) // 2
    out = np.zeros(n, dtype=np.uint8)
    got, st = dev.lzw_decompress_into(M.encode_fast(codes, coder), out, CID[coder])
    assert got == n and st["codes"] == z
    assert int(np.count_nonzero(out != 97)) == 0


def _valid_after(ctx, coder):
    data = b"still here " * 50
    assert ctx.lzw_decompress(M.compress(data, coder), CID[coder])[0] == data


@pytest.mark.parametrize("coder", CODERS)
def test_refusals(dev, coder):
    good = M.compress(T.gen_english(50000, 3).tobytes(), coder)
    cut = good[:len(good) // 2 - 1] + bytes([good[len(good) // 2 - 1] & 0xF8 | (3 if coder == "bit" else 1)])
    for bad in (M.encode([256], coder), M.encode([97, 98, 99, 259], coder), M.encode([97] * 700 + [256 + 700], coder), cut):
        with pytest.raises(M.Malformed):
            M.decode(bad, coder)
        with pytest.raises(T.TdcGpuError) as e:
            dev.lzw_decompress(bad, CID[coder])
        assert e.value.status == ERR_ARG
        _valid_after(dev, coder)
    assert dev.lzw_decompress(M.encode([97] * 700 + [255 + 700], coder), CID[coder])[0] == b"a" * 702     # equality is KwKwK


@pytest.mark.parametrize("coder", CODERS)
def test_oversized_claim(dev, coder):
    """97, 256, 257, ... with 92 682 codes describes 4.29e9 bytes: refused before anything of that size is allocated"""
    z = 92682
    assert z * (z + 1) // 2 > 2**32 - 2 >= (z - 1) * z // 2
    stream = M.encode_fast(np.concatenate(([97], 256 + np.arange(z - 1))), coder)
    t0 = time.perf_counter()
    with pytest.raises(T.TdcGpuError) as e:
        dev.lzw_decompress(stream, CID[coder])
    assert e.value.status == ERR_TOO_LARGE
    assert time.perf_counter() - t0 < 1.0
    _valid_after(dev, coder)


@pytest.mark.parametrize("coder", CODERS)
def test_into_short_buffer_and_other_coders(dev, coder):
    data, codes = _big("dna")
    stream = M.encode_fast(codes, coder)
    short = np.zeros(len(data) - 1, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        dev.lzw_decompress_into(stream, short, CID[coder])
    assert e.value.status == ERR_OOM and e.value.required == len(data)
    _valid_after(dev, coder)
    for other in (T.CODER_HUFF, T.CODER_ASCII):
        with pytest.raises(T.TdcGpuError) as e:
            dev.lzw_decompress(stream, other)
        assert e.value.status == ERR_UNSUPPORTED
        with pytest.raises(T.TdcGpuError) as e:
            dev.lzw_compress(b"abc", other)
        assert e.value.status == ERR_UNSUPPORTED
    _valid_after(dev, coder)


def test_dec_parse_picks_the_path(gpu_ctx):
    """the default (dec_parse = 1): the device from the threshold on, the host loop below it; 0: the host loop for every size"""
    data, codes = _big("dna")
    big = M.encode_fast(codes, "bit")
    small = M.compress(b"abcabcabc" * 20, "bit")
    got, st = gpu_ctx.lzw_decompress(big)
    assert got == data and st["device_parse"] == 1
    got, st = gpu_ctx.lzw_decompress(small)
    assert got == b"abcabcabc" * 20 and st["device_parse"] == 0
    with T.Context(0, options={"dec_parse": 0}) as host:
        got, st = host.lzw_decompress(big)
        assert got == data and st["device_parse"] == 0


@pytest.mark.parametrize("coder", CODERS)
def test_differential_damaged_streams(dev, coder):
    """150 single-bit flips and truncations of one 200 KB stream: the device path and the facade's host loop return the same bytes, or
    both refuse.  More than half refused by both would show little (tests/test_lzw_model.py checks the seed on the CPU)."""
    data, stream = base_stream(coder)
    assert dev.lzw_decompress(stream, CID[coder])[0] == data
    host = T.LZWCompressor(None, coder=coder, dec="host")
    both_refuse = 0
    cases = damaged_streams(coder)
    for i, s in enumerate(cases):
        try:
            want = host.decompress(s)
        except T.TdcGpuError as e:
            want = e.status
        try:
            got = dev.lzw_decompress(s, CID[coder])[0]
        except T.TdcGpuError as e:
            got = e.status
        assert got == want, i
        both_refuse += isinstance(want, int)
    print("lzw(%s): %d of %d damaged streams refused by both" % (coder, both_refuse, len(cases)))
    assert both_refuse * 2 <= len(cases)
    _valid_after(dev, coder)


@pytest.mark.parametrize("coder", CODERS)
def test_facade_round_trip(dev, coder):
    data, codes = _big("english")
    for dec in ("gpu", "host"):
        z = T.LZWCompressor(dev, coder=coder, lz78trie="ternary", dec=dec)
        stream = z.compress(data)
        assert stream == M.encode_fast(codes, coder)
        assert z.decompress(stream) == data
        assert z.decompress(z.compress(b"")) == b""


@pytest.mark.parametrize("algo", ["lzw(coder=bit,dec=gpu)", "lzw(coder=gamma)", "lzw", "lzw(coder=bit,lz78trie=ternary,dec=gpu)"])
def test_tdc_round_trip(tmp_path, algo):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    data, codes = _big("dna")
    src, packed, back = tmp_path / "in.bin", tmp_path / "in.tdc", tmp_path / "in.out"
    src.write_bytes(data)
    r = subprocess.run([TDC, "-a", algo, "-o", str(packed), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blob = packed.read_bytes()
    assert blob.startswith(algo.encode() + b"%")
    assert blob[len(algo) + 1:] == M.encode_fast(codes, "gamma" if "gamma" in algo else "bit")
    r = subprocess.run([TDC, "-d", "-o", str(back), str(packed)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == data
