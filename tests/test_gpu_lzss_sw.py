"""GPU tests of lzss (tdc_gpu_lzss_sw_factorize, tdc_gpu_lzss_sw_compress{,_into}; lzss_sw.hip and the shared field coder, field_coder.hpp): the
device factors against the host parse tdc_lzss_sw_factors (which tests/test_lzss_sw_cli.py holds against the model), the device streams
byte for byte against the model's coders (tests/models/lzss_sw.py), every stream back through tdc_lzss_sw_decode, the refusals, and the
`tdc` round trip."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests.models import lzss_sw as M

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CID = {"ascii": T.CODER_ASCII, "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
TILE = 4096            # SW_TILE of lzss_sw.hip: text positions per workgroup of the match kernel


@pytest.fixture(scope="module")
def dev():
    with T.Context(0) as ctx:
        yield ctx


def host(data, w, t):
    p, s, l = T.lzss_sw_factors(data, w, t)
    return list(zip(p.tolist(), s.tolist(), l.tolist()))


def device(ctx, data, w, t):
    p, s, l = ctx.lzss_sw_factorize(data, w, t)
    return list(zip(p.tolist(), s.tolist(), l.tolist()))


def tokens(data, factors):
    """the token list of the model from a factor list sorted by pos"""
    out, p = [], 0
    for pos, src, ln in factors:
        out.extend((q, None, data[q]) for q in range(p, pos))
        out.append((pos, src, ln))
        p = pos + ln
    out.extend((q, None, data[q]) for q in range(p, len(data)))
    return out


def check_factors(ctx, data, w, t):
    want = host(data, w, t)
    assert device(ctx, data, w, t) == want, (len(data), w, t)
    return want


def check_stream(ctx, data, w, t, coder, factors=None):
    """the device stream equals the model's and decodes to the text; returns (stream, stats)"""
    factors = host(data, w, t) if factors is None else factors
    want = M.encode(tokens(data, factors), coder, w)
    got, st = ctx.lzss_sw_compress(data, w, t, CID[coder])
    assert got == want, (len(data), w, t, coder)
    assert T.lzss_sw_decode(got, CID[coder], w) == data
    assert st["n"] == len(data) and st["out_len"] == len(got) and st["factors"] == len(factors)
    assert st["flen_max"] == max((f[2] for f in factors), default=0)
    assert len(got) <= T.lzss_sw_bound(len(data), w, CID[coder])
    return got, st


def two_letters(n, seed):
    return (np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8) + ord("a")).tobytes()


@functools.lru_cache(maxsize=None)
def english(n):
    return T.gen_english(n, 42).tobytes()


def fibonacci_word(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


@pytest.mark.parametrize("w", [1, 2, 3, 4, 16])
def test_every_length_to_200(dev, w):
    for t in (1, 3):
        for n in range(201):
            check_factors(dev, two_letters(n, 1000 * w + n), w, t)


@pytest.mark.parametrize("w", [1, 3, 16, 100])
def test_lengths_around_the_window_and_the_tiles(dev, w):
    for n in (w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5):
        for t in (1, 3):
            f = check_factors(dev, two_letters(n, 7 * n + w), w, t)
            if n >= 2 * w and w > 1 and t == 1:
                assert f, (n, w)


@pytest.mark.parametrize("w", [2, 3, 5, 16, 64])
def test_runs_and_periodic_texts(dev, w):
    n = 2 * TILE + 37
    f = check_factors(dev, b"a" * n, w, 3)
    if w >= 2:
        assert f[0] == (1, 0, 2 * w - 1)                        # the longest factor there is, overlapping its own source
    for period in (w, w + 1, w - 1):                           # a source at the far end of the window, just outside it, just inside
        if period < 1:
            continue
        unit = bytes((7 * i) % 251 for i in range(period))      # pairwise distinct bytes: the only matches are a period away
        data = (unit * (n // period + 1))[:n]
        f = check_factors(dev, data, w, 2)
        assert bool(f) == (period <= w), (w, period)            # a period of w + 1 has its source one byte outside the window
    for coder in ("bit", "gamma"):
        if not (coder == "bit" and M.truncates(b"a" * 4 * w, w, 3)):
            check_stream(dev, b"a" * n, w, 3, coder)


def test_sources_and_factors_across_a_tile_border(dev):
    rng = np.random.default_rng(5)
    base = bytearray(rng.permutation(np.arange(3 * TILE) % 251).astype(np.uint8).tobytes())
    a = bytearray(base)
    a[TILE + 2:TILE + 10] = a[TILE - 10:TILE - 2]               # the best source lies in the previous tile
    f = check_factors(dev, bytes(a), 16, 3)
    assert any(p == TILE + 2 and s == TILE - 10 and l >= 8 for p, s, l in f)
    b = bytearray(base)
    b[TILE - 4:TILE + 6] = b[TILE - 15:TILE - 5]                # a factor that starts in one tile and ends in the next
    f = check_factors(dev, bytes(b), 16, 3)
    assert any(p < TILE < p + l for p, s, l in f)
    check_stream(dev, bytes(b), 16, 3, "bit", f)


def test_fibonacci_word_and_english(dev):
    fib = fibonacci_word(20000)
    for w in (16, 100):
        check_factors(dev, fib, w, 3)
    check_stream(dev, fib, 16, 3, "delta")
    data = english(1 << 20)
    f = check_factors(dev, data, 16, 3)
    assert len(f) > 1000
    got, st = dev.lzss_sw_compress(data, 16, 3, T.CODER_BIT)
    assert st["factors"] == len(f) and T.lzss_sw_decode(got, T.CODER_BIT, 16) == data


def test_largest_window(dev):
    n = 3 * 4096 + 7
    for data in (english(n), two_letters(n, 3), (english(3000) * 5)[:n]):
        f = check_factors(dev, data, 4096, 3)
        assert f
        check_stream(dev, data, 4096, 3, "bit", f)              # (4096 is a power of two: 13 bits hold 8191)
    assert max(l for _, _, l in host((english(3000) * 5)[:n], 4096, 3)) > 4096      # longer than the window


def test_threshold_above_every_match(dev):
    data = b"ab" * 500
    assert check_factors(dev, data, 16, 33) == []               # t > 2w: no factor at all
    assert check_factors(dev, data, 16, 30)[0] == (2, 0, 30)    # (the look-ahead at p = 2 is 2w - 2)
    check_stream(dev, data, 16, 33, "gamma")
    assert check_factors(dev, data, 16, 0) == host(data, 16, 1)
    # every position a literal: as many tokens as bytes.  Token counts on both sides of the coder's tile border (2048 tokens, 8 per
    # thread), and 13 and 14 tokens: under bit their streams end with 5 and with 6 bits in the last byte, the two sides of the
    # terminator rule (9 bits per literal)
    for n in (13, 14, 2047, 2048, 2049, 4096, 4097):
        text = two_letters(n, n)
        assert host(text, 16, 33) == []
        for coder in M.CODERS:
            got, _ = check_stream(dev, text, 16, 33, coder, [])
            if coder == "bit":
                assert len(got) == (9 * n) // 8 + (1 if (9 * n) % 8 <= 5 else 2)


def test_of_equal_matches_the_farther_one(dev):
    assert check_factors(dev, b"abxabyab", 16, 2)[-1] == (6, 0, 2)
    data = b"0123abcd4567abcd89abcd"
    assert check_factors(dev, data, 16, 3)[-1] == (18, 4, 4)    # sources 4 and 12 both match 4 bytes


@pytest.mark.parametrize("coder", M.CODERS)
def test_coders(dev, coder):
    data = english(64 << 10)
    f = host(data, 16, 3)
    check_stream(dev, data, 16, 3, coder, f)
    check_stream(dev, b"a" * 5000, 16, 3, coder)
    check_stream(dev, b"", 16, 3, coder)
    check_stream(dev, b"q", 16, 3, coder)
    check_stream(dev, english(5000) + b"\x00\xff" * 9, 64, 2, coder)


def test_into_and_the_short_buffer(dev):
    data = english(20000)
    want, _ = check_stream(dev, data, 16, 3, "gamma")
    out = np.full(T.lzss_sw_bound(len(data), 16, T.CODER_GAMMA), 0xA5, dtype=np.uint8)
    n, st = dev.lzss_sw_compress_into(data, len(data), out, 16, 3, T.CODER_GAMMA)
    assert out[:n].tobytes() == want and (out[n:] == 0xA5).all() and st["out_len"] == n
    short = np.full(len(want) - 1, 0xA5, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        dev.lzss_sw_compress_into(data, len(data), short, 16, 3, T.CODER_GAMMA)
    assert e.value.status == ERR_OOM and e.value.required == len(want) and (short == 0xA5).all()
    check_stream(dev, data, 16, 3, "gamma")                     # a valid call after the refusal


def test_bit_coder_refuses_lengths_it_would_truncate(dev):
    data = b"aaaaaaaa"
    assert M.truncates(data, 3, 3)
    out = np.full(64, 0xA5, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        dev.lzss_sw_compress_into(data, len(data), out, 3, 3, T.CODER_BIT)
    assert e.value.status == ERR_UNSUPPORTED and (out == 0xA5).all()
    L = T._native.load()
    a = np.frombuffer(data, dtype=np.uint8)
    p, n = ctypes.c_void_p(0x1234), ctypes.c_size_t(77)
    assert L.tdc_gpu_lzss_sw_compress(dev._h, a.ctypes.data, len(a), 3, 3, T.CODER_BIT, ctypes.byref(p), ctypes.byref(n), None) == ERR_UNSUPPORTED
    assert p.value == 0x1234 and n.value == 77                  # nothing written
    check_stream(dev, data, 3, 3, "gamma")                      # the same text under a coder that ignores the range
    check_stream(dev, data, 4, 3, "bit")                        # and under a window whose field holds 2w - 1
    check_factors(dev, data, 3, 3)


def test_refused_arguments(dev):
    data = b"abcabcabc"
    for w, status in ((0, ERR_ARG), (4097, ERR_UNSUPPORTED)):
        with pytest.raises(T.TdcGpuError) as e:
            dev.lzss_sw_compress(data, w, 3, T.CODER_BIT)
        assert e.value.status == status
        check_stream(dev, data, 16, 3, "bit")
        with pytest.raises(T.TdcGpuError) as e:
            dev.lzss_sw_factorize(data, w, 3)
        assert e.value.status == status
        check_factors(dev, data, 16, 3)
    for coder in (T.CODER_HUFF, T.CODER_ARITH, T.CODER_SLE, 99):
        with pytest.raises(T.TdcGpuError) as e:
            dev.lzss_sw_compress(data, 16, 3, coder)
        assert e.value.status == ERR_UNSUPPORTED
        check_stream(dev, data, 16, 3, "ascii")
    L = T._native.load()
    n = ctypes.c_size_t()
    a = np.frombuffer(data, dtype=np.uint8)
    assert L.tdc_gpu_lzss_sw_compress(dev._h, a.ctypes.data, len(a), 16, 3, T.CODER_BIT, None, ctypes.byref(n), None) == ERR_ARG
    assert L.tdc_gpu_lzss_sw_compress(dev._h, None, 5, 16, 3, T.CODER_BIT, None, ctypes.byref(n), None) == ERR_ARG
    check_stream(dev, data, 16, 3, "delta")


def test_facade_and_command_line(dev, tmp_path):
    data = english(30000) + b"\x00\xff" + b"a" * 300
    z = T.LZSSSlidingWindowCompressor(dev, coder="ascii", window=64, threshold=2)
    s = z.compress(data)
    assert s == M.encode(tokens(data, host(data, 64, 2)), "ascii", 64) and z.decompress(s) == data
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    src = tmp_path / "in.txt"
    src.write_bytes(data)
    for algo, w, t, coder in (("lzss(coder=bit)", 16, 3, "bit"), ("lzss(coder=ascii,window=64,threshold=2)", 64, 2, "ascii")):
        packed, back = tmp_path / "p.tdc", tmp_path / "p.out"
        r = subprocess.run([TDC, "-a", algo, "-f", "-o", str(packed), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert packed.read_bytes() == algo.encode() + b"%" + M.encode(tokens(data, host(data, w, t)), coder, w)
        r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(packed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data
