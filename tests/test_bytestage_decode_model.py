"""CPU tests of the parallel formulations behind the device decoders of rle, mtf and encode(huff) (tests/models/bytestage_decode.py)
against the host decoders of the C ABI, which are their specification: same bytes, and the same verdict on every malformed stream."""
import random

import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.models import bwtzip as M
from tests.models import bytestage_decode as D

RLE_VECTORS = [(b"\x61" * 5, "616103"), (b"\x61" * 5 + b"\x62", "61610362"), (b"\x80" * 5, "808000800080008000"),
               (b"\xff" * 3 + b"\x62", "ffff00ff0062"), (b"\x62\xff", "62ff"), (b"\x61" * 300, "6161aa02"), (b"\x62\xff\xff", "62ffff00")]


def host(fn, *args):
    """(True, bytes) or (False, None): what the host decoder does with the stream"""
    try:
        return True, fn(*args)
    except T.TdcGpuError as e:
        assert e.status == -2
        return False, None


LIMIT = 1 << 22


def host_rle(s, off):
    """the host decoder with the stage limit scaled down to LIMIT: measured first (a stream may ask for 2^64 - 1 bytes)"""
    import ctypes
    import numpy as np
    L = T._native.load()
    a = np.frombuffer(bytes(s), dtype=np.uint8)
    n = ctypes.c_size_t()
    rc = L.tdc_rle_decode(a.ctypes.data_as(ctypes.c_void_p) if len(a) else None, len(a), ctypes.c_uint64(off), None, 0, ctypes.byref(n))
    if rc or n.value > LIMIT:
        return False, None
    return True, T.rle_decode(s, off)


def model(fn, *args, **kw):
    try:
        return True, fn(*args, **kw)
    except D.Refused:
        return False, None


def texts():
    rng = random.Random(11)
    out = [d for _, d in corpus.small_corpus() + corpus.random_small(30, 5)]
    out += [b"", b"a", b"\xff", bytes(range(256)) * 3, corpus.run_rich(2000, rng), T.gen_english(3000, 3).tobytes(), corpus.fib_word(14)]
    out += [bytes(rng.choice([0x61, 0x7F, 0x80, 0xFF, 0x00]) for _ in range(rng.randrange(1, 200))) for _ in range(40)]
    out += [b"\x80" * 40, b"\xff" * 40, b"\x80\x80\x00" * 9, b"cc\x63" * 5]
    return out


def test_rle_vectors_and_quirks():
    for data, enc in RLE_VECTORS:
        for tile, group, piece in ((11, 2, 1), (16, 4, 8), (512, 512, 256)):
            assert D.rle_decode(bytes.fromhex(enc), 0, tile, group, piece) == data


@pytest.mark.parametrize("offset", [0, 3, 200])
def test_rle_model_equals_host(offset):
    for data in texts():
        e = M.rle_encode(data, offset)
        assert D.rle_decode(e, offset) == data == T.rle_decode(e, offset)
        assert D.rle_decode(e, offset, tile=11, group=2, piece=3) == data
        # the stream read with another offset, and the text itself read as a stream: both decoders agree on accept / refuse and bytes
        for s, o in ((e, offset + 1), (e, 0), (data, offset)):
            assert model(D.rle_decode, s, o, limit=LIMIT) == host_rle(s, o), (s[:40], o)


def test_rle_vbyte_lengths_one_to_five():
    for k in range(1, 6):
        run = 1 << (7 * (k - 1))                                   # the shortest run whose vbyte has k bytes
        s = b"aa" + M.vbyte(run) + b"b"
        assert len(M.vbyte(run)) == k
        got = D.rle_decode(s, 0, tile=16, group=4, piece=1 << 20)
        assert got == T.rle_decode(s) == b"a" * (run + 2) + b"b"
        big = (1 << (7 * (k - 1))) + 5                              # ... and small runs behind a large offset
        s = M.rle_encode(b"xxyyyzzzz" * 20, big)
        assert D.rle_decode(s, big) == T.rle_decode(s, big) == b"xxyyyzzzz" * 20


def test_rle_malformed():
    bad = [b"aa", b"aa\x80\x80", b"aa" + b"\x80" * 10 + b"\x01", b"aa" + b"\x80" * 9 + b"\x01", b"aa" + b"\xff" * 9 + b"\x01",
           b"ab" * 20 + b"cc", b"\x80\x80", b"\xff\xff\xff", b"cc\x63\x63", b"q" * 7]
    for s in bad:
        for off in (0, 3, 200):
            assert model(D.rle_decode, s, off, limit=LIMIT) == host_rle(s, off), (s, off)
    rng = random.Random(3)
    for _ in range(300):                                            # random bytes rich in pairs and continuation bits
        s = bytes(rng.choice([0x61, 0x61, 0x62, 0x80, 0x81, 0x01, 0xFF]) for _ in range(rng.randrange(1, 60)))
        off = rng.choice([0, 1, 3])
        assert model(D.rle_decode, s, off, tile=11, group=2, piece=16, limit=LIMIT) == host_rle(s, off), (s, off)


def test_mtf_model_equals_host():
    rng = random.Random(5)
    for data in texts() + [bytes([255]) * 700, bytes(rng.randrange(256) for _ in range(3000))]:
        for chunk, group in ((1, 2), (16, 4), (1024, 256)):
            assert D.mtf_decode(data, chunk, group) == T.mtf_decode(data)
        assert D.mtf_decode(M.mtf_encode(data)) == data
    a, b, c = [D.mtf_chunk(bytes(rng.randrange(256) for _ in range(50)))[0] for _ in range(3)]
    assert bytes(D.compose(D.compose(a, b), c)) == bytes(D.compose(a, D.compose(b, c)))


def fib_text(k):
    """symbol i occurs fib(i) times: code lengths grow by one per symbol"""
    f, out = [1, 1], b""
    for i in range(k):
        out += bytes([65 + i]) * f[i]
        f.append(f[-1] + f[-2])
    return out


def test_huff_model_equals_host():
    rng = random.Random(9)
    cases = [b"", b"a", b"aaaa", b"ab", b"abab" * 9, bytes(range(256)), fib_text(18), T.gen_english(2000, 1).tobytes()]
    cases += [bytes(range(256)) + bytes(rng.randrange(256) for _ in range(600))]        # sigma = 256, mixed lengths
    cases += [d for _, d in corpus.small_corpus()]
    cases += [b"ab" * k + b"c" for k in range(1, 17)]                                   # the last code ends 0 .. 7 bits before the terminator
    for data in cases:
        s = O.huff_encode_literals(data)
        ok, got = host(T.huff_decode_literals, s)
        for tile, group in ((64, 4), (2048, 512)):
            assert model(D.huff_decode, s, tile, group) == (ok, got), data[:30]
        if ok and len(set(data)) < 256:
            assert got == data


def test_huff_malformed():
    hs = O.huff_encode_literals(b"hello world, hello")
    bits = "1" + "0" + format(2, "07b") + "0" + format(1, "07b") + "0" + format(0, "07b") + "0" + format(1, "07b") + format(65, "08b") + "11"
    bits += "0" * (-len(bits) % 8)
    kraft = int(bits, 2).to_bytes(len(bits) // 8, "big") + bytes([7])
    bad = [b"", hs[:1], hs[:4] + hs[-1:], b"\x80", b"\x06", b"\x07", b"\x00", b"\x01", kraft, hs[:-1], hs + b"\x00", hs + b"\x07"]
    rng = random.Random(2)
    base = O.huff_encode_literals(T.gen_english(300, 2).tobytes())
    for _ in range(250):
        s = bytearray(base)
        for _ in range(rng.randrange(1, 4)):
            s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
        bad.append(bytes(s[:rng.randrange(1, len(s) + 1)]) if rng.random() < 0.3 else bytes(s))
    for s in bad:
        assert model(D.huff_decode, s) == host(T.huff_decode_literals, s), s.hex()
