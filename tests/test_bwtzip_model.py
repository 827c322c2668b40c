"""CPU tests of the model behind rle, mtf and encode(huff) (tests/models/bwtzip.py) and of the host decoders of the C ABI
(tdc_rle_decode, tdc_mtf_decode, tdc_huff_decode_literals): the vectors of the reference's rle loop, the chunk-summary formulation of
mtf the device kernels use, round trips, and malformed input."""
import random

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.models import bwtzip as M

# input -> output of the reference's rle_encode loop over std::stringstream (g++, libstdc++, x86-64: signed char); the last input makes
# that loop run for ever -- ours ends it with what a 0xFF in mid-stream emits
RLE_VECTORS = [(b"\x61" * 5, "616103"), (b"\x61" * 5 + b"\x62", "61610362"), (b"\x80" * 5, "808000800080008000"),
               (b"\xff" * 3 + b"\x62", "ffff00ff0062"), (b"\x62\xff", "62ff"), (b"\x61" * 300, "6161aa02"), (b"\x62\xff\xff", "62ffff00")]


def inputs():
    rng = random.Random(7)
    out = [d for _, d in corpus.small_corpus() + corpus.random_small(60, 99)]
    out += [b"", b"a", b"aaaa", b"\xff", bytes(range(256)) * 5, corpus.run_rich(3000, rng), T.gen_english(5000, 3).tobytes()]
    out += [bytes(rng.choice([0x61, 0x7F, 0x80, 0xFF, 0x00]) for _ in range(rng.randrange(1, 300))) for _ in range(60)]
    out += [bytes(rng.randrange(256) for _ in range(2000))]
    return out


def test_rle_vectors():
    for data, want in RLE_VECTORS:
        assert M.rle_encode(data).hex() == want
        assert M.rle_encode_np(data).hex() == want
        assert M.rle_decode(bytes.fromhex(want)) == data
        assert T.rle_decode(bytes.fromhex(want)) == data


def test_vbyte():
    for v, want in ((0, "00"), (127, "7f"), (128, "8001"), (298, "aa02"), (1 << 63, "80" * 9 + "01")):
        assert M.vbyte(v).hex() == want and M.read_vbyte(bytes.fromhex(want), 0) == (v, len(want) // 2)


def test_round_trips_and_host_decoders():
    for data in inputs():
        for off in (0, 1, 200, 1 << 33):
            e = M.rle_encode(data, off)
            assert e == M.rle_encode_np(data, off)
            assert M.rle_decode(e, off) == data and T.rle_decode(e, off) == data
        m = M.mtf_encode(data)
        assert len(m) == len(data) and M.mtf_decode(m) == data and T.mtf_decode(m) == data
        if len(set(data)) < 256:            # (256 symbols of one length: the reference's u8 length counters wrap, its own decoder fails)
            assert T.huff_decode_literals(O.huff_encode_literals(data)) == data


@pytest.mark.parametrize("chunk", [1, 2, 7, 256, 4096])
def test_mtf_by_chunk_summaries(chunk):
    rng = random.Random(chunk)
    texts = [bytes(rng.randrange(256) for _ in range(9000)), corpus.run_rich(9000, rng), bytes(range(256)) * 36,
             bytes(reversed(range(256))) * 20 + b"zzz", b"", b"q"] + [d for _, d in corpus.small_corpus()]
    for data in texts:
        assert M.mtf_encode_chunked(data, chunk) == M.mtf_encode(data)
    a, b, c = [M.chunk_summary(bytes(rng.randrange(40) for _ in range(30))) for _ in range(3)]
    assert M.compose(M.compose(a, b), c) == M.compose(a, M.compose(b, c))


def refused(fn, *args):
    with pytest.raises(T.TdcGpuError) as e:
        fn(*args)
    assert e.value.status == -2
    return True


def test_host_decoders_refuse_malformed_input():
    assert refused(T.rle_decode, b"aa")                               # the vbyte runs off the end
    assert refused(T.rle_decode, b"aa\x80\x80")
    assert refused(T.rle_decode, b"aa" + b"\x80" * 10 + b"\x01")     # longer than ten bytes
    assert refused(T.rle_decode, b"aa\x02", 3)                        # vbyte < offset
    hs = O.huff_encode_literals(b"hello world, hello")
    assert refused(T.huff_decode_literals, b"")                       # no header
    assert refused(T.huff_decode_literals, hs[:1])                    # header cut off
    assert refused(T.huff_decode_literals, hs[:4] + hs[-1:])
    assert refused(T.huff_decode_literals, b"\x80")
    # a table that leaves codes unassigned: longest 2, numl = (1, 0), sigma 1 -> the code 11 is outside the table
    bits = "1" + "0" + format(2, "07b") + "0" + format(1, "07b") + "0" + format(0, "07b") + "0" + format(1, "07b") + format(65, "08b") + "11"
    bits += "0" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big")
    assert refused(T.huff_decode_literals, raw + bytes([7]))
    # nothing is written past out_cap, and a text that does not fit is refused
    import ctypes
    L = T._native.load()
    e = np.frombuffer(M.rle_encode(b"a" * 1000), dtype=np.uint8)
    out = np.full(64, 0xA5, dtype=np.uint8)
    n = ctypes.c_size_t()
    rc = L.tdc_rle_decode(e.ctypes.data_as(ctypes.c_void_p), len(e), 0, out.ctypes.data_as(ctypes.c_void_p), 16, ctypes.byref(n))
    assert rc == -2 and n.value == 1000 and bool((out[16:] == 0xA5).all()) and out[:16].tobytes() == b"a" * 16
    bomb = np.frombuffer(b"aa" + b"\xff" * 9 + b"\x01", dtype=np.uint8)          # a run of 2^64 - 1
    rc = L.tdc_rle_decode(bomb.ctypes.data_as(ctypes.c_void_p), len(bomb), 0, out.ctypes.data_as(ctypes.c_void_p), 16, ctypes.byref(n))
    assert rc == -2 and bool((out[16:] == 0xA5).all())
    m = np.frombuffer(M.mtf_encode(b"hello" * 10), dtype=np.uint8)
    rc = L.tdc_mtf_decode(m.ctypes.data_as(ctypes.c_void_p), len(m), out.ctypes.data_as(ctypes.c_void_p), 16, ctypes.byref(n))
    assert rc == -2 and n.value == 50 and bool((out[16:] == 0xA5).all())
