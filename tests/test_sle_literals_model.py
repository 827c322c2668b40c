"""CPU tests of the model of encode(sle) (tests/models/sle_literals.py).

The model is pinned to the committed oracle without a reference binary: the oracle writes lcpcomp(coder=sle) streams for a caller's
factor list, and with an EMPTY list that stream is the ranking, n in 32 bits, flen_min / flen_max / fdist_max in bits_for(n) bits (the
values 2^32 - 1 truncated, 0 and n), the bit 1, n in bits_for(n) bits and then the very symbol codes and flush of encode(sle)
(LZSSCoding.hpp:41-91 with no factor; every encode(v, Range) in front of the first literal flushes an empty buffer).  Built from the
model's own pieces, that stream must equal the oracle's byte for byte -- for every kmer and one alphabet size per sigma_bits class,
which fixes the ranking's tie order and all four class codes.  Then: hand-derived known answers, the round trip, and the device
formulation of the decoder against the plain loop on good and on damaged streams."""
import json
import os
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests.models import sle_literals as M
from tests.models.sle_decode import BitWriter, bits_for
from tests.util import factors_struct

HERE = os.path.dirname(os.path.abspath(__file__))
KMERS = (1, 2, 3, 4, 7)
ALPHABETS = (1, 2, 8, 9, 16, 17, 33, 64, 65, 129, 256)


def text_over(d, seed, n=None):
    """every one of the byte values 0 .. d - 1 at least once, skewed so that counts tie and differ, 0-terminated"""
    rng = np.random.default_rng(seed)
    n = n or 12 * d + 40
    body = (rng.integers(0, d, n, dtype=np.int64) * rng.integers(0, d, n, dtype=np.int64)) // max(d, 1)
    return bytes(range(d)) + body.astype(np.uint8).tobytes() + b"\x00"


def zero_factor_stream(text, k):
    symbols, sb = M.ranking_symbols(text, k)
    n, W = len(text), bits_for(len(text))
    w = BitWriter()
    M.header_bits(w, symbols)
    w.write(n, 32)
    w.write(0xFFFFFFFF & ((1 << W) - 1), W)
    w.write(0, W)
    w.write(n, W)
    w.write(1, 1)
    w.write(n, bits_for(n))
    val, bits = M.symbol_codes(text, k, symbols, sb)
    return M.finish(np.concatenate([np.array(w.bits, dtype=np.uint8), M.pack_bits(val, bits)]))


@pytest.mark.parametrize("k", KMERS)
def test_model_pieces_equal_the_oracle_on_an_empty_factor_list(k):
    none = np.zeros(0, dtype=np.uint32)
    classes = set()
    for d in ALPHABETS:
        text = text_over(d, 100 + d)
        want, _ = O.encode_sle(text, factors_struct(none, none, none), k)
        assert zero_factor_stream(text, k) == want, (k, d)
        classes.add(min(M.ranking_symbols(text, k)[1], 7))
    assert classes >= ({1, 3, 4, 5, 6, 7} if k == 1 else {4, 5, 6, 7})           # every class code is in play
    for text in (b"abc" * 50 + b"\x00", b"abcdefg" * 30 + b"\x00", b"a" * 100 + b"\x00", b"ab\x00", b"\x00"):
        want, _ = O.encode_sle(text, factors_struct(none, none, none), k)
        assert zero_factor_stream(text, k) == want, (k, text[:8])


def test_known_answers_derived_by_hand():
    kats = json.load(open(os.path.join(HERE, "golden", "sle_literal_kats.json")))
    assert "derived by hand" in kats["source"] and len(kats["cases"]) >= 2
    for c in kats["cases"]:
        data, stream = bytes.fromhex(c["data_hex"]), bytes.fromhex(c["stream_hex"])
        assert M.encode(data, c["kmer"]) == stream, c["note"]
        assert M.decode(stream, c["kmer"]) == data and M.decode_tiles(stream, c["kmer"], tile=16) == data
    assert M.encode(b"", 1) == M.encode(b"", 7) == b"\x00\x00"


def good_cases():
    out = [b"", b"a", b"ab", b"abc" * 700, b"abcdefg" * 301, b"\xff" * 50, bytes(range(256)) * 3]
    for d in ALPHABETS:
        out.append(text_over(d, d, 300))
    return out


@pytest.mark.parametrize("k", KMERS)
def test_round_trip_and_tiles_equal_the_plain_loop(k):
    for data in good_cases():
        z = M.encode(data, k)
        assert M.decode(z, k) == data, (k, data[:8])
        for tile, group in ((16, 3), (64, 2), (2048, 512)):
            assert M.decode_tiles(z, k, tile=tile, group=group) == data, (k, tile, data[:8])
    with pytest.raises(ValueError):
        M.encode(b"abc", 8)


def outcome(f, *a, **kw):
    try:
        return "ok", f(*a, **kw)
    except M.Malformed:
        return "malformed", None
    except M.TooLarge:
        return "too large", None


@pytest.mark.parametrize("k", (1, 3, 7))
def test_damaged_streams_tiles_refuse_what_the_plain_loop_refuses(k):
    rng = random.Random(k)
    seen = set()
    for data in (b"abracadabra" * 9, text_over(17, 5, 120), text_over(65, 6, 150), text_over(129, 7, 200)):
        z = M.encode(data, k)
        damaged = [z[:i] for i in range(0, len(z), max(1, len(z) // 60))]
        for _ in range(60):
            i = rng.randrange(len(z) * 8)
            damaged.append(z[:i >> 3] + bytes([z[i >> 3] ^ (0x80 >> (i & 7))]) + z[(i >> 3) + 1:])
        for s in damaged:
            want = outcome(M.decode, s, k)
            assert outcome(M.decode_tiles, s, k, tile=32, group=4) == want, (k, s.hex())
            seen.add(want[0])
    assert seen == {"ok", "malformed"}
    # every refusal by name
    with pytest.raises(M.Malformed):
        M.decode(b"", k)
    w = BitWriter(); w.compressed_int(1025)
    assert outcome(M.decode, w.finish(), k)[0] == "malformed"                   # sigma > 1024
    w = BitWriter(); w.compressed_int(2); w.compressed_int(0x61)
    assert outcome(M.decode, w.finish(), k)[0] == "malformed"                   # the ranking runs off the end
    w = BitWriter(); w.compressed_int(1); w.compressed_int(0x161)
    assert outcome(M.decode, w.finish(), k)[0] == "malformed"                   # neither a byte nor a k-mer
    if k < 7:
        w = BitWriter(); w.compressed_int(1); w.compressed_int(M.MARK | (1 << (8 * k)))
        assert outcome(M.decode, w.finish(), k)[0] == "malformed"               # a k-mer of another k
    w = BitWriter(); M.header_bits(w, [0x61, 0x62, 0x63]); w.write(3, 2)
    for f in (M.decode, M.decode_tiles):
        assert outcome(f, w.finish(), k)[0] == "malformed"                      # rank 3 >= sigma 3
    w = BitWriter(); M.header_bits(w, list(range(17))); w.write(1, 1); w.write(16, 5); w.write(1, 1); w.write(0, 2)
    for f in (M.decode, M.decode_tiles):
        assert outcome(f, w.finish(), k)[0] == "malformed"                      # 1 + 5 bits wanted, 3 left
    w = BitWriter(); M.header_bits(w, [M.MARK | 0x61] if k == 7 else [0x61, 0x62]); w.write(0, 40)
    for f in (M.decode, M.decode_tiles):
        assert outcome(f, w.finish(), k, limit=39)[0] == "too large" and outcome(f, w.finish(), k, limit=40 * (7 if k == 7 else 1))[0] == "ok"
