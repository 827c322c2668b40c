"""CPU tests: the device formulation of the lcpcomp(coder=sle) parse (tests/models/sle_decode.py: next() of every bit position, orbit
of the first token start, tokens side by side, segments, references by pointer jumping) decodes the oracle's SLE streams back to
the text, and pins the three points where the SLE token differs from the Huffman one -- the k-mer cut at the end of a run, the
classes of the length field, eof() inside a k-mer -- before any kernel is involved."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import corpus, factor_lists as FL
from tests.models import sle_decode as M
from tests.util import factors_struct

KMERS = (1, 2, 3, 5, 7)


def _small_cases():
    return [(name, d) for name, d in corpus.small_corpus() if len(d) <= 1500]


@pytest.mark.parametrize("name,data", _small_cases(), ids=lambda x: x if isinstance(x, str) else "")
def test_model_round_trip_corpus(name, data):
    text = O.escape(data)
    for k in KMERS:
        for thr, fl in ((2, 1), (5, 0)):
            stream, _ = O.lcpcomp_sle_compress(text, thr, fl, k)
            if len(stream) > 1200:
                continue                                   # (next() of every bit in pure Python)
            assert M.decode(stream, k) == text, (k, thr, fl)
            assert M.sequential_decode(stream, k) == text


def test_model_round_trip_random_small():
    rng = random.Random(11)
    for name, data in corpus.random_small(120, 41):
        text = O.escape(data[:300])
        k = rng.choice(KMERS)
        thr = rng.randrange(1, 6)
        stream, _ = O.lcpcomp_sle_compress(text, thr, rng.randrange(2), k)
        seg = rng.choice((37, 64, 501, 1 << 30))           # segments far shorter than the stream: exits become entries
        assert M.decode(stream, k, seg=seg) == text, (name, k, thr, seg)


LISTS = (("no_factors", 1, {}), ("no_factors", 2, {}), ("no_factors", 200, {}), ("one_literal", 3, {}), ("one_literal", 700, {}),
         ("one_literal_len1", 400, {}), ("equal_lengths", 600, {"flen": 1}), ("equal_lengths", 600, {"flen": 2}),
         ("equal_lengths", 3000, {"flen": 255}), ("extreme_sources", 1000, {"p0": 0}), ("random_mix", 1 << 10, {}))


@pytest.mark.parametrize("shape,n,kw", LISTS, ids=["%s-n%d%s" % (s, n, "".join("-%s%s" % i for i in kw.items())) for s, n, kw in LISTS])
def test_model_decodes_hand_shaped_factor_lists(shape, n, kw):
    text, pos, src, length = FL.make_case(shape, n, seed=3, **kw)
    f = factors_struct(pos, src, length)
    for k in KMERS:
        stream, _ = O.encode_sle(text, f, k)
        assert O.lcpcomp_sle_decompress(stream, k) == text
        bits = M.Bits(stream)
        seg = max(16, bits.total // 7)
        assert M.decode(stream, k, seg=seg) == text, k
        H, tokens = M.parse_tokens(stream, k, seg=seg)
        assert [t[2] for t in tokens if t[2]] == [int(x) for x in length]
        assert [t[1] for t in tokens if t[2]] == [int(x) for x in src]


def _header(w, k, ranking, n, flen_min, flen_max, fdist_max):
    w.compressed_int(len(ranking))
    for e in ranking:
        w.compressed_int(e if isinstance(e, int) else (0xFF << 56) | int.from_bytes(e, "big"))
    W = M.bits_for(n)
    w.write(n, 32); w.write(flen_min, W); w.write(flen_max, W); w.write(fdist_max, W)
    return W, M.bits_for(flen_max - flen_min), M.bits_for(fdist_max)


def test_kmer_is_cut_at_the_end_of_a_run():
    """a run of 4 literals written as two 3-mers: the second yields one byte, its other two are dropped, a factor follows"""
    k = 3
    w = M.BitWriter()
    W, lbits, dbits = _header(w, k, [b"abc", ord("x"), 0], n=8, flen_min=3, flen_max=3, fdist_max=4)       # sigma 3: 2 plain rank bits
    w.write(1, 1); w.write(4, dbits); w.write(0, 2); w.write(0, 2)                                           # abc a|bc
    w.write(0, W); w.write(0, lbits)                                                                         # factor (src 0, len 3)
    w.write(1, 1); w.write(1, dbits); w.write(2, 2)                                                          # the sentinel
    stream = w.finish()
    want = b"abcaabc\0"
    assert O.lcpcomp_sle_decompress(stream, k) == want
    assert M.sequential_decode(stream, k) == want
    for seg in (5, 1 << 30):
        assert M.decode(stream, k, seg=seg) == want
    H, tokens = M.parse_tokens(stream, k)
    assert tokens[0] == (b"abca", 0, 3) and tokens[1] == (b"\0", 0, 0)


def test_length_field_classes():
    """lbits > 5: a 2-bit class, then 3 / 3 / 4 / lbits bits (values 0..7, 8..15, 16..31, anything)"""
    k = 1
    values = (0, 7, 8, 15, 16, 31, 32, 100)
    n = 1 + sum(2 + v for v in values) + 1
    w = M.BitWriter()
    W, lbits, dbits = _header(w, k, [ord("a"), 0], n=n, flen_min=2, flen_max=102, fdist_max=1)
    assert lbits == 7
    w.write(1, 1); w.write(1, dbits); w.write(0, 1)                                                          # 'a'
    first = True
    for v in values:
        if not first:
            w.write(0, 1)                                                                                    # no literals
        first = False
        w.write(0, W)
        if v < 8:
            w.write(0, 2); w.write(v, 3)
        elif v < 16:
            w.write(1, 2); w.write(v - 8, 3)
        elif v < 32:
            w.write(2, 2); w.write(v - 16, 4)
        else:
            w.write(3, 2); w.write(v, lbits)
    w.write(1, 1); w.write(1, dbits); w.write(1, 1)
    stream = w.finish()
    want = b"a" * (n - 1) + b"\0"
    assert O.lcpcomp_sle_decompress(stream, k) == want
    H, tokens = M.parse_tokens(stream, k, seg=29)
    assert [t[2] for t in tokens] == [2 + v for v in values] + [0]
    assert M.decode(stream, k, seg=29) == want
    # lbits <= 5: plain bits
    w = M.BitWriter()
    W, lbits, dbits = _header(w, k, [ord("a"), 0], n=1 + 33 + 1, flen_min=2, flen_max=33, fdist_max=1)
    assert lbits == 5
    w.write(1, 1); w.write(1, dbits); w.write(0, 1); w.write(0, W); w.write(31, lbits); w.write(1, 1); w.write(1, dbits); w.write(1, 1)
    stream = w.finish()
    assert M.decode(stream, k) == O.lcpcomp_sle_decompress(stream, k) == b"a" * 34 + b"\0"


def test_eof_inside_a_kmer():
    """the last run ends inside a k-mer: eof() is false there, so a factor is read all the same -- from the zeros behind the end.
    The sequential parser accepts the stream if that phantom factor (src 0, length flen_min) completes the text, and so do the model
    and the oracle; where it does not, all of them refuse."""
    k = 3
    for n, ok in ((4, True), (5, False)):
        w = M.BitWriter()
        W, lbits, dbits = _header(w, k, [b"ab\0", ord("x")], n=n, flen_min=2, flen_max=2, fdist_max=2)      # sigma 2: 1 rank bit
        w.write(1, 1); w.write(2, dbits); w.write(0, 1)                                                      # "ab" of ab\0, cut; the stream ends
        stream = w.finish()
        if ok:
            want = b"abab"
            assert O.lcpcomp_sle_decompress(stream, k) == want
            assert M.sequential_decode(stream, k) == want
            assert M.decode(stream, k) == want
            assert M.parse_tokens(stream, k)[1] == [(b"ab", 0, 2)]
        else:
            with pytest.raises(RuntimeError):
                O.lcpcomp_sle_decompress(stream, k)
            for dec in (M.sequential_decode, M.decode):
                with pytest.raises(M.Malformed):
                    dec(stream, k)
    # the same run with the k-mer used up: the stream ends there, no factor
    w = M.BitWriter()
    W, lbits, dbits = _header(w, k, [b"ab\0", ord("x")], n=3, flen_min=2, flen_max=2, fdist_max=3)
    w.write(1, 1); w.write(3, dbits); w.write(0, 1)
    stream = w.finish()
    assert M.decode(stream, k) == M.sequential_decode(stream, k) == O.lcpcomp_sle_decompress(stream, k) == b"ab\0"


def _oracle_outcome(stream, k):
    try:
        return O.lcpcomp_sle_decompress(stream, k)
    except RuntimeError:
        return None


@pytest.mark.parametrize("k", (1, 3, 7))
def test_damaged_streams(k):
    """truncated and bit-flipped streams: refused, or decoded to what the oracle's decoder returns; the model and the sequential
    restatement agree on every one of them"""
    text = O.escape(b"she sells sea shells by the sea shore; the shells she sells are sea shells " * 3)
    good, _ = O.lcpcomp_sle_compress(text, 2, 1, k)
    assert M.decode(good, k) == text
    rng = np.random.default_rng(17 + k)
    damaged = []
    for _ in range(60):
        bad = bytearray(good)
        bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        damaged.append(bytes(bad))
    damaged += [good[:c] for c in range(0, len(good), max(1, len(good) // 25))] + [good[:-1], good[:-2], b"\x00"]
    refused = 0
    for i, bad in enumerate(damaged):
        outcome = []
        for dec in (M.decode, M.sequential_decode):
            try:
                outcome.append(dec(bad, k))
            except M.Malformed:
                outcome.append(None)
        assert outcome[0] == outcome[1], i
        if outcome[0] is None:
            refused += 1
        else:
            assert outcome[0] == _oracle_outcome(bad, k), i
    assert refused > 0
