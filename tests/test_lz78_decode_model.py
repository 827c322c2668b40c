"""CPU tests: the device formulation of the lz78(coder=gamma) decoder (tests/models/lz78_decode.py: next() of every bit, orbit of
bit 0, pairs side by side, lengths by pointer jumping, factor list, references by pointer jumping) reproduces the input of the
oracle's streams, and rejects malformed streams."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import corpus
from tests.coder_borders import LZ78_COUNTS, phrase_prefixes, residue, two_letters_64k
from tests.models import lz78_decode as M


def _ascii_tail(data):
    """the reference writes a left-over phrase that ends in a byte >= 0x80 as a sign-extended char: keep it ASCII"""
    return data if not data or data[-1] < 0x80 else data + b"."


def _small_cases():
    return [(name, _ascii_tail(d)) for name, d in corpus.small_corpus() if len(d) <= 3000]


@pytest.mark.parametrize("name,data", _small_cases(), ids=lambda x: x if isinstance(x, str) else "")
def test_model_round_trip_corpus(name, data):
    stream = O.lz78_gamma_compress(data)
    assert M.decode(stream) == data


def test_model_round_trip_random_small():
    for _, data in corpus.random_small(300, 78):
        data = _ascii_tail(data)
        assert M.decode(O.lz78_gamma_compress(data)) == data


def test_model_segments_and_all_bytes():
    rng = random.Random(5)
    data = bytes(rng.randrange(256) for _ in range(1500)) + bytes(range(256)) + b"!"
    stream = O.lz78_gamma_compress(data)
    for seg in (64, 97, 1000, 1 << 30):                # segments much shorter than the stream: exits become entries
        assert M.decode(stream, seg=seg) == data


def test_model_pairs_and_lengths_match_the_parse():
    data = b"abracadabra" * 40 + b"a" * 300
    ids, chars = M.parse_pairs(O.lz78_gamma_compress(data))
    want_ids, want_chars = O.lz78_factors(data)
    assert list(ids) == [int(x) for x in want_ids] and bytes(chars) == bytes(want_chars)
    lengths, rounds = M.phrase_lengths(ids)
    assert int(lengths.sum()) == len(data)
    assert rounds <= int(np.ceil(np.log2(lengths.max()))) + 1


def test_model_empty_and_one_byte():
    assert M.decode(O.lz78_gamma_compress(b"")) == b""
    assert M.decode(b"") == b""
    assert M.decode(O.lz78_gamma_compress(b"x")) == b"x"


def test_model_sign_extended_leftover():
    w = M.BitWriter()
    w.pair(0, ord("a"))
    w.pair(0, ord("b"))
    w.pair(1, 0xFFFFFFFFFFFFFF80)                      # the reference's left-over (parent 1 = "a", char (int8)0x80 as u64)
    assert M.decode(w.finish()) == b"ab" + b"a\x80"


def _malformed_streams():
    out = {}
    good = O.lz78_gamma_compress(b"abcabcabcabd" * 4)
    bits, total = M.stream_bits(good)
    w = M.BitWriter()                                   # the same pairs, the last one cut off by one bit
    w.bits = [int(b) for b in bits[:total - 1]]
    out["truncated"] = w.finish()
    w = M.BitWriter()
    w.pair(0, 97)
    w.pair(2, 98)                                       # pair 1 names phrase 2: not there yet
    out["id_ahead"] = w.finish()
    w = M.BitWriter()
    w.pair(0, 97)
    w.pair(1, 98, id_width=33)                          # id field of 33 bits
    out["id_33_bits"] = w.finish()
    return out


@pytest.mark.parametrize("kind", ["truncated", "id_ahead", "id_33_bits"])
def test_model_rejects_malformed(kind):
    with pytest.raises(M.Malformed):
        M.decode(_malformed_streams()[kind])


def _outcome(fn, stream):
    try:
        return fn(stream)
    except M.Malformed:
        return None


def test_model_random_streams_match_the_sequential_reading():
    """random byte strings: the orbit / segment formulation accepts exactly the streams the sequential reading accepts, and decodes
    them to the same text (short streams, so that a fair share of them are valid pair sequences; segments shorter than a pair too)"""
    rng = random.Random(11)
    accepted = rejected = 0
    for i in range(400):
        if i % 2:
            s = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 13)))
        else:                                           # random pair sequences, some ids ahead, some bits flipped
            w = M.BitWriter()
            for k in range(rng.randrange(1, 9)):
                w.pair(rng.randrange(0, k + 2), rng.choice((rng.randrange(256), rng.randrange(1 << 64))))
            if rng.random() < 0.3:
                j = rng.randrange(len(w.bits))
                w.bits[j] ^= 1
            s = w.finish()
        want = _outcome(M.sequential_decode, s)
        for seg in (1 << 30, 16, 5):
            assert _outcome(lambda t: M.decode(t, seg=seg), s) == want, (s.hex(), seg)
        if want is None:
            rejected += 1
        else:
            accepted += 1
    assert accepted >= 30 and rejected >= 30


def test_model_sequential_reading_matches_the_oracle():
    for _, data in corpus.random_small(50, 79):
        data = _ascii_tail(data)
        assert M.sequential_decode(O.lz78_gamma_compress(data)) == data


def test_model_oversized_claim_is_found_before_the_text():
    # pair k extends phrase k (id k): len_k = k + 1, 93 000 pairs claim ~4.3e9 bytes
    ids = np.arange(93000, dtype=np.int64)
    lengths, rounds = M.phrase_lengths(ids)
    assert int(lengths.sum()) > M.MAX_TEXT and rounds <= 18
    with pytest.raises(M.TooLarge):
        M.factor_list(ids, lengths)


def test_coder_border_inputs():
    """what tests/test_gpu_parity.py relies on: a prefix that ends where phrase k ends parses into k pairs.  A pair is two gamma codes of
    odd length, so no stream ends with 5 bits in its last byte; the far side of the terminator rule, 6, is among the prefixes."""
    text = two_letters_64k()
    lengths = M.phrase_lengths(O.lz78_factors(text)[0].astype(np.int64))[0]
    residues = set()
    for k, prefix in phrase_prefixes(text, lengths, LZ78_COUNTS):
        assert len(O.lz78_factors(prefix)[0]) == k
        residues.add(residue(O.lz78_gamma_compress(prefix)))
    assert 6 in residues and all(r % 2 == 0 for r in residues)
