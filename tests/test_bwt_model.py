"""CPU tests of the numpy model of the bwt compressor (tests/models/bwt.py): the forward transform against the reference's
known-answer test, the device formulation of the inverse (LF, hashed heads, bounded walks, head ranking, second walk, validation)
against the plain loop, and the `C[255]` behaviour of the loop as the reference wrote it."""
import json
import os
import random

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.models import bwt as M

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "reference_kats.json")))


def forward(text):
    return M.bwt_from_sa(text, O.suffix_array(text))


def check(text, samples=(1, 2, 7, 64), steps=(0, 1, 3)):
    b = forward(text)
    if len(text) <= 1:                                   # decode_bwt: an input of at most one byte decodes to nothing
        text = b""
    assert M.inverse_loop(b) == text
    for s in samples:
        for m in steps:
            st = {}
            assert M.inverse_device(b, s, m, st) == text, (s, m)
            if m == 1 and len(text) > 1:
                assert st["heads"] == len(text) and st["longest"] == 1       # every row became a head


@pytest.mark.parametrize("k", KATS["bwt"], ids=lambda k: k["source"][:24])
def test_forward_matches_the_reference_kat(k):
    text = bytes.fromhex(k["text_hex"])
    want = bytes.fromhex(k["bwt_hex"])
    assert M.bwt_forward(text) == want
    assert forward(text) == want
    check(text)
    assert M.inverse_loop(want, reference_bug=True) == text          # no 0xFF in it: the reference's own table is right here


def test_mix_is_a_bijection_with_a_fixed_zero():
    for n in (2, 3, 5, 17, 64, 65, 1000, 4097):
        m, mask, _ = M.mix_params(n)
        img = [M.mix(i, n) for i in range(mask + 1)]
        assert sorted(img) == list(range(mask + 1)) and img[0] == 0
        assert all(M.unmix(M.mix(i, n), n) == i for i in range(mask + 1))


@pytest.mark.parametrize("name,data", [c for c in corpus.small_corpus() if len(c[1]) <= 6000], ids=lambda v: v if isinstance(v, str) else "")
def test_small_corpus(name, data):
    check(T.escape(data), samples=(1, 7, 64), steps=(0, 1))


def test_random_texts():
    for name, data in corpus.random_small(200, 77):
        check(T.escape(data), samples=(2, 64), steps=(0, 1, 5))


@pytest.mark.parametrize("text", [b"a" * 777 + b"\0", b"ab" * 400 + b"\0", corpus.fib_word(14) + b"\0", corpus.thue_morse(10) + b"\0",
                                  T.escape(b"\xff\x00\xff\xff\x00ab\xfe" * 40), T.escape(bytes(range(256)) * 2), b"\0", b"x\0"],
                         ids=["a^k", "(ab)^k", "fib", "thue", "escapes", "all_bytes", "sentinel_only", "one_byte"])
def test_structured_texts(text):
    check(text)


def test_tiny_inputs_decode_to_nothing():
    assert M.inverse_device(b"") == b"" and M.inverse_device(b"\0") == b"" and M.inverse_device(b"a") == b""
    assert M.inverse_loop(b"") == b"" and M.inverse_loop(b"q") == b""


def two_cycles():
    """a buffer with exactly one 0 whose LF permutation has a second cycle: 'ba\\0' has LF = (1 2 0)(...)"""
    rng = random.Random(5)
    while True:
        b = bytes(rng.randrange(1, 4) for _ in range(11)) + b"\0"
        b = bytes(rng.sample(list(b), len(b)))
        lf = M.lf_table(b)
        seen, i = 0, 0
        while True:
            i = int(lf[i]); seen += 1
            if i == 0:
                break
        if seen < len(b):
            return b


@pytest.mark.parametrize("s,m", [(1, 0), (2, 1), (7, 3), (64, 0)])
def test_malformed_inputs_are_refused(s, m):
    good = forward(T.escape(b"mississippi river"))
    for bad in (good.replace(b"\0", b"x"), good[:3] + b"\0" + good[3:], two_cycles(), bytes([7, 7, 0, 7, 0, 9])):
        with pytest.raises(M.Malformed):
            M.inverse_device(bad, s, m)
    assert M.inverse_device(good, s, m) == T.escape(b"mississippi river")


def test_reference_table_breaks_on_0xff():
    """compute_LF (ds/bwt.hpp:38) leaves C[255] unaccumulated: its walk does not invert a text that holds 0xFF"""
    text = b"ab\xff\xfecd\xff\xffab\xfe\xfe\0"
    b = forward(text)
    assert b.hex() == "feff006161fe63feff62ff6264"
    assert M.inverse_loop(b) == text and M.inverse_device(b, 2, 3) == text
    assert M.inverse_loop(b, reference_bug=True) != text
    plain = T.escape(b"no such byte in here")
    assert M.inverse_loop(forward(plain), reference_bug=True) == plain
