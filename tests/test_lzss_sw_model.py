"""CPU tests of the lzss model (tests/models/lzss_sw.py): the literal restatement of the reference's sliding-buffer loop and the closed
form the library implements yield the same tokens; the token coders against hand-derived bit strings; decode inverts encode."""
import pytest

from tests.models import lzss_sw as M
from tests.models.lzss_coders import bits_for, terminate
from tests.util import load_json

WINDOWS, sweep = M.WINDOWS, M.sweep


def test_closed_form_equals_reference_loop():
    longest = {w: 0 for w in WINDOWS}
    trunc = set()
    cases = 0
    for data, w, t in sweep(20261019, 4000):
        toks = M.parse(data, w, t)
        assert toks == M.reference_loop(data, w, t), (data, w, t)
        assert sum(1 if s is None else j for _, s, j in toks) == len(data)
        for _, s, j in toks:
            if s is not None:
                longest[w] = max(longest[w], j)
        if M.truncates(data, w, t):
            trunc.add(w)
        cases += 1
    assert cases == 4000
    assert all(longest[w] == 2 * w - 1 for w in WINDOWS if w > 1), longest      # longer than the window
    assert {3, 5} <= trunc                                                       # no power of two: 2w - 1 >= 2^bits_for(w)
    assert not trunc & {1, 2, 4, 8, 16}


def test_threshold_zero_is_one_and_empty_input():
    for data, w, _ in sweep(7, 200):
        assert M.parse(data, w, 0) == M.parse(data, w, 1)
    for w in WINDOWS:
        assert M.parse(b"", w, 3) == M.reference_loop(b"", w, 3) == []
    for coder in M.CODERS:
        assert M.encode([], coder, 16) == b"\x00"
        assert M.decode(b"\x00", coder) == b"" and M.decode(b"", coder) == b""


def test_smallest_source_among_the_longest_wins():
    # "ab" occurs at 0 and 3 in front of p = 6: both match 2 bytes, the reference's strict `>` keeps source 0
    assert M.parse(b"abxabyab", 16, 2)[-1] == (6, 0, 2) == M.reference_loop(b"abxabyab", 16, 2)[-1]


def test_truncating_example():
    toks = M.parse(b"aaaaaaaa", 3, 3)
    assert toks == M.reference_loop(b"aaaaaaaa", 3, 3)
    assert M.truncates(b"aaaaaaaa", 3, 3) and max(j for _, s, j in toks if s is not None) >= 1 << bits_for(3)
    assert M.decode(M.encode(toks, "bit", 3), "bit", 3) != b"aaaaaaaa"           # the reference's own decoder yields another text
    for coder in ("gamma", "delta", "ascii"):
        assert M.decode(M.encode(toks, coder, 3), coder, 3) == b"aaaaaaaa"


def test_hand_derived_bit_strings():
    k = load_json("lzss_sw_kats.json")
    text, w, t = k["text"].encode(), k["window"], k["threshold"]
    toks = M.parse(text, w, t)
    assert toks == [tuple(x) for x in k["tokens"]]
    for coder, bits in k["bits"].items():
        assert M.encode_bits(toks, coder, w) == bits.replace(" ", ""), coder
        assert M.encode(toks, coder, w) == terminate(bits.replace(" ", ""))
    assert M.encode(toks, "ascii", w) == k["ascii_text"].encode() + b"\x00"
    for coder, hx in k["stream_hex"].items():
        assert M.encode(toks, coder, w).hex() == hx, coder
    for coder in M.CODERS:
        assert M.decode(M.encode(toks, coder, w), coder, w) == text


@pytest.mark.parametrize("coder", M.CODERS)
def test_decode_inverts_encode(coder):
    for data, w, t in sweep(99, 600):
        if coder == "bit" and M.truncates(data, w, t):
            continue
        assert M.decode(M.encode(M.parse(data, w, t), coder, w), coder, w) == data, (data, w, t)


def test_decode_refusals():
    with pytest.raises(M.Malformed):                    # distance 0
        M.decode(M.encode([(0, None, 97), (1, 1, 2)], "gamma", 16), "gamma")
    with pytest.raises(M.Malformed):                    # a distance above the text so far
        M.decode(M.encode([(0, None, 97), (1, -1, 2)], "gamma", 16), "gamma")
    bits = M.encode_bits(M.parse(b"abcabcabc", 16, 3), "bit", 16)
    with pytest.raises(M.Malformed):                    # the last token cut off
        M.decode(terminate(bits[:-3]), "bit")
    with pytest.raises(M.TooLarge):                     # a^(2^32 - 1)
        M.decode(M.encode([(0, None, 97), (1, 0, M.TEXT_MAX)], "gamma", 16), "gamma")
    assert M.decode(M.encode([(0, None, 97), (1, 0, 0)], "gamma", 16), "gamma") == b"a"      # length 0 decodes to nothing
