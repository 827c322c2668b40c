"""CPU tests of the repair model (tests/models/repair.py): the literal restatement of the reference's rounds against hand-derived
grammars, the device formulation (table, deltas, tie pass, compaction) against that restatement, and the coders."""
import itertools

import numpy as np
import pytest

from tests.coder_borders import repair_borders, residue
from tests.models import repair as M
from tests.models.lzss_coders import terminate
from tests.util import load_json

MAX_RULES = (0, 1, 2, 7)


def same(data):
    for mr in MAX_RULES:
        want = M.grammar(data, mr)
        for recount in (False, True):
            assert M.device_grammar(data, mr, recount) == want, (data[:40], len(data), mr, recount)
    return M.grammar(data, 0)


def expand(rules, start):
    out = bytearray()
    stack = list(reversed(start))
    while stack:
        x = stack.pop()
        if x < 256:
            out.append(x)
        else:
            stack.extend(reversed(rules[x - 256]))
    return bytes(out)


def fibonacci_word(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def thue_morse(n):
    return bytes(ord("a") + (bin(i).count("1") & 1) for i in range(n))


def test_hand_derived_grammars_and_streams():
    k = load_json("repair_kats.json")
    assert [c["text"] for c in k["cases"]] == ["abcdcdab", "aaa", "aaaaa", "ababab", "xaaay"]
    for c in k["cases"]:
        text = c["text"].encode()
        rules, start = M.grammar(text)
        assert rules == [tuple(x) for x in c["rules"]] and start == c["start"], c["text"]
        assert M.device_grammar(text) == (rules, start)
        bits = c["bit"].replace(" ", "")
        assert M.encode_bits(rules, start, "bit") == bits, c["text"]
        assert M.encode(rules, start, "bit") == terminate(bits) == M.encode_fields(rules, start)
        assert M.encode(rules, start, "ascii") == c["ascii"].encode() + b"\x00", c["text"]
        for coder in M.CODERS:
            assert M.sequential_decode(M.encode(rules, start, coder), coder) == text


def test_the_winner_is_the_pair_that_reaches_the_count_first():
    rules, start = M.grammar(b"abcdcdab")
    assert rules[0] == (ord("c"), ord("d"))                       # not the pair that occurs first
    assert M.grammar(b"abcdcdab", 1) == ([(99, 100)], [97, 98, 256, 256, 97, 98])


def test_empty_and_single():
    assert M.grammar(b"") == M.device_grammar(b"") == ([], [])
    assert M.grammar(b"q") == M.device_grammar(b"q") == ([], [ord("q")])
    for coder in M.CODERS:
        assert M.sequential_decode(M.compress(b"", coder), coder) == b""
        assert M.sequential_decode(M.compress(b"q", coder), coder) == b"q"
    assert M.compress(b"", "bit") == b"\x00\x00\x00\x00\x00"      # 32 bits of 0 and the terminator
    assert M.compress(b"", "ascii") == b"0:\x00"


def test_runs():
    for k in range(71):
        rules, start = same(b"a" * k)
        assert expand(rules, start) == b"a" * k
    assert M.grammar(b"aaa") == ([(97, 97)], [256, 97])           # left-greedy: the count was 2, one pair goes
    stats = M.DeviceStats()
    M.device_grammar(b"a" * 70, stats=stats)
    assert stats.rounds == 5 and stats.replaced == 35 + 17 + 8 + 4 + 2      # the last (E,E) counts 1


def test_two_letter_runs():
    for i in range(13):
        for j in range(13):
            same(b"a" * i + b"b" * j)
            same(b"a" * i + b"b" * j + b"a" * i)


def test_all_short_strings_over_three_letters():
    ties = M.DeviceStats()
    for n in range(9):
        for t in itertools.product(b"abc", repeat=n):
            data = bytes(t)
            want = M.grammar(data, 0)
            assert M.device_grammar(data, 0, False, ties) == want, data
            assert expand(*want) == data
            for mr in MAX_RULES[1:]:
                assert M.device_grammar(data, mr) == M.grammar(data, mr), (data, mr)
    assert ties.tie_rounds > 1000


@pytest.mark.parametrize("word", [fibonacci_word, thue_morse])
def test_fibonacci_and_thue_morse_words(word):
    for n in (1, 2, 3, 5, 8, 13, 21, 100, 1000, 4096):
        rules, start = same(word(n))
        assert expand(rules, start) == word(n)


@pytest.mark.parametrize("sigma", [2, 4, 256])
def test_random_texts(sigma):
    rng = np.random.default_rng(sigma)
    for n in (10, 33, 100, 257, 1000, 3000):
        data = rng.integers(0, sigma, n, dtype=np.uint8).tobytes()
        rules, start = same(data)
        assert expand(rules, start) == data


@pytest.mark.parametrize("coder", M.CODERS)
def test_decode_inverts_encode(coder):
    rng = np.random.default_rng(11)
    texts = [b"", b"a", b"ab", b"a" * 37, fibonacci_word(500), thue_morse(300), bytes(range(256)) * 2 + b"\x00\xff" * 9]
    texts += [rng.integers(0, s, 400, dtype=np.uint8).tobytes() for s in (2, 4, 256)]
    for data in texts:
        for mr in MAX_RULES:
            rules, start = M.grammar(data, mr)
            s = M.encode(rules, start, coder)
            assert M.parse(s, coder) == (rules, start)
            assert M.sequential_decode(s, coder) == data, (data[:20], mr)


def test_decode_refusals():
    enc = lambda rules, start, coder="bit": M.encode(rules, start, coder)
    for coder in M.CODERS:
        with pytest.raises(M.Malformed):                          # rule 1 names itself (bit: Range(1) holds 1)
            M.sequential_decode(enc([(97, 98), (257, 97)], [257], coder), coder)
        with pytest.raises(M.Malformed):                          # a start symbol that names a rule >= rules
            M.sequential_decode(enc([(97, 98)], [257], coder), coder)
        bits = M.encode_bits([(97, 98)], [256, 99], coder)
        with pytest.raises(M.Malformed):                          # a cut-off field
            M.sequential_decode(terminate(bits[:-3]), coder)
    with pytest.raises(M.Malformed):                              # forward reference: rule 0 names rule 1
        M.sequential_decode(enc([(257, 97), (97, 98)], [256], "gamma"), "gamma")
    with pytest.raises(M.Malformed):                              # more rules than the stream can hold
        M.sequential_decode(terminate(format(1000, "032b")), "bit")
    doubling = [(97, 97)] + [(256 + i, 256 + i) for i in range(39)]
    assert M.expansion_lengths(doubling)[-1] == 1 << 40
    with pytest.raises(M.TooLarge):
        M.sequential_decode(enc(doubling, [256 + 39]), "bit")
    many = [(97, 97)] + [(256 + i, 256 + i) for i in range(69)]
    assert M.expansion_lengths(many)[-1] == (1 << 64) - 1         # saturates
    with pytest.raises(M.TooLarge):
        M.sequential_decode(enc(many, [256 + 69] * 3), "bit")


def test_coder_border_inputs():
    """what tests/test_gpu_repair.py relies on: the field counts 1 + 2 rules + start symbols of tests/coder_borders.py, a grammar whose
    rule sides reach across the first tile border of the coder, and streams on both sides of the terminator rule"""
    residues = set()
    for data, mr, fields in repair_borders():
        rules, start = M.grammar(data, mr)
        if fields is None:
            assert len(rules) == mr == 1100 and 1 + 2 * len(rules) > 2048          # field 2048 is a rule side
        else:
            assert len(rules) == 0 and 1 + len(start) == fields
        residues |= {residue(M.encode(rules, start, coder)) for coder in M.CODERS}
    assert {5, 6} <= residues
