"""The device decoder of repair, pass by pass (tests/models/repair_decode.py), against the reference's loop (repair.sequential_decode):
CPU only."""
import itertools
import random

import pytest

from tests.models import repair as R
from tests.models import repair_decode as D
from tests.models.lzss_coders import Malformed, bits_for
from tests.util import load_json

CODERS = ("bit", "gamma", "delta")
# (segment bits, rules the host reads under bit): the defaults, and small segments with every stretch on the "device"
SHAPES = ((1 << 30, D.HOST_RULES), (64, 0), (4096, 3))


def both(stream, coder, **kw):
    """(verdict, text) of the model, checked against the host loop's"""
    def run(f):
        try:
            return "ok", f()
        except Malformed:
            return "arg", None
        except R.TooLarge:
            return "too large", None
    want = run(lambda: R.sequential_decode(stream, coder))
    got = run(lambda: D.decode(stream, coder, **kw))
    assert got == want
    return got


def check_grammar(rules, start, want=None):
    for coder in CODERS:
        s = R.encode(rules, start, coder)
        for seg, host in SHAPES:
            st = {}
            verdict, text = both(s, coder, seg_bits=seg, host_rules=host, stats=st)
            assert verdict == "ok" and st["device"] == 1
            if want is not None:
                assert text == want


def fibonacci_word(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def thue_morse(n):
    return bytes(97 + bin(i).count("1") % 2 for i in range(n))


def test_kats():
    for case in load_json("repair_kats.json")["cases"]:
        rules = [tuple(r) for r in case["rules"]]
        check_grammar(rules, case["start"], case["text"].encode("latin-1"))


def test_runs():
    for k in range(71):
        text = b"a" * k
        check_grammar(*R.grammar(text), text)


def test_short_strings_over_three_letters():
    for n in range(9):
        for t in itertools.product(b"abc", repeat=n):
            text = bytes(t)
            rules, start = R.grammar(text)
            for coder in CODERS:
                assert D.decode(R.encode(rules, start, coder), coder, seg_bits=64, host_rules=0) == text


def test_words():
    for text in (fibonacci_word(500), thue_morse(300)):
        check_grammar(*R.grammar(text), text)
        check_grammar(*R.grammar(text, 5), text)


def random_grammar(rng, nrules):
    """foreign grammars: unused rules, shared subtrees, chains"""
    rules = []
    for i in range(nrules):
        def side():
            return R.SIGMA + rng.randrange(i) if i and rng.random() < 0.6 else rng.choice(b"abcd")
        rules.append((R.SIGMA + i - 1, side()) if i and rng.random() < 0.2 else (side(), side()))
    used = [rng.randrange(nrules) for _ in range(rng.randrange(1, 4))] if nrules else []
    start = [R.SIGMA + rng.choice(used) if used and rng.random() < 0.5 else rng.choice(b"abcd") for _ in range(rng.randrange(0, 12))]
    return rules, start


def test_random_foreign_grammars():
    rng = random.Random(20)
    for _ in range(150):
        rules, start = random_grammar(rng, rng.randrange(0, 41))
        ln = R.expansion_lengths(rules)
        if sum(1 if x < R.SIGMA else ln[x - R.SIGMA] for x in start) > 1 << 16:
            continue
        check_grammar(rules, start)


@pytest.mark.parametrize("k", range(1, 11))
def test_stretch_boundaries_under_bit(k):
    """every segment starts at the bit where its first token starts, reads it and all it keeps with their true width, and the segments
    tile the tokens"""
    for nrules in ((1 << k) - 1, 1 << k, (1 << k) + 1):
        rules = [(97 + i % 3, 98) if i < 2 or i % 5 == 0 else (R.SIGMA + (i * 7) % i, 99) for i in range(nrules)]
        start = [R.SIGMA + nrules - 1, 100, R.SIGMA + nrules // 2, 101]
        syms = [x for r in rules for x in r] + start
        width = [bits_for(t >> 1) if t < 2 * nrules else bits_for(nrules) for t in range(len(syms))]
        at = [32]                                                 # the bit at which token t starts
        for x, w in zip(syms, width):
            at.append(at[-1] + (9 if x < R.SIGMA else 1 + w))
        stream = R.encode(rules, start, "bit")
        for seg, host in ((1 << 30, 0), (96, 0), (1 << 30, 3), (1 << 30, D.HOST_RULES)):
            log = []
            assert D.parse_device(stream, "bit", seg, host, log) == (rules, start)
            t = 2 * min(nrules, host)
            for x_in, t_in, w, keep in log:
                assert t_in == t and x_in == at[t] and keep >= 1
                assert all(width[j] == w for j in range(t, t + keep))
                t += keep
            assert t == len(syms)
            if host == 0 and seg == 1 << 30:                      # one segment per stretch where the estimate holds: k + 1 widths, and the start
                assert len({w for _, t_in, w, _ in log if t_in < 2 * nrules}) == len(set(width[:2 * nrules]))


def chain(n):
    return [(97, 98)] + [(R.SIGMA + i - 1, 98) for i in range(1, n)]


def test_depth_cap():
    rules, start = chain(50), [R.SIGMA + 49, 99]
    want = b"a" + b"b" * 50 + b"c"
    for coder in CODERS:
        s = R.encode(rules, start, coder)
        st = {}
        assert D.decode(s, coder, cap=16, stats=st) == want and st["device"] == 0          # the fall-back is reported
        assert D.decode(s, coder, cap=64, stats=st) == want and st["device"] == 1
        # the quiet round counts: 50 rounds fill the lengths; the start sequence seeds the top rule, 49 rounds walk down the chain
        assert st["len_rounds"] == 51 and st["first_rounds"] == 50


def test_unused_saturated_rule_does_not_fail_the_call():
    doubling = [(97, 97)] + [(R.SIGMA + i - 1, R.SIGMA + i - 1) for i in range(1, 40)]
    for coder in CODERS:
        assert both(R.encode(doubling, [97], coder), coder) == ("ok", b"a")
        assert both(R.encode(doubling, [R.SIGMA + 39], coder), coder) == ("too large", None)
        assert both(R.encode(doubling, [R.SIGMA + 10], coder), coder) == ("ok", b"a" * 2048)


def test_refusals_and_caps():
    rules, start = [(97, 98), (R.SIGMA, 99), (R.SIGMA + 1, R.SIGMA)], [R.SIGMA + 2, 100]
    for coder in CODERS:
        s = R.encode(rules, start, coder)
        for cut in range(len(s)):                                 # every truncation: the host loop's verdict
            both(s[:cut], coder, seg_bits=64, host_rules=0)
        bits = R.encode_bits(rules, start, coder)
        for i in range(len(bits)):                                # every single-bit flip
            flipped = bits[:i] + ("1" if bits[i] == "0" else "0") + bits[i + 1:]
            both(R.terminate(flipped), coder, seg_bits=64, host_rules=0)
    # a gamma literal of nine value bits: the host keeps the low byte, the device hands the stream over
    wide = R.terminate("010" + "0" + "0" * 9 + "1" + "101100001")   # no rules (gamma of 0), then flag 0 and gamma(0x161)
    st = {}
    assert D.decode(wide, "gamma", stats=st) == R.sequential_decode(wide, "gamma") == b"a" and st["device"] == 0
