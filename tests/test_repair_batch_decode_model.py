"""CPU tests of the model of repair's batch decoder (tests/models/repair_batch_decode.py) against the reference's decode loop
(tests/models/repair.sequential_decode) on each stream alone: the damaged streams of tests/repair_damage.py, foreign grammars with
unused, repeated and saturating rules, indices that only a neighbour's rules would make valid, chains at the height cap, and the
call-level limits on made-up counts."""
import random

import pytest

from tests import repair_batch_decode_cases as C
from tests import repair_damage as RD
from tests.models import repair as M
from tests.models import repair_batch_decode as B


def alone(streams, coder, cap=B.ROUNDS):
    v = [B.expected(s, coder, cap) for s in streams]
    return [x[1] for x in v], [x[0] for x in v]


def check_batch(streams, coder, cap=B.ROUNDS):
    """the batch formulation against the verdict on every stream alone"""
    rc, texts, status, out_off = B.decode_batch(streams, coder, cap)
    want_texts, want_status = alone(streams, coder, cap)
    assert rc == 0 and status == want_status
    assert texts == want_texts
    assert out_off[-1] == sum(len(x) for x in want_texts)
    return texts, status


@pytest.mark.parametrize("coder", C.CODERS)
def test_damaged_streams_against_the_host_loop(coder):
    streams = [s for _, s in RD.damaged_streams(coder)]
    assert len(streams) == C.DAMAGED[coder]
    excepted = 0
    for s in streams:
        status, text, exc = B.expected(s, coder)
        h_status, h_text = B.host(s, coder)
        if exc:                                                   # a cap: the host loop reads the token and does not refuse the stream
            assert status == B.ERR_ARG and h_status != B.ERR_ARG and text == b""
            excepted += 1
        else:
            assert (status, text) == (h_status, h_text)
    assert excepted <= C.EXCEPTED_MOST * len(streams) and (coder != "bit" or excepted == 0), excepted
    check_batch(streams, coder)


@pytest.mark.parametrize("coder", C.CODERS)
def test_foreign_grammars(coder):
    streams, texts = [], []
    for nr in (0, 1, 2, 3, 5, 17, 64, 255, 256, 257):
        s, t = C.foreign_stream(nr, coder)
        assert M.sequential_decode(s, coder) == t
        streams.append(s)
        texts.append(t)
    # rules of saturating length that nothing names, behind a shallow start sequence; and the same grammar used up to 2^20 bytes
    rules = [(97, 97)] + [(256 + k - 1, 256 + k - 1) for k in range(1, 40)]
    streams += [M.encode(rules, [98, 256, 99], coder), M.encode(rules, [256 + 9, 256 + 3, 256 + 9], coder)]
    texts += [b"baac", b"a" * (1024 + 16 + 1024)]
    got, status = check_batch(streams, coder)
    assert got == texts and status == [0] * len(streams)


@pytest.mark.parametrize("coder", C.CODERS)
def test_random_small_grammars(coder):
    rng = random.Random(7)
    streams = []
    for _ in range(60):
        nr = rng.randrange(0, 9)
        rules = [tuple(256 + rng.randrange(i) if i and rng.random() < 0.5 else rng.randrange(97, 100) for _ in range(2)) for i in range(nr)]
        start = [256 + rng.randrange(nr) if nr and rng.random() < 0.5 else rng.randrange(65, 70) for _ in range(rng.randrange(0, 7))]
        streams.append(M.encode(rules, start, coder))
    check_batch(streams, coder)


@pytest.mark.parametrize("coder", C.CODERS)
def test_own_stream(coder):
    streams, status, texts = C.own_stream_batch(coder)
    assert check_batch(streams, coder) == (texts, status)
    # under a global count the third would pass: the stream in front of it has a rule 1
    assert len(M.parse(streams[4], coder)[0]) >= 2


@pytest.mark.parametrize("coder", C.CODERS)
def test_chains_at_the_cap(coder):
    streams, texts, at_d, below = C.depth_batch(coder)
    got, status = check_batch(streams, coder, C.DEPTH)
    assert (got, status) == (texts, at_d)
    got, status = check_batch(streams, coder, C.DEPTH - 1)
    assert status == below and got == [b"" if v else x for v, x in zip(below, texts)]
    assert check_batch(streams, coder)[1] == at_d                 # the default cap
    rules, _, _ = C.chain(C.DEPTH)
    assert max(B.heights(rules)) == C.DEPTH
    ln, rounds = B.strict_lengths(rules, C.DEPTH - 1)
    assert ln.count(0) == 1 and rounds == C.DEPTH - 1            # exactly the rule of height d is left


@pytest.mark.parametrize("coder", C.CODERS)
def test_minimal_streams(coder):
    good = C.known(coder)[2]
    for s, want in C.minimal(coder):
        texts, status = check_batch([good, s, good], coder)
        assert status == [0, want, 0] and texts == [C.KNOWN[2], b"", C.KNOWN[2]]
        assert B.host(s, coder)[0] == want


@pytest.mark.parametrize("coder", C.CODERS)
def test_oversized_claims(coder):
    good = C.known(coder)[0]
    rc, texts, status, out_off = B.decode_batch([good, C.doubling(30, [30, 30], coder), good], coder)
    assert rc == 0 and status == [0, B.ERR_TOO_LARGE, 0] and texts == [C.KNOWN[0], b"", C.KNOWN[0]]
    assert B.host(C.doubling(30, [30, 30], coder), coder)[0] == B.ERR_TOO_LARGE
    three = [C.doubling(30, [30], coder)] * 3
    for cap in (None, 100):
        rc, texts, status, out_off = B.decode_batch(three, coder, out_cap=cap)
        assert rc == B.ERR_TOO_LARGE and texts is None and status == [0, 0, 0] and out_off == [0, 2**31, 2**32, 3 * 2**31]
    assert B.expected(three[0], coder, decode=False)[0] == 0
    assert B.expected(C.bad_and_large(coder), coder)[0] == B.ERR_ARG == B.host(C.bad_and_large(coder), coder)[0]
    rc, texts, status, out_off = B.decode_batch([good, good], coder, out_cap=2 * len(C.KNOWN[0]) - 1)
    assert rc == B.ERR_OOM and texts is None and out_off == [0, 12, 24] and status == [0, 0]


def test_call_level_limits():
    assert B.call_limits(0, 0) == 0 and B.call_limits(2**32 - 259, 2**32 - 2) == 0
    assert B.call_limits(2**32 - 258, 0) == B.ERR_TOO_LARGE and B.call_limits(2**33, 5) == B.ERR_TOO_LARGE
    assert B.call_limits(10, 2**32 - 1) == B.ERR_TOO_LARGE
    assert 256 + (B.TOKEN_LIMIT - 1) // 2 < 2**32                 # a rebased reference leaves 32 bits with room to spare
    with pytest.raises(ValueError):
        B.decode_batch([], "ascii")
    assert B.decode_batch([], "bit") == (0, [], [], [0])
