"""CPU tests of the model of bwt over a batch (tests/models/bwt_batch.py) against the model of the single compressor
(tests/models/bwt.py): the per-text doubling with its round counter and invariant, and the forest of LF cycles with its verdicts."""
import numpy as np
import pytest

from tests import bwt_batches as B
from tests.models import bwt as M
from tests.models import bwt_batch as MB


def test_forward_equals_the_naive_suffix_array_per_text():
    texts = B.model_texts()
    st = {}
    sas, outs, status = MB.forward(texts, stats=st)
    assert status == [0] * len(texts)
    for t, sa, out in zip(texts, sas, outs):
        assert sa == M.suffix_array_naive(t).tolist()
        assert out == M.bwt_forward(t)
    assert 0 < st["rounds"] <= st["bound"]


def test_rounds_of_a_run():
    """a^n 0 takes the most rounds: 4 * 2^r symbols must reach n"""
    for n, rounds in ((4097, 11), (8, 1), (9, 2), (5, 1), (4, 0)):
        st = {}
        t = b"a" * n + b"\x00"
        sas, outs, status = MB.forward([b"b\x00", t, t], stats=st)
        assert status == [0, 0, 0]
        assert outs[1] == outs[2]
        if n < 100:
            assert outs[1] == M.bwt_forward(t)
        else:
            assert outs[1] == b"a" * n + b"\x00"                    # SA = n, n - 1, ..., 0: every row but the last has an a in front
        assert sas[1] == list(range(n, -1, -1))
        assert st["rounds"] == rounds <= st["bound"], (n, st)


def test_borders_do_not_leak():
    a = B.text("random2", 60, 5)
    pre, suf = a[:20] + b"\x00", a[30:]
    batch = [a, a, pre, a, suf, b"\x00", a, b"\x00", pre]
    sas, outs, status = MB.forward(batch)
    assert status == [0] * len(batch)
    assert outs == [M.bwt_forward(t) for t in batch]


def test_forward_refusals_stand_alone():
    good = B.text("english", 100, 2)
    batch = [good, b"ab\x00cd\x00", good, b"abc", b"", good, b"x" * 100 + b"\x00", b"\x00\x00", good]
    sas, outs, status = MB.forward(batch, cap=100)
    assert status == [0, MB.ERR_ARG, 0, MB.ERR_NO_SENTINEL, MB.ERR_NO_SENTINEL, 0, MB.ERR_TOO_LARGE, MB.ERR_ARG, 0]
    assert [o for o, s in zip(outs, status) if s == 0] == [M.bwt_forward(good)] * 4
    assert all(o is None for o, s in zip(outs, status) if s)


@pytest.mark.parametrize("sample,steps", [(0, 0), (4, 8), (2, 3), (16, 1000)])
def test_inverse_round_trip(sample, steps):
    texts = B.model_texts()
    bwts = [M.bwt_forward(t) for t in texts]
    st = {}
    res, status = MB.inverse(bwts, sample, steps, st)
    assert status == [0] * len(texts)
    assert res == [t if len(t) >= 2 else b"" for t in texts]
    assert res == [M.inverse_loop(b) for b in bwts]
    if (sample, steps) == (4, 8):
        assert st["launches"] >= 2 and st["slots"] > M.head_threshold(sum(map(len, bwts)), 4) + len(bwts)


def no_transforms():
    """buffers with one 0 whose LF mapping has two cycles or more: all over {0, a, b} of length 2 and 3"""
    import itertools
    found = []
    for n in (2, 3):
        for b in itertools.product((0, 97, 98), repeat=n):
            b = bytes(b)
            if b.count(0) == 1 and MB.cycles(b) > 1:
                found.append(b)
    return found


def test_the_smallest_buffers_that_are_no_transform():
    found = no_transforms()
    assert [len(b) for b in found].count(2) == 2 and [len(b) for b in found].count(3) == 8
    assert b"\x00a" in found


@pytest.mark.parametrize("sample,steps", [(0, 0), (4, 8), (2, 2)])
def test_inverse_verdicts_stand_alone(sample, steps):
    good_t = [B.text("english", 300, 9), B.text("ab", 41, 1), b"q\x00"]
    good = [M.bwt_forward(t) for t in good_t]
    bad = no_transforms() + [b"a\x00b\x00c", b"abcabc", b"\x00\x00"]
    rng = np.random.default_rng(11)
    swapped = None
    base = bytearray(M.bwt_forward(B.text("random255", 400, 4)))
    for _ in range(50):
        i, j = (int(x) for x in rng.integers(0, len(base), 2))
        if base[i] and base[j] and base[i] != base[j]:
            cand = bytearray(base)
            cand[i], cand[j] = cand[j], cand[i]
            if MB.cycles(bytes(cand)) == 2:
                swapped = bytes(cand)
                break
    assert swapped is not None
    bad.append(swapped)
    batch, want = [], []
    for k, b in enumerate(bad):
        g = k % len(good)
        batch += [good[g], b]
        want += [good_t[g], None]
    batch += [b"", b"a", b"\x00", good[0]]
    want += [b"", b"", b"", good_t[0]]
    res, status = MB.inverse(batch, sample, steps)
    assert res == want
    assert status == [MB.ERR_ARG if w is None else 0 for w in want]
    for b, w in zip(batch, want):                               # the verdict of the single model on every buffer alone
        try:
            alone = M.inverse_device(b)
        except M.Malformed:
            alone = None
        assert alone == w
