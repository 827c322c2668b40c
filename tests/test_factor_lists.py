"""CPU checks of the factor-list generator (tests/factor_lists.py) against the oracle: every shape resolves to its text, the
oracle's flatten keeps that meaning, the oracle's huff / ascii / sle streams of every list decode back to the text, and `resolve`
refuses cyclic lists.  The large shapes run at small n here; tests/test_gpu_factor_lists.py takes them to full size."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import factor_lists as FL
from tests.util import factors_struct

CASES = FL.cases("cpu")
IDS = [c[0] for c in CASES]


def _case(cid, shape, n, kw):
    return FL.make_case(shape, n, FL.case_seed(cid), **kw)


def _literals(text, pos, length):
    """the text with every factor position zeroed: only the literals survive"""
    lit = np.frombuffer(text, dtype=np.uint8).copy()
    for p, l in zip(pos, length):
        lit[p:p + l] = 0
    return lit


def test_every_shape_is_listed():
    assert {c[1] for c in CASES} == set(FL.SHAPES)


@pytest.mark.parametrize("cid,shape,n,kw", CASES, ids=IDS)
def test_shape_resolves_flattens_and_round_trips(cid, shape, n, kw):
    text, pos, src, length = _case(cid, shape, n, kw)
    n = len(text)
    assert text[-1] == 0 and 0 not in text[:-1] and 255 not in text
    assert FL.resolve(n, _literals(text, pos, length), pos, src, length) == text, cid
    f = factors_struct(pos, src, length)
    flat, nf, md = O.flatten(f)
    assert (flat["pos"] == pos).all() and (flat["len"] == length).all()
    assert FL.resolve(n, _literals(text, pos, length), pos, flat["src"], length) == text, cid
    assert (nf == 0) == (md == 0)
    for lst in (f, flat):
        stream, _ = O.encode_huff(text, lst)
        assert O.lcpcomp_huff_decompress(stream) == text, cid
        stream, _ = O.encode_ascii(text, lst)
        assert O.lcpcomp_ascii_decompress(stream) == text, cid
        for k in (1, 3, 7):
            stream, _ = O.encode_sle(text, lst, k)
            assert O.lcpcomp_sle_decompress(stream, k) == text, (cid, k)


def test_shape_details():
    """what the shapes promise beyond validity"""
    text, pos, src, length = _case("one_literal-n70000", "one_literal", 70_000, {})
    assert len(set(text)) == 2 and list(pos) == [1] and list(src) == [0] and list(length) == [len(text) - 2]
    text, pos, src, length = _case("one_literal_len1-n2000", "one_literal_len1", 2000, {})
    assert (length == 1).all() and (src == pos - 1).all() and len(pos) == len(text) - 2
    for L in (1, 4097):
        _, _, _, length = _case("equal_lengths-L%d" % L, "equal_lengths", 48 * (L + 2), {"flen": L})
        assert len(length) > 8 and (length == L).all()
    text, pos, src, length = _case("extreme_sources-n5000", "extreme_sources", 5000, {"p0": 0})
    n = len(text)
    assert pos[0] == 0 and src[0] > 0 and (src + length == n - 1).any() and (src > pos).any() and (src < pos).any()
    text, pos, src, length = _case("extreme_sources-n300000", "extreme_sources", 300_000, {"p0": 5})
    assert (src == 0).any() and (src + length == len(text) - 1).any()
    text, pos, src, length = _case("overlap_runs", "overlap_runs", 200_000, {})
    d = src.astype(np.int64) - pos
    assert ((d >= -3) & (d <= -1)).any() and ((d >= 1) & (d <= 3)).any()
    for shape, want in (("run_512", 512), ("run_513", 513)):
        text, pos, src, length = _case(shape, shape, 1 << 15, {})
        f = factors_struct(pos, src, length)
        _, st = O.encode_huff(text, f)
        assert st["fdist_max"] == want
        inner = pos.astype(np.int64) - np.concatenate([[0], (pos.astype(np.int64) + length)[:-1]])
        assert inner.max() == 512 and len(text) - int(pos[-1] + length[-1]) == want


def test_million_steps_closed_form():
    big = 1 << 14
    text, pos, src, length = _case("million_steps", "million_steps", 0, {"big": big})
    flat, nf, md = O.flatten(factors_struct(pos, src, length))
    fin, dep = FL.million_steps_expected(pos, src, length, big)
    assert (flat["src"] == fin).all()
    assert nf == len(pos) - 1 and md == dep.max() and md > big - 16


def test_staircase_closed_form():
    text, pos, src, length = _case("staircase", "staircase", 0, {"K": 300})
    flat, nf, md = O.flatten(factors_struct(pos, src, length))
    assert (flat["src"] == src[0]).all() and nf == len(pos) - 1 and md == 1


def test_resolve_rejects_cycles():
    lit = np.full(10, 7, dtype=np.uint8); lit[-1] = 0
    with pytest.raises(FL.CycleError):                      # 2 <-> 5
        FL.resolve(10, lit, [2, 5], [5, 2], [1, 1])
    with pytest.raises(FL.CycleError):                      # src == pos
        FL.resolve(10, lit, [3], [3], [2])
    with pytest.raises(FL.CycleError):                      # a longer loop through two factors
        FL.resolve(10, lit, [1, 5], [5, 1], [3, 3])
    assert FL.resolve(10, lit, [2, 5], [5, 7], [1, 1]) == bytes(lit)
    with pytest.raises(ValueError):
        FL.resolve(10, lit, [2, 3], [0, 0], [2, 1])           # overlapping factors
