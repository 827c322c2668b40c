"""CPU check of the chunked flatten model (tests/models/flatten_chunks.py) against the round model it is derived from
(tests/models/position_space.py::flatten_rounds): on every small factor list of tests/factor_lists.py, K rank ranges done one after the
other give the sources, num_flattened and max_depth_lb of the rounds over the whole list -- for K = 2, 3, 7, one factor per range
(K = z) and more ranges than factors (K = z + 5, clamped)."""
import functools

import pytest

from tests import factor_lists as FL
from tests.models.flatten_chunks import chunk_bounds, flatten_rounds_chunked
from tests.models.position_space import flatten_rounds

CASES = FL.cases("cpu")
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _whole(cid):
    _, shape, n, kw = CASES[IDS.index(cid)]
    _, pos, src, length = FL.make_case(shape, n, FL.case_seed(cid), **kw)
    factors = [(int(p), int(s), int(l)) for p, s, l in zip(pos, src, length)]
    return factors, flatten_rounds(factors)


def test_bounds_are_equal_counts_and_clamped():
    assert chunk_bounds(10, 3) == [0, 3, 6, 10]
    assert chunk_bounds(3, 8) == [0, 1, 2, 3] and chunk_bounds(1, 16) == [0, 1] and chunk_bounds(5, 0) == [0, 5]
    for z in (1, 2, 7, 1000, 150_000_001):
        for K in (1, 2, 3, 7, 16):
            b = chunk_bounds(z, K)
            sizes = [y - x for x, y in zip(b, b[1:])]
            assert b[0] == 0 and b[-1] == z and min(sizes) >= 1 and max(sizes) - min(sizes) <= 1


@pytest.mark.parametrize("cid", IDS)
def test_chunked_rounds_equal_whole_rounds(cid):
    factors, (want, nf, md, _) = _whole(cid)
    z = len(factors)
    for K in sorted({2, 3, 7, z, z + 5}):
        got, gnf, gmd, _ = flatten_rounds_chunked(factors, K)
        assert got == want, "%s K=%d: %d sources differ" % (cid, K, sum(a != b for a, b in zip(got, want)))
        assert (gnf, gmd) == (nf, md), "%s K=%d: num_flattened / max_depth_lb" % (cid, K)
