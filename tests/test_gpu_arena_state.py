"""GPU tests of one property: what a call returns does not depend on what its scratch held before (pytest -m gpu).

Every device buffer of the library comes from the context's arena, a bump allocator that never clears a byte (csrc/common.hpp).  A
kernel that reads one element too many, or an element its producer skipped, reads the leftovers of the call before.  On a fresh
context those are zeros; on the session-wide context they are buffers of the same layout from a similar text.  Here every case of
tests/arena_cases.py runs on an arena filled with each of the three byte values the code gives a meaning to -- 0x00 ("unset",
"factor 0"), 0x01 ("mark set", "class 1") and 0xFF (NONE32: "literal", "no entry", "empty slot") -- and then after other cases in a
shuffled order, and must return what the specification says, bit for bit.  tests/test_arena_cases.py checks the table on the CPU."""
import random

import numpy as np
import pytest

import tudocomp_amd as T
from tests import arena_cases as A
from tests.test_gpu_prims import _scan_reference

pytestmark = pytest.mark.gpu

ERR_ARG = -2


def _agrees(case, got, when):
    want = case.want()
    assert A.same(got, want), "%s %s: %s" % (case.name, when, A.first_difference(got, want))


@pytest.mark.parametrize("fill", A.FILLS, ids=["fill%02X" % f for f in A.FILLS])
@pytest.mark.parametrize("case", A.CASES, ids=[c.name for c in A.CASES])
def test_result_does_not_depend_on_scratch_content(case, fill):
    with T.Context(0, options=case.options) as ctx:
        if case.reserve:
            ctx.reserve(case.reserve)
        got, stats = case.run(ctx)                               # sizes the arena
        _agrees(case, got, "on a fresh context")
        if case.check:
            case.check(stats)
        where = ctx.prim_arena_fill(fill)
        assert where[1] > 0, "%s: the call left no arena behind" % case.name
        got2, stats2 = case.run(ctx)
        # a call that reallocated got fresh memory and would prove nothing
        assert ctx.prim_arena_fill() == where, "%s: the arena moved or grew in the second call" % case.name
        _agrees(case, got2, "on an arena full of 0x%02X" % fill)
        assert stats2 == stats, "%s on an arena full of 0x%02X: stats %r, on the fresh context %r" % (case.name, fill, stats2, stats)


def test_result_does_not_depend_on_the_calls_before():
    """big call, then small call, then another algorithm: one context, no fill, every default-options case in a shuffled order, twice
    through with two seeds"""
    cases = [c for c in A.CASES if c.default_options]
    assert len({c.family for c in cases}) >= 10
    before = "nothing (a fresh context)"
    with T.Context(0, options=A.DEV) as ctx:
        for seed in (1, 2):
            random.Random(seed).shuffle(cases)
            for case in cases:
                got, _ = case.run(ctx)
                _agrees(case, got, "(order %d) after %s" % (seed, before))
                before = case.name


def test_arena_fill_entry_point():
    a = np.random.default_rng(7).integers(0, 1 << 32, size=3 * 4096 + 5, dtype=np.uint32)
    want, want_total = _scan_reference("sum_u32", a)
    with T.Context(0) as ctx:
        assert ctx.prim_arena_fill() == (0, 0)                   # no arena yet: nothing to fill, and no error
        assert ctx.prim_arena_fill(0xFF) == (0, 0)
        ctx.reserve(1 << 20)
        base, size = ctx.prim_arena_fill()
        assert base != 0 and size > 0
        assert ctx.prim_arena_fill(0xA5) == (base, size)
        assert ctx.prim_arena_fill(0x00) == (base, size)
        got, total = ctx.prim_scan("sum_u32", a)
        assert np.array_equal(got, want) and total == want_total
        assert ctx.prim_arena_fill() == (base, size)             # (the scan ran in the memory that was filled)
        with pytest.raises(T.TdcGpuError) as e:
            ctx.prim_arena_fill(256)
        assert e.value.status == ERR_ARG
        assert ctx.prim_arena_fill(-1) == ctx.prim_arena_fill()  # a negative byte fills nothing either
        got, _ = ctx.prim_scan("sum_u32", a)
        assert np.array_equal(got, want)
