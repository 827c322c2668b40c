"""GPU tests of the shared device primitives (csrc/prim.hip, the MSD partition of csrc/ssort.hip), each driven alone through the entry
points of csrc/api_prims.hip (pytest -m gpu) and compared with numpy on exact integers -- every comparison is array_equal.  The sizes
are the ones at which the code forks ("Where the primitives fork"; constants in tests/prim_inputs.py); the generators are
checked on the CPU by tests/test_prim_inputs.py."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import prim_inputs as P

pytestmark = pytest.mark.gpu

S = P.STILE
M20 = 1 << 20
ERR_ARG = -2


@pytest.fixture(scope="module")
def lsd_scatter_ctx():
    """bucketed_scatter_u32 with two stable LSD passes instead of the MSD partition"""
    with T.Context(0, options={"msd_partition": 0}) as ctx:
        yield ctx


# ---- scans -----------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [0, 1, 3, S - 1, S, S + 1, 2 * S + 1, S * S - 1, S * S, S * S + 1]      # one level up to S, two up to S^2, three above


def _tile_slots(n):
    """first / last slots of tiles (of both scan levels) that exist in an array of n elements"""
    want = {0, S - 1, S, 2 * S - 1, 2 * S, S * S - 1, S * S, n - 1, (n - 1) // S * S, (n - 1) // S * S - 1}
    return sorted(p for p in want if 0 <= p < n)


def _scan_inputs(op, n, rng):
    if op == "sum_u32":
        yield "all_ones", np.full(n, 0xFFFFFFFF, dtype=np.uint32)                     # wraps from the second element on
        yield "random", rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        for p in _tile_slots(n):
            a = np.zeros(n, dtype=np.uint32)
            a[p] = 7
            yield "spike@%d" % p, a
    elif op == "sum_u64":
        # carries cross 2^32 inside a tile (2^40 * 4096 = 2^52) and between tiles; near 2^63 the sum wraps mod 2^64 every other element
        yield "near_2^40", np.uint64(1 << 40) - rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
        yield "near_2^63", np.uint64(1 << 63) + rng.integers(0, 1 << 33, size=n, dtype=np.uint64) - np.uint64(1 << 32)
    else:
        yield "decreasing", (np.uint32(0xFFFFFFFF) - np.arange(n, dtype=np.uint32))    # the first element wins across all tiles
        yield "random", rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        for p in _tile_slots(n):
            a = rng.integers(0, 1 << 20, size=n, dtype=np.uint32)
            a[p] = 1 << 30                                                              # a single maximum at a tile border
            yield "peak@%d" % p, a


def _scan_reference(op, a):
    if op == "max_u32":
        return (np.maximum.accumulate(a) if len(a) else a.copy()), None
    inc = np.cumsum(a, dtype=np.uint64)                                                 # exact mod 2^64
    if op == "sum_u32":
        inc &= np.uint64(0xFFFFFFFF)
    exc = np.concatenate([np.zeros(1, dtype=np.uint64), inc[:-1]])[:len(a)].astype(a.dtype)
    return exc, (int(inc[-1]) if len(a) else 0)


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("op", ["sum_u32", "sum_u64", "max_u32"])
def test_scan_vs_numpy(gpu_ctx, op, n):
    rng = np.random.default_rng(n + 17)
    big = n >= S * S - 1
    for q, (name, a) in enumerate(_scan_inputs(op, n, rng)):
        if big and q >= 4 and "@%d" % (S * S - 1) not in name and "@%d" % (S * S) not in name:
            continue                                      # 64 MB arrays: of the spikes, the two at the border of the second level
        want, want_total = _scan_reference(op, a)
        for in_place in (False, True):
            # the big arrays alternate between a null and a real d_total, the others take both: there every combination of
            # (in_place, total) occurs with some input, but not with every input -- the pairing is not exhaustive
            for want_tot in ((bool((q + in_place) & 1),) if big else (True, False)):
                got, total = gpu_ctx.prim_scan(op, a, in_place=in_place, want_total=want_tot)
                assert np.array_equal(got, want), (op, n, name, in_place, want_tot)
                if op != "max_u32" and want_tot:
                    assert total == want_total, (op, n, name, in_place)                # = the last inclusive value
                else:
                    assert total is None


# ---- LSD radix sorts -------------------------------------------------------------------------------------------------------------
LSD_RANGES_U32 = [(0, 1), (0, 13), (0, 8), (0, 32), (5, 21), (11, 12), (24, 32)]
LSD_RANGES_U64 = LSD_RANGES_U32 + [(0, 64), (32, 47), (57, 64)]
T4 = P.RS_TILE
# 4096: the tile; 64 tiles: the XCD walk starts; 128 tiles: CS_ROWS; 2^22: eight-wave tiles with radix_waves = 8
LSD_SIZES = [1, T4 - 1, T4, T4 + 1, 2 * T4 + 1, 64 * T4 - 1, 64 * T4 + 1, 128 * T4 - 1, 128 * T4 + 1, (1 << 22) - 1, 1 << 22]
LSD_BORDERS = [T4 + 1, 64 * T4 - 1, 64 * T4 + 1, 128 * T4 - 1, 128 * T4 + 1, (1 << 22) - 1, 1 << 22]


def _lsd_check(ctx, kind, keys, begin, end, rng, tag):
    n = len(keys)
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    order = P.stable_order(keys, begin, end)
    k, v = ctx.prim_sort_pairs(kind, keys, vals, begin, end)
    assert np.array_equal(v, vals[order]), tag                # stable: equal digits keep their input order
    assert np.array_equal(k, keys[order]), tag                # and the whole key travels, the bits outside [begin, end) too


def _lsd_keys(n, width, begin, end, rng, only=None):
    yield from P.sort_key_cases(n, rng, width, only)
    yield "equal_on_bits", P.equal_on_bits_keys(n, rng, begin, end, width)


LSD_GROUPS = (P.SORT_KEY_CASES[:4], P.SORT_KEY_CASES[4:8], P.SORT_KEY_CASES[8:] + ("equal_on_bits",))
LSD_ALL = P.SORT_KEY_CASES + ("equal_on_bits",)


def _lsd_params():
    """every distribution meets every bit range at every size: up to 8 193 pairs in one test per size, up to 128 tiles in one test
    per bit range, at 4 Mi pairs in three tests per bit range (the numpy reference of eleven 4 Mi sorts takes too long for one)"""
    for kind, ranges in (("u32", LSD_RANGES_U32), ("u64", LSD_RANGES_U64)):
        for n in LSD_SIZES:
            if n <= 2 * T4 + 1:
                yield pytest.param(kind, n, tuple(ranges), LSD_ALL, id="%s-%d" % (kind, n))
                continue
            for r in ranges:
                if n < (1 << 21):
                    yield pytest.param(kind, n, (r,), LSD_ALL, id="%s-%d-%d_%d" % (kind, n, r[0], r[1]))
                else:
                    for g, names in enumerate(LSD_GROUPS):
                        yield pytest.param(kind, n, (r,), names, id="%s-%d-%d_%d-g%d" % (kind, n, r[0], r[1], g))


@pytest.mark.parametrize("kind,n,ranges,names", list(_lsd_params()))
def test_lsd_sort_is_stable_on_bit_ranges(gpu_ctx, kind, n, ranges, names):
    width = 32 if kind == "u32" else 64
    rng = np.random.default_rng(n * 3 + width)
    for begin, end in ranges:
        for name, keys in _lsd_keys(n, width, begin, end, rng, set(names)):
            if name in names:
                _lsd_check(gpu_ctx, kind, keys, begin, end, rng, (kind, n, begin, end, name))


OPTION_SETS = {"radix_lds0": {"radix_lds": 0}, "radix_lds2": {"radix_lds": 2}, "xcd_remap0": {"xcd_remap": 0}, "radix_waves8": {"radix_waves": 8}}
OPTION_RANGES = {"u32": [(0, 13), (5, 21), (24, 32)], "u64": [(0, 13), (32, 47), (57, 64)]}


@pytest.fixture(scope="module", params=list(OPTION_SETS))
def option_ctx(request):
    with T.Context(0, options=OPTION_SETS[request.param]) as ctx:
        yield ctx


@pytest.mark.parametrize("n", LSD_BORDERS)
@pytest.mark.parametrize("kind,begin,end", [(k, b, e) for k in ("u32", "u64") for b, e in OPTION_RANGES[k]])
def test_lsd_sort_borders_under_options(option_ctx, kind, begin, end, n):
    """radix_lds 0 / 1 / 2: direct scatter, LDS-reordered scatter, the latter for u32 keys only; xcd_remap 0: plain tile walk;
    radix_waves 8: 8 192-pair tiles from 2^22 pairs.  (The defaults -- radix_lds 1, xcd_remap 1, radix_waves 4 -- are what
    test_lsd_sort_is_stable_on_bit_ranges runs.)  Long runs of equal digits in random order, all-ones keys next to the padding of a
    partial last tile, and keys that tie on every sorted bit."""
    width = 32 if kind == "u32" else 64
    rng = np.random.default_rng(n + width + begin)
    for name, keys in _lsd_keys(n, width, begin, end, rng, {"37_values", "max_keys"}):
        _lsd_check(option_ctx, kind, keys, begin, end, rng, (kind, n, begin, end, name))


# ---- distinct sort ---------------------------------------------------------------------------------------------------------------
# bitonic up to 2048 (begin_bit = 0), one-workgroup radix up to 8192, the device-wide radix sort above (and up to 2048 with begin_bit != 0)
DISTINCT_SIZES = [1, 2, 7, 8, 9, 2047, 2048, 2049, 8191, 8192, 8193, 20000]


@pytest.mark.parametrize("begin,end", [(0, 32), (0, 45), (0, 56), (0, 64), (8, 40)])
def test_distinct_sort_vs_numpy(gpu_ctx, begin, end):
    rng = np.random.default_rng(begin * 64 + end)
    for n in DISTINCT_SIZES:
        keys = P.distinct_on_bits_keys(n, rng, begin, end)     # random bits below begin and above end; the all-ones field among them
        vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        order = np.argsort(P.sort_field(keys, begin, end), kind="stable")
        k, v = gpu_ctx.prim_sort_pairs("distinct", keys, vals, begin, end)
        assert np.array_equal(k, keys[order]), (n, begin, end)  # the outside bits travel and do not influence the order
        assert np.array_equal(v, vals[order]), (n, begin, end)


# ---- bucketed scatter ------------------------------------------------------------------------------------------------------------
# The partition starts at 2^20 pairs.  (The db = 9 branch of the MSD partition needs more than 2^29 destinations -- 2 GiB of them: it
# stays with the full-size pipeline tests; msd_partition_pairs_u32 itself is driven with db = 9 below.)
SCATTER_M = [1, 1000, M20 - 1, M20, M20 + 1, 3 * M20 + 5]
FILL = 0xDEADBEEF


def _scatter_check(ctxs, idx, val, n_dst, permutation, full_cross):
    want = np.full(n_dst, FILL, dtype=np.uint32)
    want[idx] = val                                             # every other slot still holds the fill word
    for msd, ctx in enumerate(ctxs):
        for second_tmp in (True, False):
            for offset in (0, 1):
                if not full_cross and (msd == 0 or not second_tmp):
                    continue
                got = ctx.prim_bucketed_scatter(idx, val, n_dst, fill=FILL, permutation=permutation, second_tmp=second_tmp, offset=offset)
                assert np.array_equal(got, want), (len(idx), n_dst, permutation, msd, second_tmp, offset)


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("m", SCATTER_M)
def test_bucketed_scatter_permutation(gpu_ctx, lsd_scatter_ctx, m, extra):
    """idx holds every index of [0, m) once; n_dst = m, or m + 1 with the last index absent (the window-image pass and its partial
    last window from 2^20 pairs on)"""
    rng = np.random.default_rng(m + extra)
    idx = P.permutation_indices(m, rng)
    val = rng.integers(0, 1 << 32, size=m, dtype=np.uint32)
    _scatter_check((lsd_scatter_ctx, gpu_ctx), idx, val, m + extra, True, True)


def _injection_params():
    for m in SCATTER_M:
        for n_dst in sorted({m, M20 + 7, 1 << 24, (1 << 27) + 3}):
            if n_dst >= m:
                yield pytest.param(m, n_dst, id="%d-into-%d" % (m, n_dst))


@pytest.mark.parametrize("m,n_dst", list(_injection_params()))
def test_bucketed_scatter_injection(gpu_ctx, lsd_scatter_ctx, m, n_dst):
    """random pairwise distinct indices; n_dst = m (every slot written), 2^20 + 7, 2^24 and 2^27 + 3 (21, 24 and 28 index bits)"""
    rng = np.random.default_rng(m + n_dst)
    idx = P.distinct_indices(m, n_dst, rng)
    val = rng.integers(0, 1 << 32, size=m, dtype=np.uint32)
    # below 2^20 pairs nothing is partitioned: neither the option nor the temporaries are looked at, only the alignment of the views is
    # -- over 512 MB of destinations those cases take the two offsets only
    _scatter_check((lsd_scatter_ctx, gpu_ctx), idx, val, n_dst, False, m >= M20 or n_dst <= (1 << 24))


# ---- MSD partition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,db", [(17, 8), (20, 8), (24, 8), (32, 8), (19, 9), (30, 9), (32, 9)])
def test_msd_partition_groups_and_keeps_the_pairs(gpu_ctx, bits, db):
    rng = np.random.default_rng(bits * 16 + db)
    for m in (1, 4095, M20 + 1, 3 * M20):
        for kind in ("uniform", "one_group", "two_groups"):
            idx = P.msd_indices(m, bits, db, kind, rng)
            val = rng.integers(0, 1 << 32, size=m, dtype=np.uint32)
            oi, ov = gpu_ctx.prim_msd_partition(idx, val, bits, db)
            group = (oi >> np.uint32(bits - 2 * db)).astype(np.int64)
            assert (np.diff(group) >= 0).all(), (bits, db, m, kind)
            # the multiset of pairs: both sides in lexicographic order
            pairs_in = np.sort((idx.astype(np.uint64) << np.uint64(32)) | val)
            pairs_out = np.sort((oi.astype(np.uint64) << np.uint64(32)) | ov)
            assert np.array_equal(pairs_in, pairs_out), (bits, db, m, kind)


# ---- selection -------------------------------------------------------------------------------------------------------------------
# tiles of 2048; an aligned 8-byte class load with a scalar tail; more than 4096 tiles: the tile counts take the two-level scan
SELECT_M = [0, 1, 7, 8, 9, P.SEL_TILE - 1, P.SEL_TILE, P.SEL_TILE + 1, 4096 * P.SEL_TILE + 9]
FILL_A, FILL_B = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A


@pytest.mark.parametrize("want", [0, 3, 255])
@pytest.mark.parametrize("m", SELECT_M)
def test_select_by_class_vs_numpy(gpu_ctx, m, want):
    rng = np.random.default_rng(m + want)
    src_a = rng.integers(0, 1 << 32, size=m, dtype=np.uint32)
    src_b = rng.integers(0, 1 << 64, size=m, dtype=np.uint64)
    for density in P.SELECT_DENSITIES:
        cls = P.select_classes(m, want, density, rng)
        sel = np.flatnonzero(cls == want)                       # ascending: the order is preserved
        for with_a in (False, True):
            for with_b in (False, True):
                oa, ob, cnt = gpu_ctx.prim_select(cls, want, src_a if with_a else None, src_b if with_b else None, FILL_A, FILL_B)
                tag = (m, want, density, with_a, with_b)
                assert cnt == len(sel), tag
                assert np.array_equal(oa[:cnt], src_a[sel] if with_a else sel.astype(np.uint32)), tag
                assert (oa[cnt:] == FILL_A).all(), tag          # nothing is written behind the count
                if with_b:
                    assert np.array_equal(ob[:cnt], src_b[sel]), tag
                    assert (ob[cnt:] == FILL_B).all(), tag
                else:
                    assert ob is None


# ---- orbit -----------------------------------------------------------------------------------------------------------------------
ORBIT_SIZES = [1, 2, P.ORB_TILE - 1, P.ORB_TILE, P.ORB_TILE + 1, P.ORB_SUPER - 1, P.ORB_SUPER, P.ORB_SUPER + 1, 3 * P.ORB_SUPER + 17]


@pytest.mark.parametrize("n", ORBIT_SIZES)
@pytest.mark.parametrize("kind", P.ORBIT_KINDS)
def test_mark_orbit_vs_serial_walk(gpu_ctx, kind, n):
    nxt = P.orbit_next(n, kind, np.random.default_rng(n))
    assert np.array_equal(gpu_ctx.prim_mark_orbit(nxt), P.orbit_reference(nxt)), (kind, n)


# ---- tile entries ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntiles,states,kinds", P.TILE_EXIT_CASES, ids=P.TILE_EXIT_IDS)
def test_tile_entries_vs_sequential_walk(gpu_ctx, ntiles, states, kinds):
    for kind in kinds:
        ex = P.tile_exits(ntiles, states, kind, np.random.default_rng(ntiles + states))
        want = P.tile_entries_reference(ex) if ex.size <= 1 << 24 else P.tile_entries_reference_array(ex)
        assert np.array_equal(gpu_ctx.prim_tile_entries(ex), want), (kind, ntiles, states)


def test_tile_entries_refuses_exits_outside_the_table(gpu_ctx):
    u16 = lambda rows: np.array(rows, dtype=np.uint16)
    _refused(lambda: gpu_ctx.prim_tile_entries(u16([[0, 1], [2, 0]])))                    # an exit == states
    _refused(lambda: gpu_ctx.prim_tile_entries(u16([[0, 1], [0, 0xFFFE]])))               # ... and one just below NONE
    _refused(lambda: gpu_ctx.prim_tile_entries(np.zeros((3, 0), dtype=np.uint16)))        # no states
    wide = np.zeros((3, 255), dtype=np.uint16)
    wide[1, 254] = 255
    _refused(lambda: gpu_ctx.prim_tile_entries(wide))                                      # an exit == states at the huff decoder's widest
    wide[1, 254] = 254
    assert gpu_ctx.prim_tile_entries(wide).tolist() == [0, 0, 0]
    assert gpu_ctx.prim_tile_entries(u16([[1, 0], [0xFFFF, 0xFFFF], [0, 0]])).tolist() == [0, 1, 0xFFFF]      # the context survives


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(T.TdcGpuError) as e:
        call()
    assert e.value.status == ERR_ARG


def test_broken_preconditions_are_refused_and_the_context_survives(gpu_ctx):
    u32 = lambda *x: np.array(x, dtype=np.uint32)
    u64 = lambda *x: np.array(x, dtype=np.uint64)
    _refused(lambda: gpu_ctx.prim_mark_orbit(u32(1, 1, 3)))                               # next[i] <= i
    _refused(lambda: gpu_ctx.prim_mark_orbit(u32(1, 2, 4)))                               # next[i] > n
    _refused(lambda: gpu_ctx.prim_bucketed_scatter(u32(0, 2, 0), u32(1, 2, 3), 4))        # idx not pairwise distinct
    _refused(lambda: gpu_ctx.prim_bucketed_scatter(u32(0, 4), u32(1, 2), 4))              # idx >= n_dst
    _refused(lambda: gpu_ctx.prim_bucketed_scatter(u32(0, 3, 1), u32(1, 2, 3), 4, permutation=True))   # not every index of [0, m)
    _refused(lambda: gpu_ctx.prim_bucketed_scatter(u32(0, 1), u32(1, 2), 4, permutation=True))         # m is neither n_dst nor n_dst - 1
    _refused(lambda: gpu_ctx.prim_msd_partition(u32(1, 2), u32(1, 2), 16, 8))             # bits <= 2 * db
    _refused(lambda: gpu_ctx.prim_msd_partition(u32(1, 2), u32(1, 2), 18, 9))
    _refused(lambda: gpu_ctx.prim_msd_partition(u32(1, 2), u32(1, 2), 24, 7))             # db is neither 8 nor 9
    _refused(lambda: gpu_ctx.prim_msd_partition(u32(1, 2), u32(1, 2), 24, 10))
    _refused(lambda: gpu_ctx.prim_msd_partition(u32(1, 1 << 20), u32(1, 2), 20, 8))       # idx >= 2^bits
    _refused(lambda: gpu_ctx.prim_sort_pairs("u64", u64(2, 1), u32(0, 1), 0, 65))         # end_bit beyond the key
    _refused(lambda: gpu_ctx.prim_sort_pairs("u32", u32(2, 1), u32(0, 1), 0, 33))
    _refused(lambda: gpu_ctx.prim_sort_pairs("distinct", u64(2, 1), u32(0, 1), 0, 65))
    _refused(lambda: gpu_ctx.prim_sort_pairs("u64", u64(2, 1), u32(0, 1), 9, 8))          # begin_bit > end_bit
    _refused(lambda: gpu_ctx.prim_sort_pairs("distinct", u64(0x105, 0x205, 3), u32(0, 1, 2), 0, 8))    # distinct keys that collide on the sorted bits
    _refused(lambda: gpu_ctx.prim_sort_pairs("distinct", u64(1, 2), u32(0, 1), 8, 8))     # ... as any two keys do on no bits at all
    a = np.random.default_rng(3).integers(0, 1 << 32, size=2 * S + 1, dtype=np.uint32)
    want, want_total = _scan_reference("sum_u32", a)
    got, total = gpu_ctx.prim_scan("sum_u32", a)
    assert np.array_equal(got, want) and total == want_total
