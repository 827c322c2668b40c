"""CPU tests of tests/prim_inputs.py: every generator of the primitive tests meets the preconditions the entry points of
csrc/api_prims.hip enforce, and reaches the branch of the primitive it is named after -- a generator bug must not turn a GPU test
into a vacuous one."""
import numpy as np
import pytest

from tests import prim_inputs as P


def test_sort_key_cases_keep_their_shapes():
    assert [c[0] for c in P.sort_key_cases(3, np.random.default_rng(0))] == list(P.SORT_KEY_CASES)
    assert [c[0] for c in P.sort_key_cases(3, np.random.default_rng(0), 32, {"sorted", "uniform"})] == ["uniform", "sorted"]
    for width, dt in ((64, np.uint64), (32, np.uint32)):
        cases = dict(P.sort_key_cases(5000, np.random.default_rng(1), width))
        assert len(cases) == 10
        for name, k in cases.items():
            assert k.dtype == dt and len(k) == 5000, name
        assert len(np.unique(cases["all_equal"])) == 1
        assert set(np.unique(cases["two_values"]).tolist()) == {0, (1 << width) - 1}
        assert len(np.unique(cases["37_values"])) <= 37
        assert int(cases["low_bits_only"].max()) < 1 << 20
        assert not (cases["high_bits_only"] & dt((1 << (width - 20)) - 1)).any() and cases["high_bits_only"].any()
        assert (np.diff(cases["sorted"].astype(np.float64)) >= 0).all() and (np.diff(cases["reversed"].astype(np.float64)) <= 0).all()
        assert (cases["max_keys"] == dt((1 << width) - 1)).sum() > 1000
        # duplicates in every case but the uniform 64-bit one: stability is observable
        assert len(np.unique(cases["heavy_keys"])) < 3000


@pytest.mark.parametrize("begin,end,width", [(0, 1, 32), (0, 13, 32), (5, 21, 32), (24, 32, 32), (11, 12, 64), (32, 47, 64), (57, 64, 64), (0, 64, 64)])
def test_equal_on_bits_keys_collide_on_the_field_only(begin, end, width):
    k = P.equal_on_bits_keys(3000, np.random.default_rng(2), begin, end, width)
    assert len(np.unique(P.sort_field(k, begin, end))) == 1                  # they really collide on the sorted bits
    if end - begin < width:
        assert len(np.unique(k)) > 1                                         # ... and differ elsewhere, so a moved key is seen
    assert np.array_equal(P.stable_order(k, begin, end), np.arange(3000))


def test_sort_field_and_stable_order():
    k = np.array([0x30, 0x1F, 0x3F, 0x10, 0x20], dtype=np.uint32)
    assert P.sort_field(k, 4, 6).tolist() == [3, 1, 3, 1, 2]
    assert P.stable_order(k, 4, 6).tolist() == [1, 3, 4, 0, 2]
    k64 = np.array([1 << 63, 0, (1 << 63) | 5], dtype=np.uint64)
    assert P.sort_field(k64, 0, 64).dtype == np.uint64 and P.stable_order(k64, 63, 64).tolist() == [1, 0, 2]


@pytest.mark.parametrize("begin,end", [(0, 32), (0, 45), (0, 56), (0, 64), (8, 40)])
@pytest.mark.parametrize("n", [1, 2, 9, 2049, 20000])
def test_distinct_on_bits_keys(n, begin, end):
    k = P.distinct_on_bits_keys(n, np.random.default_rng(n + end), begin, end)
    assert k.dtype == np.uint64 and len(k) == n
    f = P.sort_field(k, begin, end)
    assert len(np.unique(f)) == n                                            # the precondition of the distinct sort
    assert int(f.max()) == (1 << (end - begin)) - 1                          # the all-ones field (= the padding key for (0, 64))
    if n >= 2049:                                                            # the bits outside the field are random, not zero
        if begin:
            assert (k & np.uint64((1 << begin) - 1)).any()
        if end < 64:
            assert (k >> np.uint64(end)).any()
        if end < 64:
            assert not np.array_equal(np.argsort(f), np.argsort(k))          # ... and would change the order if they took part


@pytest.mark.parametrize("m,n_dst", [(1, 1), (1000, 1000), (1000, (1 << 20) + 7), ((1 << 20) + 1, (1 << 20) + 7), ((1 << 20) - 1, 1 << 24),
                                     (3 * (1 << 20) + 5, 3 * (1 << 20) + 5), (1000, (1 << 27) + 3)])
def test_distinct_indices(m, n_dst):
    idx = P.distinct_indices(m, n_dst, np.random.default_rng(m))
    assert idx.dtype == np.uint32 and len(idx) == m
    assert len(np.unique(idx)) == m and int(idx.max()) < n_dst
    if m >= 1000:
        assert (np.diff(idx.astype(np.int64)) < 0).any()                     # not sorted: the partition has work to do
    if m >= 1000 and n_dst > (1 << 16):
        assert len(np.unique(idx >> np.uint32(max(0, int(n_dst - 1).bit_length() - 16)))) > 100    # many destination windows


def test_permutation_indices():
    for m in (1, 1000, (1 << 20) + 1):
        idx = P.permutation_indices(m, np.random.default_rng(m))
        assert idx.dtype == np.uint32 and np.array_equal(np.sort(idx), np.arange(m))


@pytest.mark.parametrize("bits,db", [(17, 8), (20, 8), (24, 8), (32, 8), (19, 9), (30, 9), (32, 9)])
def test_msd_indices(bits, db):
    rng = np.random.default_rng(bits)
    for kind, groups in (("uniform", None), ("one_group", 1), ("two_groups", 2)):
        idx = P.msd_indices(50000, bits, db, kind, rng)
        assert idx.dtype == np.uint32 and int(idx.max()) < (1 << bits)
        g = np.unique(idx >> np.uint32(bits - 2 * db))
        if groups:
            assert len(g) == groups
        else:
            assert len(g) > 20000
        assert len(np.unique(idx)) > 1                                       # the low bits vary


def _preconditions(nxt):
    n = len(nxt)
    i = np.arange(n, dtype=np.int64)
    return nxt.dtype == np.uint32 and (nxt.astype(np.int64) > i).all() and (nxt.astype(np.int64) <= n).all()


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, (1 << 20) - 1, (1 << 20) + 1, 3 * (1 << 20) + 17])
@pytest.mark.parametrize("kind", P.ORBIT_KINDS)
def test_orbit_next(kind, n):
    rng = np.random.default_rng(n)
    nxt = P.orbit_next(n, kind, rng)
    assert len(nxt) == n and _preconditions(nxt)
    mark = P.orbit_reference(nxt)
    on = np.flatnonzero(mark)
    assert on[0] == 0
    tiles = np.unique(on // P.ORB_TILE)
    supers = np.unique(on // P.ORB_SUPER)
    ntiles, nsupers = -(-n // P.ORB_TILE), -(-n // P.ORB_SUPER)
    if kind == "step1":
        assert mark.all()                                                    # the chain sits on every element of every tile
    elif kind == "stop_at_0":
        assert len(on) == 1 and nxt[0] == n
    elif kind == "step1024":
        assert len(on) == ntiles and (on % P.ORB_TILE == 0).all()             # one element per tile, always the first slot
    elif kind == "step1023":
        assert np.array_equal(on, np.arange(0, n, 1023))                      # the entry slot walks backwards through the tiles
    elif kind == "tile_last":
        if n >= P.ORB_TILE:
            assert (on[1:] % P.ORB_TILE == P.ORB_TILE - 1).all() and len(on) == 1 + n // P.ORB_TILE
        if n >= P.ORB_SUPER:
            assert mark[P.ORB_SUPER - 1] == 1                                 # the last slot of a super-tile
    elif kind == "super_skip":
        if n > (1 << 21) + 1:
            assert len(supers) < nsupers and len(on) == 2                     # a whole super-tile without an entry
    elif kind == "geometric":
        if n >= 1 << 20:
            assert len(tiles) >= ntiles - 1 and len(on) > n // 80             # several chain elements in every (whole) tile
    if n >= 1025 and kind != "step1":
        off = np.flatnonzero(mark == 0)
        assert len(off) > 0                                                   # elements off the chain exist,
        assert (nxt[off].astype(np.int64) == n).any() or n < 5000             # some of them jump straight to n,
        if kind in ("step1024", "step1023", "tile_last", "geometric"):
            assert mark[np.minimum(nxt[off], n - 1)].any()                    # and some lead onto the chain without being on it


def test_orbit_reference_is_the_serial_walk():
    nxt = np.array([2, 2, 5, 4, 5, 6, 7], dtype=np.uint32)
    assert P.orbit_reference(nxt).tolist() == [1, 0, 1, 0, 0, 1, 1]


def test_tile_entries_reference_is_the_sequential_walk():
    N = P.DX_NONE
    ex = np.array([[1, 0], [N, 1], [0, 0], [1, N], [0, N], [0, 0]], dtype=np.uint16)
    assert P.tile_entries_reference(ex).tolist() == [0, 1, 1, 0, 1, N]
    assert P.tile_entries_reference(np.array([[N]], dtype=np.uint16)).tolist() == [0]      # the first tile is always entered in state 0


def test_tile_entries_array_walk_agrees_with_the_list_walk():
    for ntiles, states in ((1, 1), (7, 2), (P.DX_G + 1, 13), (3 * P.DX_G, 64), (5000, 255)):
        for kind in P.TILE_EXIT_KINDS:
            ex = P.tile_exits(ntiles, states, kind, np.random.default_rng(ntiles))
            a, b = P.tile_entries_reference_array(ex), P.tile_entries_reference(ex)
            assert a.dtype == b.dtype and np.array_equal(a, b), (ntiles, states, kind)
    N = P.DX_NONE
    assert P.tile_entries_reference_array(np.array([[1, 0], [N, 1], [0, 0], [1, N], [0, N], [0, 0]], dtype=np.uint16)).tolist() == [0, 1, 1, 0, 1, N]


def test_tile_exit_cases_cover_the_decoders_widths():
    cases = {(n, s): k for n, s, k in P.TILE_EXIT_CASES}
    assert len(cases) == len(P.TILE_EXIT_CASES) == len(set(P.TILE_EXIT_IDS))
    G = P.DX_G
    for s in (1, 13, 22):
        assert all(cases[(n, s)] == P.TILE_EXIT_KINDS for n in P.TILE_EXIT_NTILES)
    for s in (64, 255):
        assert all(cases[(n, s)] == P.TILE_EXIT_KINDS for n in (1, G - 1, G, G + 1)) and cases[(G * G + 1, s)] == ("random",)


@pytest.mark.parametrize("ntiles,states,kinds", P.TILE_EXIT_CASES, ids=P.TILE_EXIT_IDS)
def test_tile_exits(ntiles, states, kinds):
    G = P.DX_G
    for kind in kinds:
        ex = P.tile_exits(ntiles, states, kind, np.random.default_rng(ntiles + states))
        assert ex.dtype == np.uint16 and ex.shape == (ntiles, states)
        assert ((ex < states) | (ex == P.DX_NONE)).all(), kind                # the precondition of the entry point
        entry = P.tile_entries_reference(ex) if ex.size <= 1 << 24 else P.tile_entries_reference_array(ex)
        assert len(entry) == ntiles and entry[0] == 0
        ended = np.flatnonzero(entry == P.DX_NONE)
        assert (entry[:ended[0] if len(ended) else ntiles] < states).all()
        assert len(ended) == 0 or (entry[ended[0]:] == P.DX_NONE).all()       # an ended chain stays ended
        if kind == "no_none":
            assert len(ended) == 0 and (ex != P.DX_NONE).all()
            if states > 1 and ntiles >= G:
                # the chain really moves through the states (about G draws: all of a few states, most of the huff decoder's many)
                assert len(np.unique(entry)) == states if states <= 22 else len(np.unique(entry)) > states // 2
        elif kind == "all_none":
            assert len(ended) == ntiles - 1
        elif kind == "ends_in_first_group":
            assert (len(ended) == 0) == (ntiles <= P.TILE_EXIT_END + 1)
            assert len(ended) == 0 or ended[0] == P.TILE_EXIT_END + 1 < G
        elif ntiles >= G * G - 1:                                             # random: ends, but only after several groups
            assert len(ended) > 0 and ended[0] > 3 * G and (ex == P.DX_NONE).sum() > 10
        else:
            assert len(ended) == 0


@pytest.mark.parametrize("want", [0, 3, 255])
def test_select_classes(want):
    rng = np.random.default_rng(want)
    m = 200000
    counts = {d: int((P.select_classes(m, want, d, rng) == want).sum()) for d in P.SELECT_DENSITIES}
    assert counts["none"] == 0 and counts["all"] == m
    assert 50 < counts["sparse"] < 500 and 0.45 * m < counts["half"] < 0.55 * m
    assert len(np.unique(P.select_classes(m, want, "half", rng))) > 3        # other classes than `want` are present
