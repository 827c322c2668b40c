"""Input generators of the primitive tests (tests/test_gpu_prims.py, tests/test_gpu_sort.py) and the plain references they are
compared with.  tests/test_prim_inputs.py checks on the CPU that every generator meets the preconditions the entry points of
csrc/api_prims.hip enforce and reaches the branch it is meant for, so that a generator bug cannot turn a GPU test into a vacuous one.

The constants are the ones of csrc/prim.hip ("Where the primitives fork")."""
import numpy as np

STILE = 4096                 # scan: elements per workgroup; one level up to STILE, two up to STILE^2, three above
RS_TILE = 4096               # radix sort: pairs per four-wave tile (8192 with radix_waves = 8 from 2^22 pairs)
SEL_TILE = 2048              # select_by_class
ORB_TILE = 1024              # mark_orbit_u32
ORB_SUPER = 1 << 20
SMALL_SORT_MAX = 2048        # sort_pairs_u64_distinct: bitonic up to here,
MID_SORT_MAX = 8192          # one-workgroup radix up to here
SCATTER_MIN = 1 << 20        # bucketed_scatter_u32 partitions from this many pairs
DX_G = 512                   # dx_entries (csrc/tile_chain.hpp): tiles per group, groups per group of groups
DX_NONE = 0xFFFF             # "the chain ends in this tile"


def _mask(bits):
    return (1 << bits) - 1


# ---- keys of the sorts -----------------------------------------------------------------------------------------------------------
SORT_KEY_CASES = ("uniform", "low_bits_only", "high_bits_only", "all_equal", "two_values", "37_values", "heavy_keys", "sorted", "reversed",
                  "max_keys")


def sort_key_cases(n, rng, width=64, only=None):
    """(name, keys) distributions that stress a sort: heavy keys, all keys equal, few distinct keys, sorted / reversed input, keys
    that differ only in the high or only in the low bits.  width 64 -> uint64, 32 -> uint32; only: the names wanted (None: all)."""
    dt = np.uint64 if width == 64 else np.uint32
    top = 1 << width
    ones = dt(top - 1)

    def uni(size=n):
        return rng.integers(0, top, size=size, dtype=dt)

    def few_values():
        few = uni(37)
        return few[rng.integers(0, 37, size=n)]

    def heavy_keys():   # Zipf-like: half of the pairs share 5 heavy keys, the rest is uniform (the shape of text keys)
        z = uni()
        heavy = uni(5)
        m = rng.random(n) < 0.5
        z[m] = heavy[rng.integers(0, 5, size=int(m.sum()))]
        return z

    make = {
        "uniform": uni,
        "low_bits_only": lambda: rng.integers(0, 1 << 20, size=n, dtype=dt),
        "high_bits_only": lambda: rng.integers(0, 1 << 20, size=n, dtype=dt) << dt(width - 20),
        "all_equal": lambda: np.full(n, 0x0123456789ABCDEF & (top - 1), dtype=dt),
        "two_values": lambda: rng.integers(0, 2, size=n, dtype=dt) * ones,
        "37_values": few_values,
        "heavy_keys": heavy_keys,
        "sorted": lambda: np.sort(uni()),
        "reversed": lambda: np.sort(uni())[::-1].copy(),
        "max_keys": lambda: np.where(rng.random(n) < 0.3, ones, uni()),
    }
    for name in SORT_KEY_CASES:
        if only is None or name in only:
            yield name, make[name]()


def equal_on_bits_keys(n, rng, begin, end, width=64):
    """keys that all agree on bits [begin, end) and are random elsewhere: a stable sort on those bits must return them untouched"""
    dt = np.uint64 if width == 64 else np.uint32
    k = rng.integers(0, 1 << width, size=n, dtype=dt)
    field = dt(_mask(end - begin) << begin)
    pattern = dt((0x5A5A5A5A5A5A5A5A & _mask(end - begin)) << begin)
    return (k & ~field) | pattern


def sort_field(keys, begin, end):
    """(keys >> begin) & mask in the narrowest unsigned type that holds it (numpy sorts narrow integers much faster)"""
    w = end - begin
    f = (keys >> keys.dtype.type(begin)) & keys.dtype.type(_mask(w))
    return f.astype(np.uint16 if w <= 16 else np.uint32 if w <= 32 else np.uint64)


def stable_order(keys, begin, end):
    """the order a stable sort on bits [begin, end) produces"""
    return np.argsort(sort_field(keys, begin, end), kind="stable")


def distinct_on_bits_keys(n, rng, begin, end):
    """uint64 keys that are pairwise distinct on bits [begin, end), with random bits below begin and above end.  The largest field
    value (all ones) is always among them: with (0, 64) that key equals the padding of the in-LDS sorts."""
    w = end - begin
    assert n <= (1 << w)
    got = np.empty(0, dtype=np.uint64)
    while len(got) < n:
        draw = rng.integers(0, 1 << 64, size=2 * n + 16, dtype=np.uint64) & np.uint64(_mask(w))
        got = np.unique(np.concatenate([got, draw]))
    field = rng.permutation(got)[:n]
    if not (field == np.uint64(_mask(w))).any():
        field[int(rng.integers(0, n))] = np.uint64(_mask(w))
    noise = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    keep = np.uint64(_mask(w) << begin)
    return (noise & ~keep) | (field << np.uint64(begin))


# ---- indices of the scatters -----------------------------------------------------------------------------------------------------
def distinct_indices(m, n_dst, rng):
    """m pairwise distinct uint32 indices < n_dst in random order"""
    assert m <= n_dst
    if 2 * m >= n_dst:
        return rng.permutation(n_dst)[:m].astype(np.uint32)
    got = np.empty(0, dtype=np.int64)
    while len(got) < m:
        got = np.unique(np.concatenate([got, rng.integers(0, n_dst, size=m + m // 4 + 16)]))
    return rng.permutation(got)[:m].astype(np.uint32)


def permutation_indices(m, rng):
    """every index of [0, m) once (what `permutation = true` promises)"""
    return rng.permutation(m).astype(np.uint32)


def msd_indices(m, bits, db, kind, rng):
    """uint32 indices < 2^bits: "uniform", "one_group" (all share their top 2 * db bits) or "two_groups" """
    low = bits - 2 * db
    if kind == "uniform":
        return rng.integers(0, 1 << bits, size=m, dtype=np.uint64).astype(np.uint32)
    tail = rng.integers(0, 1 << low, size=m, dtype=np.uint64)
    groups = np.array([(1 << (2 * db)) - 1] if kind == "one_group" else [3, (1 << (2 * db)) - 2], dtype=np.uint64)
    g = groups[rng.integers(0, len(groups), size=m)]
    return ((g << np.uint64(low)) | tail).astype(np.uint32)


# ---- successor functions of the orbit --------------------------------------------------------------------------------------------
ORBIT_KINDS = ("step1", "step1024", "step1023", "super_skip", "geometric", "tile_last", "stop_at_0")


def orbit_chain(n, kind, rng):
    """the chain (ascending positions, first one 0) of a kind"""
    if kind == "stop_at_0":
        return np.zeros(1, dtype=np.int64)
    if kind == "tile_last":          # 0, then the last slot of every tile -- that of every super-tile among them
        return np.concatenate([[0], np.arange(ORB_TILE - 1, n, ORB_TILE)]).astype(np.int64) if n > 1 else np.zeros(1, dtype=np.int64)
    if kind == "geometric":
        jumps = rng.geometric(1.0 / 40, size=n // 8 + 8)
        pos = np.concatenate([[0], np.cumsum(jumps)])
        return pos[pos < n].astype(np.int64)
    step = {"step1": 1, "step1024": 1024, "step1023": 1023, "super_skip": (1 << 21) + 1}[kind]
    return np.arange(0, n, step, dtype=np.int64)


def orbit_next(n, kind, rng):
    """next[] (uint32, i < next[i] <= n) whose orbit of 0 is orbit_chain(n, kind); the elements off the chain get random valid
    successors -- short jumps, long ones and a few straight to n -- that must not become marked"""
    chain = orbit_chain(n, kind, rng)
    i = np.arange(n, dtype=np.int64)
    jump = rng.geometric(1.0 / 30, size=n).astype(np.int64)
    far = rng.random(n) < 0.02
    jump[far] = rng.integers(1, max(2, n), size=int(far.sum()))
    nxt = np.minimum(i + jump, n)
    nxt[rng.random(n) < 0.01] = n
    nxt[chain] = np.concatenate([chain[1:], [n]])
    return nxt.astype(np.uint32)


def orbit_reference(nxt):
    """the serial walk from 0"""
    n = len(nxt)
    mark = np.zeros(n, dtype=np.uint8)
    steps = nxt.tolist()
    on = []
    e = 0
    while e < n:
        on.append(e)
        e = steps[e]
    mark[on] = 1
    return mark


# ---- tile exits of the decoders' tile scheme --------------------------------------------------------------------------------------
TILE_EXIT_NTILES = (1, DX_G - 1, DX_G, DX_G + 1, DX_G * DX_G - 1, DX_G * DX_G, DX_G * DX_G + 1)     # the group borders of every level
TILE_EXIT_STATES = (1, 13, 22)                                                                       # sle's fewest, sle's most, rle
TILE_EXIT_KINDS = ("random", "no_none", "all_none", "ends_in_first_group")
TILE_EXIT_WIDE_STATES = (64, 255)                                                                    # encode(huff): its longest code, up to 255
# (ntiles, states, kinds): the widths of sle and rle at every group border; the huff decoder's at the borders of the first level with
# every kind and once at three levels (a table of 134 MB at 255 states)
TILE_EXIT_CASES = tuple((n, s, TILE_EXIT_KINDS) for s in TILE_EXIT_STATES for n in TILE_EXIT_NTILES) + \
    tuple((n, s, TILE_EXIT_KINDS) for s in TILE_EXIT_WIDE_STATES for n in TILE_EXIT_NTILES[:4]) + \
    tuple((DX_G * DX_G + 1, s, ("random",)) for s in TILE_EXIT_WIDE_STATES)
TILE_EXIT_IDS = ["%d-%d" % c[:2] for c in TILE_EXIT_CASES]
TILE_EXIT_END = 100          # "ends_in_first_group": the tile whose exits are all NONE


def tile_exits(ntiles, states, kind, rng):
    """(ntiles, states) uint16: exit[t][o] = the state in which the chain that enters tile t in state o enters tile t + 1, DX_NONE: it
    ends in t.  "random": about 1 NONE in 4096 and none on the chain's way through the first three groups, so that the chain from
    state 0 crosses several groups and ends in a large table"""
    if kind == "all_none":
        return np.full((ntiles, states), DX_NONE, dtype=np.uint16)
    ex = rng.integers(0, states, size=(ntiles, states), dtype=np.uint16)
    if kind == "random":
        if ntiles * states <= 1 << 24:
            ex[rng.random((ntiles, states)) < 1.0 / 4096] = DX_NONE
        else:                                                                 # the same density without a float per entry
            ex.reshape(-1)[rng.integers(0, ntiles * states, size=ntiles * states // 4096)] = DX_NONE
        e = 0
        for t in range(min(ntiles, 3 * DX_G)):
            if ex[t, e] == DX_NONE:
                ex[t, e] = rng.integers(0, states)
            e = int(ex[t, e])
    elif kind == "ends_in_first_group":
        ex[min(TILE_EXIT_END, ntiles - 1)] = DX_NONE
    return ex


def tile_entries_reference(exits):
    """the sequential definition: e = 0; for every tile t: entry[t] = e, then e = exit[t][e] unless e is NONE"""
    rows = exits.tolist()
    entry = []
    e = 0
    for row in rows:
        entry.append(e)
        if e != DX_NONE:
            e = row[e]
    return np.array(entry, dtype=np.uint16)


def tile_entries_reference_array(exits):
    """the same walk on the array itself: no list of the whole table (134 MB at 2^18 tiles of 255 states)"""
    entry = np.full(len(exits), DX_NONE, dtype=np.uint16)
    e = 0
    for t in range(len(exits)):
        entry[t] = e
        e = int(exits[t, e])
        if e == DX_NONE:
            break
    return entry


# ---- classes of the selection ----------------------------------------------------------------------------------------------------
SELECT_DENSITIES = ("none", "all", "sparse", "half")


def select_classes(m, want, density, rng):
    """class bytes of which none / all / about 1 in 1 000 / about one half equal `want`"""
    others = np.array([v for v in (0, 1, 3, 7, 128, 254, 255) if v != want], dtype=np.uint8)
    cls = others[rng.integers(0, len(others), size=m)]
    if density == "all":
        cls[:] = want
    elif density != "none":
        cls[rng.random(m) < (0.001 if density == "sparse" else 0.5)] = want
    return cls
