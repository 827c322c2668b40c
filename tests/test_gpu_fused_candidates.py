"""GPU tests (pytest -m gpu) of the passes folded into the kernels that already hold their data: the candidate classification inside
the image kernel of the fused ISA/PLCP scatter (option fused_cand) and the first candidate selection that is handed its per-tile
counts by that kernel (option sel_tile_counts).  Every case compresses with the options on and with them off, compares the two
streams and the statistics that describe the factorization, and compares the stream with the oracle's.  The texts are the smallest
at which the folded code runs at all (2^20 bytes: wide suffix sort, fused scatter, window pass), with lengths and contents chosen
for its edges; select_by_class with supplied counts is also driven alone (csrc/api_prims.hip) and compared with numpy."""
import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus

pytestmark = pytest.mark.gpu

M20 = 1 << 20
OFF = {"fused_cand": 0, "sel_tile_counts": 0}
STATS = ("factors", "entries", "num_flattened", "window_pass", "window_lcut", "maxlcp", "sa_mode")


@pytest.fixture(scope="module")
def ctx_on():
    with T.Context(0) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def ctx_off():
    with T.Context(0, options=OFF) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def ctx_no_counts():
    """the image kernel classifies, select_by_class counts itself"""
    with T.Context(0, options={"sel_tile_counts": 0}) as ctx:
        yield ctx


def _both(ctx_on, ctx_off, text, thr, what):
    """compress with the folded passes and without; the streams, the statistics and the oracle's stream agree.  Returns the statistics."""
    want, _ = O.lcpcomp_huff_compress(text, thr, 1)
    on, st_on = ctx_on.lcpcomp_compress(text, threshold=thr, flatten=1)
    off, st_off = ctx_off.lcpcomp_compress(text, threshold=thr, flatten=1)
    assert on == off, "%s t=%d: %d vs %d bytes with the options on / off" % (what, thr, len(on), len(off))
    assert on == want, "%s t=%d: %d bytes, the oracle writes %d" % (what, thr, len(on), len(want))
    for k in STATS:
        assert st_on[k] == st_off[k], "%s t=%d: %s %d vs %d" % (what, thr, k, st_on[k], st_off[k])
    return st_on


def _english(n_text, seed):
    """English-like text whose escaped, 0-terminated view has n_text bytes"""
    text = O.escape(T.gen_english(n_text - 1, seed).tobytes())
    assert len(text) == n_text
    return text


def _plant(data, src, dst, length):
    out = bytearray(data)
    out[dst:dst + length] = out[src:src + length]
    return bytes(out)


# n not a multiple of 4 (the words of class bytes), of 2 048 (selection tile), of 4 096 (owner tile), of 8 192 (the largest window); the
# last window, tile and group of four are partial
@pytest.mark.parametrize("n_text", [M20 + 1, M20 + 8191 + 3])
@pytest.mark.parametrize("thr", [2, 5])
def test_edge_lengths(ctx_on, ctx_off, n_text, thr):
    st = _both(ctx_on, ctx_off, _english(n_text, 11), thr, "english n=%d" % n_text)
    assert st["sa_mode"] == 1 and st["window_pass"] == 1, st


def test_one_list_above_the_cut_and_a_factor_across_a_tile_border(ctx_on, ctx_off, ctx_no_counts):
    """One planted copy of 100 bytes: the list of the levels above the window pass's cut is non-empty in the few selection tiles the
    two occurrences touch and empty everywhere else.  Both occurrences straddle a border of the 4 096-position tiles of build_owner
    (and so of the 2 048-position selection tiles), whichever of them becomes the factor."""
    data = T.gen_english(M20 + 100, 12).tobytes()
    data = _plant(data, 4096 * 50 - 50, 4096 * 200 - 50, 100)
    text = O.escape(data)
    for thr in (2, 5):
        st = _both(ctx_on, ctx_off, text, thr, "planted copy")
        assert st["window_pass"] == 1 and st["window_lcut"] < st["maxlcp"] < 250, st
    got, st2 = ctx_no_counts.lcpcomp_compress(text, threshold=2, flatten=1)
    assert got == O.lcpcomp_huff_compress(text, 2, 1)[0]


def test_wide_alphabet_below_the_cut_and_no_candidate_at_all(ctx_on, ctx_off):
    """maxlcp below the cut the image kernel classifies against: no class-1 byte anywhere, every tile count 0.  With a threshold above
    maxlcp there is no candidate at all (the early return of factorize_arrays; the length bytes are the image kernel's zeros)."""
    text = O.escape(corpus.alphabet_text(M20 + 77, 200, seed=4).tobytes())
    st = _both(ctx_on, ctx_off, text, 2, "sigma 200")
    assert st["sa_mode"] == 1 and 2 <= st["maxlcp"] < 56, st
    st = _both(ctx_on, ctx_off, text, st["maxlcp"] + 1, "sigma 200, threshold above maxlcp")
    assert st["factors"] == 0 and st["entries"] == 0, st


def test_threshold_1_takes_the_dense_length_array(ctx_on, ctx_off):
    """threshold 1: no byte lengths, no early encoder -- the image kernel zero-fills the dense array instead; tiles of build_owner may hold
    more starts than half their positions"""
    st = _both(ctx_on, ctx_off, _english(M20 + 1, 13), 1, "english")
    assert st["sa_mode"] == 1, st


def test_doubling_fallback_does_not_take_the_folded_code(ctx_on, ctx_off):
    """DNA-like text with copied blocks: the suffix sort falls back to doubling (sa_mode 0), there is no fused scatter and the
    classification stays with cand_class_kernel whatever the options say"""
    rng = np.random.default_rng(3)
    blk = bytes(rng.integers(0, 4, 40_000, dtype=np.uint8).astype(np.uint8) + 65)
    data = T.gen_dna(900_000, 5).tobytes() + blk + b"#" + blk[100:30_000] + T.gen_dna(M20 - 900_000 - 40_000 - 1 - 29_900 - 35_000, 6).tobytes() + blk[5_000:]
    assert len(data) == M20
    st = _both(ctx_on, ctx_off, O.escape(data), 2, "dna with copied blocks")
    assert st["sa_mode"] == 0, st


# ---- select_by_class with supplied counts ----------------------------------------------------------------------------------------
TILE = 2048
FILL = 0xABCD1234


def _counts(cls, want):
    m = len(cls)
    return np.array([np.count_nonzero(cls[t:t + TILE] == want) for t in range(0, m, TILE)], dtype=np.uint32)


@pytest.mark.parametrize("m", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_select_with_supplied_counts(gpu_ctx, m):
    rng = np.random.default_rng(m)
    tiles = (m + TILE - 1) // TILE
    patterns = {"absent": np.zeros(m, dtype=np.uint8)}
    one = np.zeros(m, dtype=np.uint8)
    lo = (tiles - 1) * TILE                                     # the last (partial) tile only
    one[lo:] = rng.integers(0, 3, m - lo, dtype=np.uint8)
    one[m - 1] = 1
    patterns["last_tile_only"] = one
    first = np.zeros(m, dtype=np.uint8)
    first[:min(m, TILE)] = rng.integers(0, 3, min(m, TILE), dtype=np.uint8)
    first[0] = 1
    patterns["first_tile_only"] = first
    every = rng.integers(0, 3, m, dtype=np.uint8)
    every[::TILE] = 1
    every[m - 1] = 1
    patterns["every_tile"] = every
    patterns["all"] = np.ones(m, dtype=np.uint8)
    src = rng.integers(0, 1 << 32, m, dtype=np.uint32)
    for name, cls in patterns.items():
        idx = np.flatnonzero(cls == 1).astype(np.uint32)
        cnts = _counts(cls, 1)
        for with_src in (False, True):
            ref = src[idx] if with_src else idx
            oa, cnt = gpu_ctx.prim_select_counts(cls, 1, cnts, src if with_src else None, FILL)
            assert cnt == len(idx), (name, with_src)
            assert np.array_equal(oa[:cnt], ref), (name, with_src)
            assert np.all(oa[cnt:] == FILL), (name, with_src)   # nothing is written behind the count
            ob, _, cnt2 = gpu_ctx.prim_select(cls, 1, src if with_src else None, None, FILL)
            assert cnt2 == cnt and np.array_equal(ob, oa), (name, with_src)


def test_select_refuses_counts_that_are_not_the_tiles(gpu_ctx):
    cls = np.zeros(TILE + 3, dtype=np.uint8)
    cls[5] = 1
    with pytest.raises(T.TdcGpuError):
        gpu_ctx.prim_select_counts(cls, 1, np.array([0, 1], dtype=np.uint32))
