"""CPU tests of tests/arena_cases.py: every case's want() computes here, and every input reaches the fork its name claims -- text
sizes against wsort_min, flush-free segment lengths against ARITH_STEP_CAP, batch borders against the 4096-position tile, dec_seg
against the streams' bit lengths, the primitives' sizes against the constants of csrc/prim.hip -- so that a slip in the table cannot
turn tests/test_gpu_arena_state.py into a vacuous test.  The numbers come from the sources of the library where it defines them."""
import os

import numpy as np
import pytest

import tudocomp_amd as T
from tests import arena_cases as A
from tests import factor_lists as FL
from tests import lzss_sw_batches as B
from tests import prim_inputs as P
from tests.test_gpu_alphabets import _arith_model, _segment_lengths

FAMILIES = ("lcpcomp", "arith", "stages", "lcpdec", "lz78", "lzw", "bwt", "pipeline", "lzss", "lzss_batch", "repair", "prims", "blocks")


def _names(family):
    return [c.name for c in A.CASES if c.family == family]


def test_table_shape():
    assert A.FAMILIES == FAMILIES
    assert len({c.name for c in A.CASES}) == len(A.CASES)
    known = open(os.path.join(A.ROOT, "tudocomp_amd", "csrc", "api_ctx.hip")).read()
    for c in A.CASES:
        assert c.name.startswith(c.family + "-") and callable(c.run) and callable(c.want)
        for name in c.options:                                                   # (an unknown option would raise on the GPU only)
            assert '{ "%s",' % name in known, (c.name, name)
    # what the shuffled test runs on one context: every family but the device decoders with small segments
    assert {c.family for c in A.CASES if c.default_options} == set(FAMILIES) - {"lcpdec"}
    assert A.FILLS == (0x00, 0x01, 0xFF)


@pytest.mark.parametrize("family", FAMILIES)
def test_every_want_computes(family):
    for c in A.CASES:
        if c.family != family:
            continue
        w = c.want()
        assert isinstance(w, tuple) and len(w) >= 1, c.name
        assert A.same(w, c.want()) and A.first_difference(w, w) == "equal", c.name
        for part in w:
            assert isinstance(part, (bytes, int, np.integer, np.ndarray, list, type(None))), (c.name, type(part))


def test_comparison_helpers_see_a_single_wrong_element():
    a = (b"abc", np.arange(5, dtype=np.uint32), [b"x", b""], 7)
    assert A.same(a, (b"abc", np.arange(5, dtype=np.uint32), [b"x", b""], 7))
    for b in ((b"abd", a[1], a[2], 7), (b"abc", np.array([0, 1, 2, 3, 5], dtype=np.uint32), a[2], 7), (b"abc", a[1], [b"x", b"y"], 7),
              (b"abc", a[1], a[2], 8), (b"abc", a[1], a[2]), (b"abcd", a[1], a[2], 7)):
        assert not A.same(b, a) and A.first_difference(b, a) != "equal"
    assert "first difference at 2" in A.first_difference((b"abd",), (b"abc",))


# ---- lcpcomp ------------------------------------------------------------------------------------------------------------------------
def test_lcpcomp_texts_lie_on_both_sides_of_the_wide_sort():
    wsort_min = A.source_constant("common.hpp", r"size_t wsort_min = ([^;]+);")
    assert wsort_min == 1 << 20
    small, english, dna = (A.text_of(k) for k in A.LCP_TEXTS)
    assert 150_000 <= len(small) <= 260_000 and len(small) < wsort_min           # about 200 KB: the classic suffix sort
    assert len(english) >= 3_000_000 and len(dna) >= 1_500_000 and min(len(english), len(dna)) >= wsort_min
    assert set(A.WIDE_MODE) == {"english3M", "dna1M5"} and set(A.WIDE_MODE.values()) == {0, 1}
    for t in (small, english, dna):
        assert t[-1] == 0 and t.count(0) == 1                                    # the escaped, 0-terminated view


def test_lcpcomp_matrix_covers_the_supported_pairs():
    names = _names("lcpcomp")
    for kind in A.LCP_TEXTS:
        for coder in A.LCP_CODERS:
            for comp in A.LCP_COMPS:
                hit = [n for n in names if n.startswith("lcpcomp-%s-%s-%s-" % (kind, coder, comp))]
                assert len(hit) == (0 if comp == "heap" and kind not in A.HEAP_TEXTS else 1), (kind, coder, comp)
    for coder in A.LCP_CODERS:                                                   # every coder meets every threshold and both flatten values
        mine = [n for n in names if "-%s-" % coder in n]
        assert {n.split("-")[-2] for n in mine} == {"t1", "t2", "t5"} and {n.split("-")[-1] for n in mine} == {"f0", "f1"}, coder
    assert set(A.LCP_CODERS) == {"huff", "arithmetic", "ascii", "sle3"} and set(A.LCP_COMPS) == {"arrays", "max_lcp", "plcppeaks", "heap"}


@pytest.mark.parametrize("m,side", [(44, "below"), (43, "above")])
def test_arithmetic_segments_lie_around_the_step_cap(m, side):
    cap = A.source_constant("arith.hip", r"constexpr u32 ARITH_STEP_CAP = ([^;]+);")
    text = A.text_of("arith_m%d" % m)
    assert 15_000 <= len(text) <= 16_000
    lits = np.frombuffer(text, dtype=np.uint8)
    C, min_range, tot = _arith_model(lits)
    longest = int(_segment_lengths(lits, C, min_range, tot, cap + 512).max())
    overflow = longest - 1 > cap                                                 # arith_next_flush_kernel: ++steps > ARITH_STEP_CAP
    if side == "below":
        assert cap - 64 <= longest and not overflow, longest                     # the parallel segments
    else:
        assert overflow and longest <= cap + 256, longest                        # the sequential pass


# ---- stages, decoders ---------------------------------------------------------------------------------------------------------------
def test_stage_inputs():
    text, f, flat, nf, md = A.stage_reference("text")
    assert text == A.text_of("levels200k") and len(f) > 1000 and nf > 0 and md >= 1
    assert (flat["src"] != f["src"]).any()                                       # flatten has something to do
    assert A.FACTOR_LIST in [c[0] for c in FL.cases("gpu")]
    text, f, flat, nf, md = A.stage_reference("list")
    FL.check_list(len(text), f["pos"], f["src"], f["len"])
    assert (f["src"] > f["pos"]).any() and (f["src"] < f["pos"]).any() and nf > 0          # forward and backward sources, chains
    assert FL.resolve(len(text), _literals(text, f), f["pos"], flat["src"], f["len"]) == text


def _literals(text, f):
    lit = np.frombuffer(text, dtype=np.uint8).copy()
    for p, l in zip(f["pos"].tolist(), f["len"].tolist()):
        lit[p:p + l] = 0
    return lit


def test_decoder_streams_span_many_segments():
    floor = int(A.source_constant("api_ctx.hip", r'"dec_seg",[^\n]*?v < (\d+) \?'))
    assert A.DEC_SEG == floor                                                    # a smaller value would be raised to this one
    for algo, coder in (("lcpcomp", "huff"), ("lcpcomp", "sle"), ("lzss_lcp", "bit"), ("lzss_lcp", "gamma"), ("lzss_lcp", "delta")):
        bits = 8 * len(A.dec_stream(algo, coder))
        assert bits >= 100 * A.DEC_SEG, (algo, coder, bits)                      # hundreds of segments
    assert T.lzss_decode(A.dec_stream("lzss_lcp", "gamma"), T.CODER_GAMMA) == A.text_of("levels200k")
    for name in A.LZ_INPUTS:
        data = A.lz_input(name)
        assert data == max((d for _, d in A.corpus.small_corpus()), key=len) + b"a" * 70_000 and len(data) == 100_000
        for z in (A.O.lz78_gamma_compress(data), A.lzw_stream(name, "bit"), A.lzw_stream(name, "gamma")):
            assert 8 * len(z) > 2 * A.DEC_SEG, name
    data = B.batch("one")[0]
    for coder in ("bit", "gamma", "delta"):
        for w, t in A.LZSS_DEC:
            status, streams = B.expected((data,), w, t, coder)
            assert status == [0] and 8 * len(streams[0]) > 2 * A.DEC_SEG, (coder, w, t)
            assert T.lzss_sw_decode(streams[0], B.CODER_ID[coder], w) == data
    for name, several in (("ties", True), ("english64k", True), ("ab4097a", False)):     # (ab)^4097 a is a grammar of a dozen rules
        for coder, cid in (("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA)):
            z = A.repair_stream(name, coder)
            assert T.repair_decode(z, cid) == A.repair_text(name)
            assert (8 * len(z) > A.DEC_SEG) == several, (name, coder, len(z))


# ---- bwt, pipelines -----------------------------------------------------------------------------------------------------------------
def test_bwt_texts():
    e = A.bwt_text("english200k")
    assert len(e) > 200_000 and b"\xff\xfe" in e and e[-1] == 0                  # escaped 0x00 / 0xFF pairs
    assert A.bwt_text("run70000") == b"a" * 70_000 + b"\0"
    f = A.bwt_text("fib22")
    assert set(f) == {0, ord("a"), ord("b")} and len(f) > 20_000
    for name in ("english200k", "run70000", "fib22"):
        assert len(A.bwt_of(name)) == len(A.bwt_text(name)) and A.bwt_of(name).count(0) == 1


def test_pipeline_inputs_sit_on_the_mtf_workgroup_border():
    assert A.MTF_GROUP == 256 * A.source_constant("bytestages.hpp", r"MTF_CHUNK = (\d+),")
    inputs = A.pipe_inputs()
    assert tuple(inputs) == A.PIPE_NAMES
    assert sorted(len(v) for k, v in inputs.items() if k.startswith("random")) == [A.MTF_GROUP * k + d for k in (1, 2) for d in (-1, 0, 1)]
    assert sorted(len(v) for k, v in inputs.items() if k.startswith("mod251")) == [A.MTF_GROUP * k + d for k in (1, 2) for d in (-1, 0, 1)]
    assert len(set(inputs["sigma1-100000"])) == 1
    assert all(len(set(v)) == 256 for k, v in inputs.items() if k.startswith("random"))
    assert set(A.CHAIN_NAMES) <= set(A.PIPE_NAMES)
    names = _names("pipeline")
    for chain in A.CHAINS:
        for direction in ("compress", "decompress"):
            want = A.CHAIN_NAMES if chain.startswith("bwtzip") else A.PIPE_NAMES
            assert [n for n in names if n.startswith("pipeline-%s-%s-" % (chain, direction))] == ["pipeline-%s-%s-%s" % (chain, direction, x) for x in want]
    # the host loops invert every model stream; a huff stream of all 256 byte values at one code length is refused by them too
    for name in A.PIPE_NAMES:
        w = A.BY_NAME["pipeline-huff-decompress-" + name].want()
        assert w == ((-2,) if name.startswith("random") else (inputs[name],)), name
    for name in A.CHAIN_NAMES:
        data, outs = A.pipe_stage_outputs("bwtzip", name)
        assert T.rle_decode(T.mtf_decode(T.huff_decode_literals(outs[3])), 0) == outs[0] and data == T.escape(inputs[name])
        data, outs = A.pipe_stage_outputs("bwtzip_sle", name)
        assert T.sle_decode_literals(outs[3], 3) == outs[2] == A.pipe_stage_outputs("bwtzip", name)[1][2]


# ---- lzss, repair, blocks -----------------------------------------------------------------------------------------------------------
def test_lzss_inputs_cross_the_tile():
    tile = A.source_constant("lzss_sw_batch.hip", r"constexpr u32 SWB_TILE = (\d+);")
    assert tile == B.TILE == A.source_constant("lzss_sw.hip", r"constexpr u32 SW_TILE = (\d+);")
    assert len(B.batch("one")[0]) == 3 * tile + 17
    ends = np.cumsum([len(x) for x in B.batch("tile_edges")]).tolist()
    for border in (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1):
        assert border in ends, border
    empties = [len(x) for x in B.batch("empties")]
    assert empties[0] == 0 and empties[-1] == 0 and max(np.diff(np.flatnonzero(np.array(empties) > 0))) > 2048     # a long run of empty texts
    widths = B.batch("widths")
    assert len(widths) == 40 and {len(x) for x in widths} == {300}
    for w in (16, 4096):                                                         # no length of the single text is truncated by coder=bit
        for t in (0, 3):
            assert B.expected((B.batch("one")[0],), w, t, "bit")[0] == [0]


def test_repair_inputs():
    ties, ab, eng = (A.repair_text(n) for n in ("ties", "ab4097a", "english64k"))
    assert ab == b"ab" * 4097 + b"a" and len(eng) == 64 << 10 and len(ties) == 1024
    pairs = np.frombuffer(eng, dtype=np.uint8).astype(np.uint32)
    assert len(np.unique(pairs[:-1] << 8 | pairs[1:])) > 1 << A.REPAIR_OPTIONS["table8"]["repair_table_bits"]     # more digrams than slots: a rebuild
    r, s = A.repair_host(ties)
    assert len(r) > 100


def test_blocks_input():
    data = A.blocks_data()
    assert len(data) == 3 * A.MiB and A.BLOCK == A.MiB + 777
    assert -(-len(data) // A.BLOCK) == 3 and len(data) % A.BLOCK not in (0, A.BLOCK)      # a ragged last block
    assert b"\x00" in data and b"\xff" in data                                   # something to escape


# ---- primitives ---------------------------------------------------------------------------------------------------------------------
def test_primitive_sizes_sit_behind_their_forks():
    S = P.STILE
    assert S == A.source_constant("prim.hip", r"constexpr int STILE = (\d+);")
    assert P.SEL_TILE == A.source_constant("prim.hpp", r"SEL_TILE_CLASSES = (\d+);")
    assert (P.ORB_TILE, P.ORB_SUPER) == (A.source_constant("prim.hip", r"constexpr int ORB_TILE = (\d+),"),
                                         A.source_constant("prim.hip", r"ORB_SUPER = ([^;]+);"))
    Z = A.PRIM_SIZES
    assert S < Z["scan"] <= S * S and Z["scan"] % S and Z["scan3"] > S * S
    assert Z["sort_pairs"] > 64 * P.RS_TILE and Z["sort_pairs"] % P.RS_TILE
    assert P.SMALL_SORT_MAX < Z["distinct_mid"] <= P.MID_SORT_MAX < Z["distinct_big"]
    assert Z["scatter"] >= P.SCATTER_MIN
    assert -(-Z["select"] // P.SEL_TILE) > 4096 and Z["select"] % 8
    assert Z["orbit"] > P.ORB_SUPER
    assert Z["tile_entries"][0] > P.DX_G * P.DX_G and Z["tile_entries"][1] in P.TILE_EXIT_STATES
    assert Z["sort_u64"] > 1 << 20


def test_primitive_inputs_meet_the_preconditions():
    keys, vals = A.prim_input("distinct_big")
    assert len(np.unique(P.sort_field(keys, 0, 45))) == len(keys) == len(vals)
    keys, _ = A.prim_input("sort_pairs")
    assert len(np.unique(P.sort_field(keys, 32, 47))) < len(keys)               # ties on the sorted bits: stability is observable
    idx, _ = A.prim_input("scatter")
    assert len(np.unique(idx)) == len(idx) and int(idx.max()) < 1 << 24
    cls, a, b = A.prim_input("select")
    assert 0.4 < float((cls == 1).mean()) < 0.6
    nxt = A.prim_input("orbit")
    i = np.arange(len(nxt))
    assert (nxt > i).all() and (nxt <= len(nxt)).all()
    mark = A.BY_NAME["prims-mark_orbit-%d" % A.PRIM_SIZES["orbit"]].want()[0]
    assert mark[0] == 1 and 1000 < int(mark.sum()) < len(nxt) and int(np.flatnonzero(mark)[-1]) > P.ORB_SUPER - 2000     # the chain reaches the second super-tile's border
    ex = A.prim_input("tile_entries")
    assert ((ex < ex.shape[1]) | (ex == P.DX_NONE)).all()
    entry = A.BY_NAME["prims-tile_entries-%d-%d" % A.PRIM_SIZES["tile_entries"]].want()[0]
    assert int((entry != P.DX_NONE).sum()) > 3 * P.DX_G                          # the chain crosses several groups
    assert len(np.unique(A.prim_input("sort_u64"))) <= 37
