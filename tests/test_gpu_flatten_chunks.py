"""GPU tests of the flatten stage run in rank ranges (option flatten_chunks) and of the pack and download that follow the ranges
(pytest -m gpu).

Stage level: tdc_gpu_flatten with 2, 3 and 16 forced ranges -- and with 3 under the smallest round budget -- must give the oracle's
sequential flatten on the hand-shaped lists whose waits and sources cross the range borders.  Pipeline: on texts of the smallest length
at which a host-buffer call overlaps pack and download, the stream must be the oracle's byte for byte with 1, 2, 5 and 16 ranges, from
the caller's pinned buffer, the malloc sink and the keep-on-device entry -- among them texts whose tile bounds coincide (empty pack
ranges) and one whose longest factor spans several ranges."""
import functools

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import factor_lists as FL
from tests import flatten_chunk_texts as X
from tests.util import factors_struct

pytestmark = pytest.mark.gpu

STAGE_OPTS = {
    "k2": {"flatten_chunks": 2},
    "k3": {"flatten_chunks": 3},
    "k16": {"flatten_chunks": 16},
    "k3_steps1_growth2": {"flatten_chunks": 3, "flatten_steps": 1, "flatten_growth": 2},
}
PIPE_K = (1, 2, 5, 16)
STAGE_IDS = ["no_factors-n513", "one_literal-n3", "staircase", "forward_chain", "million_steps", "overlap_runs", "extreme_sources-n300000",
             "equal_lengths-L4097", "random_mix-n262144-s4"]
CASES = {c[0]: c for c in FL.cases("gpu")}


@pytest.fixture(scope="module")
def ctxs():
    out = {name: T.Context(0, options=o) for name, o in STAGE_OPTS.items()}
    out.update({"pipe%d" % k: T.Context(0, options={"flatten_chunks": k}) for k in PIPE_K})
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def pinned():
    bufs = T.PinnedBuffer(X.N), T.PinnedBuffer(2 * X.N)          # (text, stream: a half of random bytes does not shrink)
    yield bufs
    for b in bufs:
        b.free()


def test_the_option_is_settable_but_not_enumerated():
    assert "flatten_chunks" not in T.option_names()
    with T.Context(0) as c:
        c.set_option("flatten_chunks", 4)
        c.set_option("TDC_GPU_FLATTEN_CHUNKS", 0)


@pytest.mark.parametrize("cid", STAGE_IDS)
def test_flatten_in_ranges_matches_oracle(ctxs, cid):
    _, shape, n, kw = CASES[cid]
    text, pos, src, length = FL.make_case(shape, n, FL.case_seed(cid), **kw)
    flat, nf, md = O.flatten(factors_struct(pos, src, length))
    for name in STAGE_OPTS:
        got, gnf, gmd = ctxs[name].flatten(len(text), pos, src, length)
        assert (got == flat["src"]).all(), "%s [%s]: %d sources differ" % (cid, name, int((got != flat["src"]).sum()))
        assert (gnf, gmd) == (nf, md), "%s [%s]: num_flattened / max_depth_lb" % (cid, name)


@functools.lru_cache(maxsize=None)
def _text(name):
    text = O.escape(X.TEXTS[name]().tobytes())
    assert len(text) == X.N
    want, st = O.lcpcomp_huff_compress(text, 2, 1)
    return text, want, st


@pytest.mark.parametrize("name", list(X.TEXTS))
def test_pipeline_streams_equal_the_oracle(ctxs, pinned, name):
    text, want, wst = _text(name)
    h_in, h_out = pinned
    h_in.a[:] = np.frombuffer(text, dtype=np.uint8)
    for k in PIPE_K:
        ctx = ctxs["pipe%d" % k]
        h_out.a[:len(want) + 16] = 0xAA
        ln, st = ctx.lcpcomp_compress_into(h_in, X.N, h_out, threshold=2, flatten=1)
        assert ln == len(want) and h_out.a[:ln].tobytes() == want, "%s K=%d (pinned into): %d vs %d bytes" % (name, k, ln, len(want))
        assert (st["num_flattened"], st["max_depth_lb"]) == (wst["num_flattened"], wst["max_depth_lb"]), (name, k)
        print("%s K=%d: ranges_early %d, d2h_early %d of %d" % (name, k, st["ranges_early"], st["d2h_early"], ln))
        if name == "english" and k >= 2:
            assert 0 < st["d2h_early"] < ln, "%s K=%d: no part of the stream left before the pack was over" % (name, k)
        assert st["ranges_early"] <= max(k - 1, 0), (name, k)          # (the last range is always packed behind the stage)
        if name == "english" and k == 16:
            # the pack really started inside the flatten stage: with 16 ranges of a few rounds each, step B's words (a histogram, the
            # code table, one pass over 2 MiB and two scans behind the second round) are there long before the last range is done
            assert st["ranges_early"] >= 1, "%s K=%d: every range was left to the end of the flatten stage" % (name, k)
        got, _ = ctx.lcpcomp_compress(text, threshold=2, flatten=1)
        assert got == want, "%s K=%d (malloc sink)" % (name, k)
        ln, _ = ctx.lcpcomp_compress_keep(h_in, X.N, threshold=2, flatten=1)
        h_out.a[:len(want) + 16] = 0x55
        assert ctx.stream_fetch(h_out) == ln == len(want) and h_out.a[:ln].tobytes() == want, "%s K=%d (keep)" % (name, k)
