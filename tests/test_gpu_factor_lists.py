"""GPU tests of flatten, the encoders and the decoder on hand-shaped factor lists (tests/factor_lists.py; pytest -m gpu).

The factorizers hand these stages lists of a few narrow shapes only.  Here the stand-alone entry points (tdc_gpu_flatten,
tdc_gpu_encode_*) and the decoder get staircases of factors that wait for one another (one flatten round each), chains of a million
steps, forward chains, equal lengths, extreme and forward sources, literal runs of exactly 512 / 513 around the switch to the device
parse and position chains of depth ~2^24.  Flatten must equal the oracle's sequential flatten under three round budgets, every
encoder must equal the oracle byte for byte, and every decoder path must give back the text that `resolve` says the list means."""
import functools

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import factor_lists as FL
from tests.util import factors_struct

pytestmark = pytest.mark.gpu

CASES = FL.cases("gpu")
IDS = [c[0] for c in CASES]

FLATTEN_OPTS = {
    "default": {},
    "steps1_growth2": {"flatten_steps": 1, "flatten_growth": 2},     # ~20 rounds in a row that finish nothing on million_steps
    "unlimited": {"flatten_steps": 0},
}
DECODE_OPTS = {
    "lean_seg4096": {"dec_parse": 2, "dec_lean": 1, "dec_seg": 4096},
    "general_seg4096": {"dec_parse": 2, "dec_lean": 0, "dec_seg": 4096},
}
OWNER_REM = (0, 1, 8)
PIPE_OPTS = {"rem%d" % r: {"enc_early": 2, "owner_rem": r} for r in OWNER_REM}


@pytest.fixture(scope="module")
def ctxs():
    out = {name: T.Context(0, options=o) for name, o in list(FLATTEN_OPTS.items()) + list(DECODE_OPTS.items()) + list(PIPE_OPTS.items())}
    yield out
    for c in out.values():
        c.close()


@functools.lru_cache(maxsize=None)
def _case(cid):
    _, shape, n, kw = CASES[IDS.index(cid)]
    text, pos, src, length = FL.make_case(shape, n, FL.case_seed(cid), **kw)
    f = factors_struct(pos, src, length)
    flat, nf, md = O.flatten(f)
    return text, pos, src, length, f, flat, nf, md


def _literals(text, pos, length):
    lit = np.frombuffer(text, dtype=np.uint8).copy()
    for p, l in zip(pos, length):
        lit[p:p + l] = 0
    return lit


@pytest.mark.parametrize("cid", IDS)
def test_flatten_matches_oracle(ctxs, cid):
    text, pos, src, length, f, flat, nf, md = _case(cid)
    n = len(text)
    lit = _literals(text, pos, length)
    for name in FLATTEN_OPTS:
        got, gnf, gmd = ctxs[name].flatten(n, pos, src, length)
        assert (got == flat["src"]).all(), "%s [%s]: %d sources differ" % (cid, name, int((got != flat["src"]).sum()))
        assert (gnf, gmd) == (nf, md), "%s [%s]: num_flattened / max_depth_lb" % (cid, name)
        assert FL.resolve(n, lit, pos, got, length) == text, "%s [%s]" % (cid, name)
    if cid == "million_steps":
        fin, dep = FL.million_steps_expected(pos, src, length)
        assert (flat["src"] == fin).all() and nf == len(pos) - 1 and md == dep.max() > FL.MILLION - 16
    if cid == "staircase":
        assert (flat["src"] == src[0]).all() and nf == len(pos) - 1 and md == 1


def _encoders(ctx):
    yield "huff", ctx.encode_huff, O.encode_huff
    yield "arith", ctx.encode_arith, O.encode_arith
    yield "ascii", ctx.encode_ascii, O.encode_ascii
    for k in (1, 3, 7):
        yield "sle%d" % k, functools.partial(ctx.encode_sle, kmer=k), functools.partial(lambda t, l, k: O.encode_sle(t, l, k), k=k)


@pytest.mark.parametrize("cid", IDS)
def test_encoders_match_oracle(ctxs, cid):
    text, pos, src, length, f, flat, nf, md = _case(cid)
    ctx = ctxs["default"]
    for which, lst in (("original", f), ("flattened", flat)):
        for name, dev, orc in _encoders(ctx):
            try:
                want, _ = orc(text, lst)
            except RuntimeError:
                assert name == "arith"                       # the reference divides by zero: the sentinel is the only literal
                with pytest.raises(T.TdcGpuError) as e:
                    dev(text, lst["pos"], lst["src"], lst["len"])
                assert e.value.status == -6
                continue
            got = dev(text, lst["pos"], lst["src"], lst["len"])
            assert got == want, "%s %s %s: %d vs %d bytes" % (cid, which, name, len(got), len(want))


@pytest.mark.parametrize("cid", IDS)
def test_decoder_gives_back_the_text(ctxs, cid):
    text, pos, src, length, f, flat, nf, md = _case(cid)
    stream, _ = O.encode_huff(text, f)
    back, st = ctxs["default"].lcpcomp_decompress(stream)
    assert back == text, "%s: default decode" % cid
    if cid in ("run_512", "run_513"):
        assert len(stream) >= (1 << 20)
        assert st["device_parse"] == (1 if cid == "run_512" else 0), cid
    if cid.startswith("deep_decode"):
        assert st["rounds"] <= 32, "%s: %d pointer-jumping rounds for a chain of depth %d" % (cid, st["rounds"], len(text) - 2)
    for name in DECODE_OPTS:
        back, st2 = ctxs[name].lcpcomp_decompress(stream)
        assert back == text, "%s [%s]" % (cid, name)
        if cid.startswith("deep_decode"):
            assert st2["rounds"] <= 32, (cid, name)
    stream, _ = O.encode_ascii(text, f)
    assert ctxs["default"].lcpcomp_decompress(stream, T.CODER_ASCII)[0] == text, "%s: ascii" % cid
    for k in (1, 3, 7):
        stream, _ = O.encode_sle(text, f, k)
        assert ctxs["default"].lcpcomp_decompress(stream, T.CODER_SLE | (k << 8))[0] == text, "%s: sle%d" % (cid, k)


# ---- the same shapes through the factorizer: the owner-word remainder path of flatten (flatten_round_kernel<*, true>) is only
# reached from the compressor when the early encoder plans it
def _pipeline_texts():
    rng = np.random.default_rng(77)
    out = []
    # random prefix + one long run + many short copies of run fragments and of the prefix
    pre = rng.integers(1, 255, 4096, dtype=np.uint8)
    run = np.full(300_000, 65, dtype=np.uint8)
    parts = [pre, run]
    for _ in range(3000):
        if rng.random() < 0.5:
            parts.append(np.full(int(rng.integers(3, 200)), 65, dtype=np.uint8))
        else:
            a = int(rng.integers(0, 4000))
            parts.append(pre[a:a + int(rng.integers(3, 90))])
        parts.append(rng.integers(1, 255, int(rng.integers(0, 3)), dtype=np.uint8))
    out.append(("run_and_copies", np.concatenate(parts).tobytes()))
    # a version chain: a random block, every copy edited at one place
    blk = rng.integers(1, 255, 20_000, dtype=np.uint8)
    parts = []
    for _ in range(60):
        blk = blk.copy()
        blk[int(rng.integers(0, len(blk)))] = rng.integers(1, 255)
        parts.append(blk)
    out.append(("version_chain", np.concatenate(parts).tobytes()))
    # a staircase in text form: the same block repeated, each copy one byte longer
    base = rng.integers(1, 255, 64, dtype=np.uint8)
    out.append(("growing_repeats", np.concatenate([np.concatenate([base, base[:k % 64]]) for k in range(2000)]).tobytes()))
    return out


PIPE = _pipeline_texts()


@pytest.mark.parametrize("name,data", PIPE, ids=[p[0] for p in PIPE])
def test_pipeline_owner_remainder_paths(ctxs, name, data):
    text = O.escape(data)
    for thr in (2, 5):
        want, _ = O.lcpcomp_huff_compress(text, thr, 1)
        for rem in OWNER_REM:
            got, _ = ctxs["rem%d" % rem].lcpcomp_compress(text, threshold=thr, flatten=1)
            assert got == want, "%s t=%d owner_rem=%d: %d vs %d bytes" % (name, thr, rem, len(got), len(want))
