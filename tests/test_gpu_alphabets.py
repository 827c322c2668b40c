"""GPU tests at the literal alphabets and code depths the English / DNA generators never reach (pytest -m gpu).

  * deep Huffman codes (tests/corpus.deep_code_text: chain-shaped literal counts): codes longer than the decoder's 12-bit lookup
    table take the canonical walk of dec_code and of the host parse, codes of more than 32 bits go through the packers' u64 code
    words; streams against the oracle's byte for byte in every encoder variant, the oracle's streams decoded by every parse;
  * an alphabet sweep at production size (sigma = 2 .. 256 counting the sentinel: every bits-per-symbol b of the wide sort's keys,
    one and two key words), the text index and the streams against the oracle's, and the level-1-behind-the-upload path on a
    200-symbol text;
  * the arithmetic coder with 0xFF literals (the all-ones word at literal_count - 1 lands mid-stream) and with models whose longest
    flush-free segment lies just below and just above ARITH_STEP_CAP (arith.hip: the sequential fall-back).

Every test first asserts that its input reaches the edge it is about (code depth from the stream header, alphabet size, key words,
device parse, segment lengths), so that none of them can pass vacuously."""
import functools

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.util import huff_header

pytestmark = pytest.mark.gpu

LUT_BITS = 12                     # decode.hip: codes up to this length are looked up, longer ones walked
ARITH_STEP_CAP = 4096             # arith.hip: a flush-free segment longer than this sends the coder to its sequential pass

CTX_OPTIONS = {
    "early0": {"enc_early": 0},                   # encoder after the factorization
    "early2": {"enc_early": 2},                   # early encoder at every size (pack_cls_kernel<REC> below 1 MiB too)
    "norec": {"enc_rec": 0},                      # pack_kernel: the pack without the records
    "dev_lean": {"dec_parse": 2, "dec_lean": 1},  # device parse of every stream, lean marking where the tokens are short
    "dev_general": {"dec_parse": 2, "dec_lean": 0},
    "host_parse": {"dec_parse": 0},
    "no_overlap": {"wsort_overlap": 0},
}


@pytest.fixture(scope="module")
def ctxs():
    cs = {k: T.Context(0, options=v) for k, v in CTX_OPTIONS.items()}
    yield cs
    for c in cs.values():
        c.close()


def _terminated(raw):
    return np.concatenate([raw, np.zeros(1, dtype=np.uint8)]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _deep_text(target, seg=(120, 230), slack=0.05):
    return _terminated(corpus.deep_code_text(target, seed=target, slack=slack, seg=seg)).tobytes()


def _oracle_factors(text, threshold, flatten):
    sa = O.suffix_array(text)
    isa, phi, plcp, maxlcp = O.isa_phi_plcp(text, sa)
    f = O.sort_factors(O.arrays_comp(sa, isa, O.lcp_array(sa, plcp), maxlcp, threshold))
    return O.flatten(f)[0] if flatten else f


def _la_bits(h):
    """decode.hip decode_lzss_huff_device: the longest token a candidate may read (the lean marking takes <= 1024 bits)"""
    code_max = h["longest"] if h["longest"] else 8
    return 1 + O.bits_for(h["fdist_max"]) + h["fdist_max"] * code_max + O.bits_for(h["n"]) + O.bits_for(h["flen_max"] - h["flen_min"])


def _check_deep(gpu_ctx, ctxs, text, thr, want_longest, encoders, decoders, default_parse):
    for fl in (0, 1):
        want, _ = O.lcpcomp_huff_compress(text, thr, fl)
        h = huff_header(want)
        assert h["longest"] >= want_longest >= LUT_BITS, (h["longest"], want_longest)
        assert h["fdist_max"] <= 512, h["fdist_max"]                      # the device parse takes the stream
        for label in encoders:
            got, st = (gpu_ctx if label == "default" else ctxs[label]).lcpcomp_compress(text, thr, fl)
            assert got == want, "%s flatten=%d: %d vs %d bytes" % (label, fl, len(got), len(want))
            assert st["fdist_max"] == h["fdist_max"] and st["flen_max"] == h["flen_max"], label
        for label in decoders:
            back, st = (gpu_ctx if label == "default" else ctxs[label]).lcpcomp_decompress(want)
            assert back == text, "%s flatten=%d" % (label, fl)
            want_dev = {"dev_lean": 1, "dev_general": 1, "host_parse": 0, "default": default_parse}[label]
            assert st["device_parse"] == want_dev, label
    # the stand-alone encoder on the oracle's factor list
    f = _oracle_factors(text, thr, 1)
    want, _ = O.encode_huff(text, f)
    assert huff_header(want)["longest"] >= want_longest
    assert gpu_ctx.encode_huff(text, f["pos"], f["src"], f["len"]) == want


@pytest.mark.parametrize("target", [12, 13, 16, 24])
def test_deep_codes_small(gpu_ctx, ctxs, target):
    """codes of exactly 12 bits (the last length the lookup table holds), 13 (the first the walk decodes), 16 and 24 bits"""
    text = _deep_text(target)
    assert len(text) <= 400_000
    want, _ = O.lcpcomp_huff_compress(text, 32, 1)
    assert huff_header(want)["longest"] == target
    _check_deep(gpu_ctx, ctxs, text, 32, target, ["default", "early0", "early2", "norec"],
                ["dev_lean", "dev_general", "host_parse", "default"], default_parse=0)


def test_deep_codes_through_the_lean_marking(ctxs):
    """short literal runs: the longest token stays within the lean marking's 1024 bits although its codes take the walk"""
    text = _deep_text(18, seg=(24, 40))
    for thr, fl in ((24, 1), (40, 0)):
        want, _ = O.lcpcomp_huff_compress(text, thr, fl)
        h = huff_header(want)
        assert h["longest"] > LUT_BITS and _la_bits(h) <= 1024, (h["longest"], _la_bits(h))
        for label in ("dev_lean", "dev_general", "host_parse"):
            back, st = ctxs[label].lcpcomp_decompress(want)
            assert back == text, (label, thr, fl)
        assert ctxs["early2"].lcpcomp_compress(text, thr, fl)[0] == want


def test_codes_longer_than_32_bits(gpu_ctx, ctxs):
    """~25 MB whose rarest literals get 33-bit codes: the code words of the packers (pack_cls_kernel<REC> at this size by default,
    pack_kernel without the records) are wider than 32 bits; the default decoder parses the stream on the device"""
    text = _deep_text(33, slack=0.03)
    assert 16_000_000 <= len(text) <= 40_000_000
    _check_deep(gpu_ctx, ctxs, text, 32, 33, ["default", "early0", "norec"], ["default", "dev_general", "host_parse"], default_parse=1)


# ---- alphabet sweep at production size ------------------------------------------------------------------------------------------
SIGMAS = [2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 200, 256]
SWEEP = [(s, d) for s in SIGMAS for d in ("uniform", "zipf") if not (s == 2 and d == "zipf")]


def _sweep_text(sigma, dist):
    i = SIGMAS.index(sigma)
    n = 1_100_000 + 7919 * i + (3 if dist == "zipf" else 0)
    escapes = sigma == 256 or (dist == "zipf" and sigma in (9, 65, 200))
    return O.escape(corpus.alphabet_text(n, sigma, dist, seed=100 + i, escapes=escapes).tobytes())


@pytest.mark.parametrize("sigma,dist", SWEEP, ids=["s%d_%s" % sd for sd in SWEEP])
def test_alphabet_sweep(gpu_ctx, sigma, dist):
    text = _sweep_text(sigma, dist)
    a = np.frombuffer(text, dtype=np.uint8)
    assert len(text) >= 1 << 20 and len(text) & (len(text) - 1)
    assert np.unique(a).size == sigma
    b = O.bits_for(sigma - 1)
    kw = 1 if b <= 4 else 2
    sa = O.suffix_array(text)
    isa, phi, plcp, maxlcp = O.isa_phi_plcp(text, sa)
    g = gpu_ctx.textds(text)
    for k, want in (("sa", sa), ("isa", isa), ("phi", phi), ("plcp", plcp)):
        bad = np.nonzero(g[k] != want)[0]
        assert bad.size == 0, "sigma %d %s: %s differs at %d slots, first %d" % (sigma, dist, k, bad.size, bad[0])
    assert g["maxlcp"] == maxlcp
    for thr in (2, 5):
        want, _ = O.lcpcomp_huff_compress(text, thr, 1)
        got, st = gpu_ctx.lcpcomp_compress(text, thr, 1)
        assert st["sa_key_words"] == kw, (sigma, b, st["sa_key_words"])
        assert got == want, "sigma %d %s thr %d: %d vs %d bytes" % (sigma, dist, thr, len(got), len(want))
        try:
            decodable = O.lcpcomp_huff_decompress(want) == text
        except RuntimeError:
            decodable = False
        if not decodable:             # 256 codes of 8 bits wrap the reference's u8 numl: it cannot decode its own stream either
            assert huff_header(want)["sigma"] == 256, (sigma, dist, thr)
            continue
        back, _ = gpu_ctx.lcpcomp_decompress(want)
        assert back == text, (sigma, dist, thr)


def test_sweep_reaches_every_key_geometry():
    bs = {O.bits_for(s - 1) for s in SIGMAS}
    assert bs == set(range(1, 9))
    assert {1 if b <= 4 else 2 for b in bs} == {1, 2}
    assert any((64 * (1 if b <= 4 else 2)) % b for b in bs) and any((64 * (1 if b <= 4 else 2)) % b == 0 for b in bs)   # pad != 0 and == 0


def test_level_one_behind_the_upload_on_a_wide_alphabet(gpu_ctx, ctxs):
    """a host-buffer text of 2^26 + 4321 bytes over 200 symbols: the first partition level runs behind the upload with the code map
    of chunk 0; the stream equals the one without the overlap, and the oracle decodes it"""
    n = (1 << 26) + 4321
    text = np.concatenate([corpus.alphabet_text(n - 1, 200, "zipf", seed=77), np.zeros(1, dtype=np.uint8)])
    assert np.unique(text).size == 200
    a, sa_ = gpu_ctx.lcpcomp_compress(text, 3, 1)
    b, sb_ = ctxs["no_overlap"].lcpcomp_compress(text, 3, 1)
    assert sa_["sa_overlapped"] == 1 and sb_["sa_overlapped"] == 0, (sa_["sa_overlapped"], sb_["sa_overlapped"])
    assert sa_["sa_key_words"] == 2
    assert a == b
    assert O.lcpcomp_huff_decompress(a) == text.tobytes()


# ---- arithmetic coder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,dist,thr", [(12, "zipf", 2), (12, "zipf", 5), (40, "uniform", 2)])
def test_arithmetic_with_ff_literals(gpu_ctx, sigma, dist, thr):
    """escaped texts of more than 1 MiB with many 0x00 / 0xFF: literal_count (the cumulative count up to byte 254, arith.hip) is
    smaller than the number of literals, so the all-ones word is written in the middle of the stream"""
    text = O.escape(corpus.alphabet_text(1_250_000 + sigma, sigma, dist, seed=sigma, escapes=True).tobytes())
    assert len(text) >= 1 << 20
    f = _oracle_factors(text, thr, 1)
    C = O.literal_histogram(text, f)
    nlit = len(text) - int(f["len"].astype(np.int64).sum())
    literal_count = int(C[:255].sum())
    assert C[255] >= 100 and 0 < literal_count <= nlit - 100, (int(C[255]), literal_count, nlit)
    want, _ = O.lcpcomp_arith_compress(text, thr, 1)
    got, _ = gpu_ctx.lcpcomp_compress(text, thr, 1, T.CODER_ARITH)
    assert got == want, "%d vs %d bytes" % (len(got), len(want))


def _arith_model(lits):
    """arith_build_model (ArithmeticCoder.hpp:72-92) in Python integers: the normalised cumulative counts, min_range, tot"""
    c = [int(x) for x in np.bincount(lits, minlength=256)]
    mn = min(x for x in c[1:] if x)
    for i in range(1, 256):
        c[i] += c[i - 1]
    c = [x // mn for x in c]
    return c, c[254], c[255]


def _segment_lengths(lits, C, min_range, tot, limit):
    """for every literal k: how many literals the coder takes, its interval reset at k, before the next flush (or the end) --
    arith_step's width update (it does not depend on `lower`) for all k at once, exact in u64: below tot the products
    range * C[v] stay under tot^2 < 2^64, above it (range / tot) * C[v] <= range"""
    n = len(lits)
    Cv = np.array(C, dtype=np.uint64)
    Cp = np.concatenate([np.zeros(1, dtype=np.uint64), Cv[:-1]])
    tot_, min_ = np.uint64(tot), np.uint64(min_range)
    width = np.full(n, np.iinfo(np.uint64).max, dtype=np.uint64)
    seg = np.zeros(n, dtype=np.int64)
    act = np.arange(n)
    t = 0
    while act.size and t < limit:
        v = lits[act + t]
        r = width[act]
        small = r <= tot_
        q = r // tot_
        hi = np.where(small, r * Cv[v] // tot_, q * Cv[v])
        lo = np.where(small, r * Cp[v] // tot_, q * Cp[v])
        width[act] = hi - lo
        t += 1
        seg[act] = t
        act = act[(act + t < n) & (width[act] >= min_)]
    return seg


@pytest.mark.parametrize("m,side", [(44, "below"), (43, "above"), (42, "above")])
def test_arithmetic_segments_around_the_step_cap(gpu_ctx, m, side):
    """literal-only texts (threshold above any LCP) of 'a' runs and 'b' clusters: the longest flush-free segment -- a run of 'a'
    from a reset -- lies just below or just above ARITH_STEP_CAP, so the coder takes the parallel segments or the sequential pass"""
    raw = (b"a" * 5000 + b"b" * m) * 3 + b"a" * 300
    text = O.escape(raw)
    lits = np.frombuffer(text, dtype=np.uint8)
    C, min_range, tot = _arith_model(lits)
    longest = int(_segment_lengths(lits, C, min_range, tot, ARITH_STEP_CAP + 512).max())
    overflow = longest - 1 > ARITH_STEP_CAP          # arith_next_flush_kernel: ++steps > ARITH_STEP_CAP
    if side == "below":
        assert ARITH_STEP_CAP - 64 <= longest and not overflow, longest
    else:
        assert overflow and longest <= ARITH_STEP_CAP + 256, longest
    thr = len(text)
    want, ost = O.lcpcomp_arith_compress(text, thr, 1)
    assert ost["factors"] == 0
    got, _ = gpu_ctx.lcpcomp_compress(text, thr, 1, T.CODER_ARITH)
    assert got == want, "%d vs %d bytes" % (len(got), len(want))
