"""The cases of tests/test_gpu_arena_state.py: one call (or a few) per entry-point family, and what the specification says it returns.

All device scratch comes from one bump allocator that never clears a byte (csrc/common.hpp Arena), so a call finds in its scratch
whatever the calls before it left there.  The GPU test runs every case here on an arena it has filled with 0x00, 0x01 and 0xFF
(tdc_gpu_prim_arena_fill) and after other cases; a kernel that reads an element its producer skipped is right under one of these and
wrong under another.  tests/test_arena_cases.py checks on the CPU that every want() computes and that every input reaches the fork
its name claims.

A case has
    name, family   -- `family` is what -k selects
    options        -- the options of its context
    run(ctx)       -- (tuple of bytes / numpy arrays / lists of them, dict of the call's deterministic stats)
    want()         -- the same tuple from the specification, cached; never calls the device
    check(stats)   -- optional: asserts that the call went the way the name claims (device-side counters)
    reserve        -- not 0: the context reserves an arena for a text of that many bytes first.  The lz78 / lzw decoder sizes its arena
                      from the stream and grows it in the middle of the call once it knows the phrase count; an arena that moved is fresh
                      memory, and the fill would not reach the call
The specification is what the GPU tests of each component already compare with: the oracle, the host loops of the C ABI, the models
under tests/models/ and numpy.  Their helpers are imported from those tests, not copied.

Nothing here needs a GPU to import."""
import functools
import os
import re

import numpy as np

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests import factor_lists as FL
from tests import lzss_sw_batches as B
from tests import prim_inputs as P
from tests.models import bwtzip as BZ
from tests.models import lzss_coders as LC
from tests.models import lzw as LZW
from tests.models import repair as RP
from tests.models import sle_literals as SLE
from tests.test_gpu_bwt import numpy_lf, want_bwt
from tests.test_gpu_bytestages import model as stage_model
from tests.test_gpu_levels import stale_levels_text
from tests.test_gpu_lzss_lcp_coders import _factors as lzss_lcp_factors
from tests.test_gpu_parity import _oracle_stages
from tests.test_gpu_prims import _scan_reference
from tests.test_gpu_repair import as_model, english as repair_english, host as repair_host, tie_text
from tests.util import factors_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
FILLS = (0x00, 0x01, 0xFF)          # what the suite sees today / "mark set", "class 1" / NONE32, "literal", "empty slot"
DEC_SEG = 4096                      # the smallest value option dec_seg takes
DEV = {"dec_parse": 2}              # every stream through the device parse; otherwise the default options

# stats that do not depend on the clock or on the order in which workgroups ran ("rounds" does: the pointer jumping of the inverse bwt
# runs in place, and how far a round gets depends on which words it finds already updated)
STAT_KEYS = ("n", "out_len", "factors", "maxlcp", "num_flattened", "max_depth_lb", "flen_min", "flen_max", "fdist_max", "sigma", "sa_mode",
             "sa_key_words", "window_pass", "small_levels", "eager_levels", "eager_phases", "rules", "replaced", "tie_rounds", "rebuilds", "heads", "launches", "phrases", "codes",
             "device_parse", "pipe_len", "pipe_dev")


def source_constant(path, pattern):
    """the integer a source file of the library defines: `pattern` has one group, an expression of digits, `<<` and casts"""
    src = open(os.path.join(ROOT, "tudocomp_amd", "csrc", path)).read()
    m = re.search(pattern, src)
    if not m:
        raise AssertionError("%s: /%s/ not found" % (path, pattern))
    expr = re.sub(r"\((?:size_t|u32|u64)\)|[ul]+\b", "", m.group(1).strip())
    if not re.fullmatch(r"[0-9<\s()*+-]+", expr):
        raise AssertionError("%s: %r is not a constant" % (path, m.group(1)))
    return int(eval(expr, {"__builtins__": {}}))


def _fail(msg):
    raise AssertionError(msg)


def det(stats):
    return {k: stats[k] for k in STAT_KEYS if k in stats}


class Case:
    def __init__(self, name, family, run, want, options=None, check=None, reserve=0):
        self.name, self.family, self.run, self.options, self.check, self.reserve = name, family, run, dict(options or {}), check, reserve
        self.want = functools.lru_cache(maxsize=None)(want)

    @property
    def default_options(self):
        return self.options in ({}, DEV)

    def __repr__(self):
        return "Case(%s)" % self.name


CASES = []


def add(name, family, run, want, options=None, check=None, reserve=0):
    CASES.append(Case(family + "-" + name, family, run, want, options, check, reserve))


def same(got, want):
    """exact equality of two result tuples (bytes, ints, numpy arrays, lists of those)"""
    if isinstance(want, (tuple, list)):
        return isinstance(got, (tuple, list)) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    if isinstance(want, np.ndarray) or isinstance(got, np.ndarray):
        return np.array_equal(np.asarray(got), np.asarray(want))
    return got == want


def describe(x):
    if isinstance(x, (tuple, list)):
        return "(" + ", ".join(describe(v) for v in x[:6]) + (", ..." if len(x) > 6 else "") + ")"
    if isinstance(x, np.ndarray):
        return "%s[%d]" % (x.dtype, x.size)
    if isinstance(x, (bytes, bytearray)):
        return "%d bytes" % len(x)
    return repr(x)


def first_difference(got, want):
    """where two result tuples part, for the failure message"""
    if isinstance(want, (tuple, list)) and isinstance(got, (tuple, list)):
        if len(got) != len(want):
            return "%d parts, want %d" % (len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            if not same(g, w):
                return "part %d: %s" % (i, first_difference(g, w))
        return "equal"
    if isinstance(want, (bytes, bytearray)) and isinstance(got, (bytes, bytearray)):
        g, w = np.frombuffer(bytes(got), dtype=np.uint8), np.frombuffer(bytes(want), dtype=np.uint8)
    elif isinstance(want, np.ndarray) and isinstance(got, np.ndarray):
        g, w = got.reshape(-1), want.reshape(-1)
    else:
        return "%s, want %s" % (describe(got), describe(want))
    m = min(len(g), len(w))
    d = np.flatnonzero(g[:m] != w[:m])
    at = int(d[0]) if len(d) else m
    return "%d vs %d elements, first difference at %d (%d differ in the common part)" % (len(g), len(w), at, len(d))


# ---- texts ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def text_of(kind):
    """escaped, 0-terminated texts of the lcpcomp cases"""
    if kind == "levels200k":        # tests/test_gpu_levels.py with K = 120, spread: repeats of 400 bytes (levels above the eager floor + 256),
        return O.escape(stale_levels_text(120, 120, True))       # 210 levels of up to 120 stale entries above the window cut
    if kind in ("english3M", "dna1M5"):     # the two texts of tests/test_gpu_bwt.py::test_every_suffix_array_path
        rng = np.random.default_rng(3)
        blk = bytes(rng.integers(0, 4, 40_000, dtype=np.uint8).astype(np.uint8) + 65)
        if kind == "english3M":
            return O.escape(T.gen_english(3_000_000, 17).tobytes())
        return O.escape(T.gen_dna(1_200_000, 5).tobytes() + blk + b"#" + blk[100:30_000] + T.gen_dna(300_000, 6).tobytes() + blk[5_000:])
    if kind.startswith("arith_m"):  # tests/test_gpu_alphabets.py::test_arithmetic_segments_around_the_step_cap
        return O.escape((b"a" * 5000 + b"b" * int(kind[7:])) * 3 + b"a" * 300)
    raise ValueError(kind)


# ---- lcpcomp compress -------------------------------------------------------------------------------------------------------------
LCP_CODERS = {"huff": (T.CODER_HUFF, "huff"), "arithmetic": (T.CODER_ARITH, "arith"), "ascii": (T.CODER_ASCII, "ascii"),
              "sle3": (T.CODER_SLE | (3 << 8), "sle")}
LCP_COMPS = {"arrays": T.COMP_ARRAYS, "max_lcp": T.COMP_MAXLCP, "plcppeaks": T.COMP_PLCPPEAKS, "heap": T.COMP_HEAP}
LCP_TEXTS = ("levels200k", "english3M", "dna1M5")
# what the wide suffix sort must report on the two large texts (test_every_suffix_array_path): separated by the sort alone / doubling
WIDE_MODE = {"english3M": 1, "dna1M5": 0}


def lcp_cell(ti, si, ci):
    """threshold and flatten of a cell, the pattern of tests/test_gpu_variants.py: a coder meets every threshold over the strategies"""
    return (1, 2, 5)[(ci + si + ti) % 3], (ci + ti) % 2


def _lcp_case(kind, coder, comp, thr, fl):
    dev_coder, orc_coder = LCP_CODERS[coder]

    def run(ctx):
        got, st = ctx.lcpcomp_compress(text_of(kind), thr, fl, dev_coder, LCP_COMPS[comp])
        return (got,), det(st)

    def want():
        return (O.lcpcomp_compress_any(text_of(kind), thr, fl, orc_coder, comp, kmer=3)[0],)

    def check(st):
        assert st["n"] == len(text_of(kind))
        if kind in WIDE_MODE:
            assert st["sa_key_words"] >= 1 and st["sa_mode"] == WIDE_MODE[kind], st
        else:
            assert st["sa_key_words"] == 0, st
            if comp == "arrays":    # the window pass, a run of levels inside one eager launch, and levels of the one-workgroup kernel
                assert st["window_pass"] == 1 and st["eager_phases"] >= 1 and st["eager_levels"] >= 1 and st["small_levels"] >= 1, st

    add("%s-%s-%s-t%d-f%d" % (kind, coder, comp, thr, fl), "lcpcomp", run, want, check=check)


# MaxHeapStrategy runs in ONE device thread, about 4.5 us per text byte: 13 s per call on the 3 MB text, 5 s on the smallest text
# the wide sort takes (2^20 bytes).  It meets the four coders on the 200 KB text; the wide sort's output is the other strategies' input too.
HEAP_TEXTS = ("levels200k",)

for _ti, _kind in enumerate(LCP_TEXTS):
    for _ci, _coder in enumerate(LCP_CODERS):
        for _si, _comp in enumerate(LCP_COMPS):
            if _comp == "heap" and _kind not in HEAP_TEXTS:
                continue
            _lcp_case(_kind, _coder, _comp, *lcp_cell(_ti, _si, _ci))


def _arith_case(m):
    kind = "arith_m%d" % m

    def run(ctx):
        text = text_of(kind)
        got, st = ctx.lcpcomp_compress(text, len(text), 1, T.CODER_ARITH)
        return (got,), det(st)

    def want():
        text = text_of(kind)
        return (O.lcpcomp_arith_compress(text, len(text), 1)[0],)

    add("step_cap-m%d" % m, "arith", run, want, check=lambda st: st["factors"] == 0 or _fail("factors in a literal-only text"))


for _m in (44, 43):
    _arith_case(_m)


# ---- stage entry points ------------------------------------------------------------------------------------------------------------
STAGE_THRESHOLD = 3
FACTOR_LIST = "random_mix-n262144-s4"          # one synthetic list of tests/factor_lists.py: forward, extreme and overlapping sources


@functools.lru_cache(maxsize=None)
def stage_reference(source):
    """(text, sorted factor list, flattened list, num_flattened, max_depth_lb) of the 200 KB text or of the synthetic list"""
    if source == "text":
        text = text_of("levels200k")
        sa, isa, phi, plcp, lcp, maxlcp = _oracle_stages(text)
        f = O.sort_factors(O.arrays_comp(sa, isa, lcp, maxlcp, STAGE_THRESHOLD))
    else:
        cid, shape, n, kw = next(c for c in FL.cases("gpu") if c[0] == FACTOR_LIST)
        text, pos, src, length = FL.make_case(shape, n, FL.case_seed(cid), **kw)
        f = factors_struct(pos, src, length)
    flat, nf, md = O.flatten(f)
    return text, f, flat, nf, md


def _stage_cases():
    text = lambda: text_of("levels200k")

    def run_sa(ctx):
        return tuple(ctx.suffix_array(text())), {}

    def want_sa():
        sa, isa = _oracle_stages(text())[:2]
        return sa, isa

    add("suffix_array-levels200k", "stages", run_sa, want_sa)

    def run_ds(ctx):
        g = ctx.textds(text())
        return (g["sa"], g["isa"], g["phi"], g["plcp"], g["lcp"], g["maxlcp"]), {}

    add("textds-levels200k", "stages", run_ds, lambda: tuple(_oracle_stages(text())))

    for fl in (0, 1):
        def run_f(ctx, fl=fl):
            pos, src, ln, st = ctx.factorize(text(), STAGE_THRESHOLD, flatten=fl)
            return (pos, src, ln), det(st)

        def want_f(fl=fl):
            _, f, flat, nf, md = stage_reference("text")
            return f["pos"], (flat if fl else f)["src"], f["len"]

        add("factorize-levels200k-f%d" % fl, "stages", run_f, want_f)

    for source in ("text", "list"):
        tag = "levels200k" if source == "text" else FACTOR_LIST

        def run_fl(ctx, source=source):
            t, f, flat, nf, md = stage_reference(source)
            src, gnf, gmd = ctx.flatten(len(t), f["pos"], f["src"], f["len"])
            return (src, gnf, gmd), {}

        def want_fl(source=source):
            t, f, flat, nf, md = stage_reference(source)
            return flat["src"], nf, md

        add("flatten-" + tag, "stages", run_fl, want_fl)
        encoders = (("huff", lambda c: c.encode_huff, O.encode_huff), ("arith", lambda c: c.encode_arith, O.encode_arith),
                    ("ascii", lambda c: c.encode_ascii, O.encode_ascii),
                    ("sle", lambda c: functools.partial(c.encode_sle, kmer=3), lambda t, f: O.encode_sle(t, f, 3)))
        for which in ("sorted", "flattened"):
            for name, dev, orc in encoders:
                def run_e(ctx, source=source, which=which, dev=dev):
                    t, f, flat, nf, md = stage_reference(source)
                    lst = f if which == "sorted" else flat
                    return (dev(ctx)(t, lst["pos"], lst["src"], lst["len"]),), {}

                def want_e(source=source, which=which, orc=orc):
                    t, f, flat, nf, md = stage_reference(source)
                    return (orc(t, f if which == "sorted" else flat)[0],)

                add("encode_%s-%s-%s" % (name, tag, which), "stages", run_e, want_e)


_stage_cases()


# ---- lcpcomp / lzss_lcp decompress on the device ------------------------------------------------------------------------------------
DEC_THRESHOLD = 3


@functools.lru_cache(maxsize=None)
def dec_stream(algo, coder):
    """the oracle's stream of the 200 KB text: lcpcomp(huff | sle, flatten = 0: chains stay deep) or lzss_lcp(bit | gamma | delta)"""
    text = text_of("levels200k")
    if algo == "lcpcomp":
        return O.lcpcomp_compress_any(text, DEC_THRESHOLD, 0, coder, "arrays", kmer=3)[0]
    return LC.encode_fast(text, lzss_lcp_factors(text, DEC_THRESHOLD), coder)


def _dec_cases():
    ids = {"huff": T.CODER_HUFF, "sle": T.CODER_SLE | (3 << 8), "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
    for lean in (0, 1):
        opts = {"dec_parse": 2, "dec_lean": lean, "dec_seg": DEC_SEG}
        for algo, coders in (("lcpcomp", ("huff", "sle")), ("lzss_lcp", ("bit", "gamma", "delta"))):
            for coder in coders:
                def run(ctx, algo=algo, coder=coder):
                    fn = ctx.lcpcomp_decompress if algo == "lcpcomp" else ctx.lzss_lcp_decompress
                    back, st = fn(dec_stream(algo, coder), ids[coder])
                    return (back,), det(st)

                add("%s-%s-lean%d" % (algo, coder, lean), "lcpdec", run, lambda: (text_of("levels200k"),), opts,
                    check=lambda st: st["device_parse"] == 1 or _fail("host parse"))


_dec_cases()


# ---- lz78(gamma), lzw(bit, gamma) ---------------------------------------------------------------------------------------------------
LZ_INPUTS = ("longest_run70000",)


@functools.lru_cache(maxsize=None)
def lz_input(name):
    """the small corpus' longest text, then a run of 70 000: streams of several segments whose last phrases are hundreds of bytes long"""
    assert name in LZ_INPUTS
    return max((d for _, d in corpus.small_corpus()), key=len) + b"a" * 70_000


def _lz_cases():
    seg = {"dec_parse": 2, "dec_seg": DEC_SEG}
    for name in LZ_INPUTS:
        def run_c(ctx, name=name):
            got, st = ctx.lz78_compress(lz_input(name))
            return (got,), det(st)

        add("lz78-compress-" + name, "lz78", run_c, lambda name=name: (O.lz78_gamma_compress(lz_input(name)),))

        def run_d(ctx, name=name):
            back, st = ctx.lz78_decompress(O.lz78_gamma_compress(lz_input(name)))
            return (back,), det(st)

        add("lz78-decompress-" + name, "lz78", run_d, lambda name=name: (lz_input(name),), seg, reserve=1)
        for coder, cid in (("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA)):
            def run_wc(ctx, name=name, cid=cid):
                got, st = ctx.lzw_compress(lz_input(name), cid)
                return (got,), det(st)

            add("lzw-compress-%s-%s" % (coder, name), "lzw", run_wc, lambda name=name, coder=coder: (lzw_stream(name, coder),))

            def run_wd(ctx, name=name, coder=coder, cid=cid):
                back, st = ctx.lzw_decompress(lzw_stream(name, coder), cid)
                return (back,), det(st)

            add("lzw-decompress-%s-%s" % (coder, name), "lzw", run_wd, lambda name=name: (lz_input(name),), seg,
                check=lambda st: st["device_parse"] == 1 or _fail("host parse"), reserve=1)


@functools.lru_cache(maxsize=None)
def lzw_stream(name, coder):
    return LZW.compress(lz_input(name), coder)


_lz_cases()


# ---- bwt ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bwt_text(name):
    """the first three texts of tests/test_gpu_bwt.py::test_inverse_stage_parameters"""
    if name == "english200k":
        return T.escape(T.gen_english(200_000, 3).tobytes() + b"\x00\xff" * 300)
    if name == "run70000":
        return b"a" * 70_000 + b"\0"
    return T.escape(corpus.fib_word(22))


@functools.lru_cache(maxsize=None)
def bwt_of(name):
    return want_bwt(bwt_text(name))


def _bwt_cases():
    for name in ("english200k", "run70000", "fib22"):
        def run_f(ctx, name=name):
            got, st = ctx.bwt_compress(bwt_text(name))
            return (got,), det(st)

        add("forward-" + name, "bwt", run_f, lambda name=name: (bwt_of(name),))

        def run_b(ctx, name=name):
            back, st = ctx.bwt_decompress(bwt_of(name))
            return (back,), det(st)

        add("decompress-" + name, "bwt", run_b, lambda name=name: (bwt_text(name),))
        for sample, steps in ((64, 5), (4096, 0)):
            def run_i(ctx, name=name, sample=sample, steps=steps):
                out, st = ctx.bwt_inverse_stage(bwt_of(name), sample, steps)
                return (out, st["lf"]), det(st)

            add("inverse-%s-s%d-m%d" % (name, sample, steps), "bwt", run_i, lambda name=name: (bwt_text(name), numpy_lf(bwt_of(name))))


_bwt_cases()


# ---- rle, mtf, encode(huff) and the chains, both directions on the device -------------------------------------------------------------
MTF_GROUP = 1 << 18                 # csrc/bytestages.hpp: bytes per workgroup of mtf
HUFF, MTF, RLE0 = T.STAGE_HUFF, T.STAGE_MTF, (T.STAGE_RLE, 0)
CHAINS = {"rle": [RLE0], "mtf": [MTF], "huff": [HUFF], "bwtzip": [T.STAGE_BWT, RLE0, MTF, HUFF], "bwtzip_sle": [T.STAGE_BWT, RLE0, MTF, (T.STAGE_SLE, 3)]}


@functools.lru_cache(maxsize=None)
def pipe_inputs():
    """{name: bytes}: the twelve inputs of tests/test_gpu_bytestages.py::test_tile_borders_of_mtf (same generator, same order) and one
    input over a single letter"""
    rng = np.random.default_rng(12)
    out = {}
    for k in (1, 2):
        for d in (-1, 0, 1):
            n = MTF_GROUP * k + d
            out["random-%d" % n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            out["mod251-%d" % n] = (np.arange(n) % 251).astype(np.uint8).tobytes()
    out["sigma1-100000"] = b"z" * 100_000
    return out


PIPE_NAMES = tuple("%s-%d" % (g, MTF_GROUP * k + d) for k in (1, 2) for d in (-1, 0, 1) for g in ("random", "mod251")) + ("sigma1-100000",)
# the chains start with the bwt of the escaped input, whose length is not the input's: the borders are the single stages' business
CHAIN_NAMES = ("random-%d" % (MTF_GROUP + 1), "mod251-%d" % (2 * MTF_GROUP - 1), "sigma1-100000")


@functools.lru_cache(maxsize=None)
def pipe_stage_outputs(chain, name):
    """(what the pipeline takes, [output of every stage])"""
    data = pipe_inputs()[name]
    stages = CHAINS[chain]
    if stages[0] == T.STAGE_BWT:
        data = T.escape(data)
    outs, cur = [], data
    for s in stages:
        if s == T.STAGE_BWT:
            cur = want_bwt(cur)
        elif isinstance(s, tuple) and s[0] == T.STAGE_SLE:
            cur = SLE.encode(cur, s[1])
        elif s == MTF and outs and chain.startswith("bwtzip"):
            cur = _mtf_of_bwtzip(name)
        else:
            cur = stage_model(s, cur)
        outs.append(cur)
    return data, outs


@functools.lru_cache(maxsize=None)
def _mtf_of_bwtzip(name):
    """the two chains share bwt:rle:mtf"""
    return BZ.mtf_encode(BZ.rle_encode_np(want_bwt(T.escape(pipe_inputs()[name])), 0))


def _pipe_cases():
    for chain, stages in CHAINS.items():
        for name in (CHAIN_NAMES if chain.startswith("bwtzip") else PIPE_NAMES):
            def run_c(ctx, chain=chain, stages=stages, name=name):
                got, st = ctx.pipeline_compress(stages, _pipe_source(chain, name))
                return (got,), det(st)

            def want_c(chain=chain, name=name):
                return (pipe_stage_outputs(chain, name)[1][-1],)

            add("%s-compress-%s" % (chain, name), "pipeline", run_c, want_c, DEV)

            def run_d(ctx, chain=chain, stages=stages, name=name):
                data, outs = pipe_stage_outputs(chain, name)
                buf = np.empty(max(len(data), 1), dtype=np.uint8)
                try:
                    n, st = ctx.pipeline_decompress_stats(stages, outs[-1], buf)
                except T.TdcGpuError as e:
                    return (e.status,), {}
                return (buf[:n].tobytes(),), det(st)

            def want_d(chain=chain, name=name):
                if chain == "huff":         # all 256 byte values at one code length: no decoder reads that header,
                    try:                    # and the device must refuse it as the host loop does
                        return (T.huff_decode_literals(pipe_stage_outputs(chain, name)[1][-1]),)
                    except T.TdcGpuError as e:
                        return (e.status,)
                return (_pipe_source(chain, name),)

            every = (1 << len(stages)) - 1
            add("%s-decompress-%s" % (chain, name), "pipeline", run_d, want_d, DEV,
                check=lambda st, every=every: st.get("pipe_dev", every) == every or _fail("a stage went through its host loop: pipe_dev %s" % bin(st["pipe_dev"])))


def _pipe_source(chain, name):
    data = pipe_inputs()[name]
    return T.escape(data) if CHAINS[chain][0] == T.STAGE_BWT else data


_pipe_cases()


# ---- lzss ---------------------------------------------------------------------------------------------------------------------------
LZSS_INPUT = ("one",)               # B.batch("one") = [material(3 * 4096 + 17, 8)]
LZSS_DEC = ((16, 3), (4096, 0))     # (window, threshold) of the streams the device decodes


def _lzss_cases():
    data = lambda: B.batch("one")[0]
    for coder in ("ascii", "bit", "gamma", "delta"):
        for w in (16, 4096):
            for t in (0, 3):
                def run(ctx, coder=coder, w=w, t=t):
                    got, st = ctx.lzss_sw_compress(data(), w, t, B.CODER_ID[coder])
                    return (got,), det(st)

                def want(coder=coder, w=w, t=t):
                    status, streams = B.expected((data(),), w, t, coder)
                    assert status == [0]
                    return (streams[0],)

                add("compress-%s-w%d-t%d" % (coder, w, t), "lzss", run, want)
    seg = {"dec_parse": 2, "dec_seg": DEC_SEG}
    for coder in ("bit", "gamma", "delta"):
        for w, t in LZSS_DEC:
            def run_d(ctx, coder=coder, w=w, t=t):
                back, st = ctx.lzss_sw_decompress(B.expected((data(),), w, t, coder)[1][0], w, B.CODER_ID[coder])
                return (back,), det(st)

            add("decompress-%s-w%d-t%d" % (coder, w, t), "lzss", run_d, lambda: (data(),), seg,
                check=lambda st: st["device_parse"] == 1 or _fail("host parse"))
    for bname in ("tile_edges", "empties", "widths"):
        for coder in ("ascii", "bit", "gamma", "delta"):
            def run_b(ctx, bname=bname, coder=coder):
                streams, status, st = ctx.lzss_sw_compress_batch(B.batch(bname), 16, 3, B.CODER_ID[coder])
                return (streams, status), det(st)

            def want_b(bname=bname, coder=coder):
                status, streams = B.expected(tuple(B.batch(bname)), 16, 3, coder)
                return streams, status

            add("batch-compress-%s-%s" % (bname, coder), "lzss_batch", run_b, want_b)
            if coder == "ascii":
                continue

            def run_bd(ctx, bname=bname, coder=coder):
                texts, status, st = ctx.lzss_sw_decompress_batch(B.expected(tuple(B.batch(bname)), 16, 3, coder)[1], B.CODER_ID[coder], 16)
                return (texts, status), det(st)

            def want_bd(bname=bname):
                texts = list(B.batch(bname))
                return texts, [0] * len(texts)

            add("batch-decompress-%s-%s" % (bname, coder), "lzss_batch", run_bd, want_bd)


_lzss_cases()


# ---- repair -------------------------------------------------------------------------------------------------------------------------
REPAIR_OPTIONS = {"default": {}, "recount": {"repair_recount": 1}, "table8": {"repair_table_bits": 8}}


@functools.lru_cache(maxsize=None)
def repair_text(name):
    return {"ties": tie_text, "ab4097a": lambda: b"ab" * 4097 + b"a", "english64k": lambda: repair_english(64 << 10)}[name]()


@functools.lru_cache(maxsize=None)
def repair_stream(name, coder):
    return RP.encode(*as_model(*repair_host(repair_text(name))), coder)


def _repair_cases():
    for name in ("ties", "ab4097a", "english64k"):
        for oname, opts in REPAIR_OPTIONS.items():
            check = None
            if oname == "table8" and name == "english64k":
                check = lambda st: st["rebuilds"] > 0 or _fail("the table was never rebuilt")
            if name == "ties":
                check = lambda st: st["tie_rounds"] > 0 or _fail("no tie round")

            def run_g(ctx, name=name):
                r, s, st = ctx.repair_grammar(repair_text(name))
                return (r, s), det(st)

            add("grammar-%s-%s" % (name, oname), "repair", run_g, lambda name=name: tuple(repair_host(repair_text(name))), opts, check)
            for coder, cid in (("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA)):
                def run_c(ctx, name=name, cid=cid):
                    got, st = ctx.repair_compress(repair_text(name), 0, cid)
                    return (got,), det(st)

                add("compress-%s-%s-%s" % (coder, name, oname), "repair", run_c, lambda name=name, coder=coder: (repair_stream(name, coder),), opts, check)
        for coder, cid in (("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA)):
            def run_d(ctx, name=name, coder=coder, cid=cid):
                back, st = ctx.repair_decompress_stats(repair_stream(name, coder), cid)
                return (back,), det(st)

            add("decompress-%s-%s" % (coder, name), "repair", run_d, lambda name=name: (repair_text(name),), DEV,
                check=lambda st: st["device_parse"] == 1 or _fail("host loop"))


_repair_cases()


# ---- the shared primitives, one input each at a size where the code forks ------------------------------------------
S = P.STILE
PRIM_SIZES = {
    "scan": 2 * S + 1,                       # two scan levels, a ragged last tile
    "scan3": S * S + 1,                      # three levels
    "sort_pairs": 64 * P.RS_TILE + 1,        # the XCD walk has started, a partial last tile
    "distinct_mid": P.MID_SORT_MAX - 1,      # the one-workgroup radix sort
    "distinct_big": P.MID_SORT_MAX + 1,      # the device-wide sort
    "scatter": P.SCATTER_MIN + 1,            # the MSD partition
    "select": 4096 * P.SEL_TILE + 9,         # the tile counts take the two-level scan
    "orbit": P.ORB_SUPER + 1,                # a second super-tile
    "tile_entries": (P.DX_G * P.DX_G + 1, 13),   # three levels of groups at sle's widest table
    "sort_u64": MiB + 123,                   # tests/test_gpu_sort.py: two partition levels of the splitter sort
}


@functools.lru_cache(maxsize=None)
def prim_input(name):
    rng = np.random.default_rng(sum(name.encode()))
    n = PRIM_SIZES[name]
    if name in ("scan", "scan3"):
        return rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    if name == "sort_pairs":
        return dict(P.sort_key_cases(n, rng, 64, {"heavy_keys"}))["heavy_keys"], rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    if name.startswith("distinct"):
        return P.distinct_on_bits_keys(n, rng, 0, 45), rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    if name == "scatter":
        return P.distinct_indices(n, 1 << 24, rng), rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    if name == "select":
        return P.select_classes(n, 1, "half", rng), rng.integers(0, 1 << 32, size=n, dtype=np.uint32), rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    if name == "orbit":
        return P.orbit_next(n, "geometric", rng)
    if name == "tile_entries":
        return P.tile_exits(n[0], n[1], "random", rng)
    if name == "sort_u64":
        return dict(P.sort_key_cases(n, rng, 64, {"37_values"}))["37_values"]
    raise ValueError(name)


FILL_A, FILL_B = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A


def _prim_cases():
    for name, op in (("scan", "sum_u32"), ("scan", "max_u32"), ("scan3", "sum_u32")):
        for in_place in (False, True):
            def run(ctx, name=name, op=op, in_place=in_place):
                return tuple(ctx.prim_scan(op, prim_input(name), in_place=in_place, want_total=op != "max_u32")), {}

            add("scan-%s-%d-%s" % (op, PRIM_SIZES[name], "in_place" if in_place else "two_buffers"), "prims", run,
                lambda name=name, op=op: tuple(_scan_reference(op, prim_input(name))))

    def run_sort(ctx):
        keys, vals = prim_input("sort_pairs")
        return tuple(ctx.prim_sort_pairs("u64", keys, vals, 32, 47)), {}

    def want_sort():
        keys, vals = prim_input("sort_pairs")
        order = P.stable_order(keys, 32, 47)
        return keys[order], vals[order]

    add("sort_pairs-u64-%d-bits32_47" % PRIM_SIZES["sort_pairs"], "prims", run_sort, want_sort)
    for name in ("distinct_mid", "distinct_big"):
        def run_d(ctx, name=name):
            keys, vals = prim_input(name)
            return tuple(ctx.prim_sort_pairs("distinct", keys, vals, 0, 45)), {}

        def want_d(name=name):
            keys, vals = prim_input(name)
            order = np.argsort(P.sort_field(keys, 0, 45), kind="stable")
            return keys[order], vals[order]

        add("sort_distinct-%d" % PRIM_SIZES[name], "prims", run_d, want_d)

    def run_sc(ctx):
        idx, val = prim_input("scatter")
        return (ctx.prim_bucketed_scatter(idx, val, 1 << 24, fill=FILL_A),), {}

    def want_sc():
        idx, val = prim_input("scatter")
        dst = np.full(1 << 24, FILL_A, dtype=np.uint32)
        dst[idx] = val
        return (dst,)

    add("bucketed_scatter-%d-into-2^24" % PRIM_SIZES["scatter"], "prims", run_sc, want_sc)

    def run_msd(ctx):
        idx, val = prim_input("scatter")
        oi, ov = ctx.prim_msd_partition(idx, val, 24, 8)
        # the order inside a group is the primitive's own: the groups in order, and the multiset of pairs
        return ((oi >> np.uint32(8)).astype(np.uint32), np.sort((oi.astype(np.uint64) << np.uint64(32)) | ov)), {}

    def want_msd():
        idx, val = prim_input("scatter")
        return np.sort(idx >> np.uint32(8)).astype(np.uint32), np.sort((idx.astype(np.uint64) << np.uint64(32)) | val)

    add("msd_partition-%d-bits24" % PRIM_SIZES["scatter"], "prims", run_msd, want_msd)

    def run_sel(ctx):
        cls, a, b = prim_input("select")
        oa, ob, cnt = ctx.prim_select(cls, 1, a, b, FILL_A, FILL_B)
        return (oa, ob, cnt), {}

    def want_sel():
        cls, a, b = prim_input("select")
        sel = np.flatnonzero(cls == 1)
        oa, ob = np.full(len(cls), FILL_A, dtype=np.uint32), np.full(len(cls), FILL_B, dtype=np.uint64)
        oa[:len(sel)], ob[:len(sel)] = a[sel], b[sel]
        return oa, ob, len(sel)

    add("select-%d" % PRIM_SIZES["select"], "prims", run_sel, want_sel)

    def run_selc(ctx):
        cls, a, b = prim_input("select")
        return tuple(ctx.prim_select_counts(cls, 1, _tile_counts(cls), a, FILL_A)), {}

    def want_selc():
        return want_sel()[::2]

    add("select_counts-%d" % PRIM_SIZES["select"], "prims", run_selc, want_selc)
    add("mark_orbit-%d" % PRIM_SIZES["orbit"], "prims", lambda ctx: ((ctx.prim_mark_orbit(prim_input("orbit")),), {}),
        lambda: (P.orbit_reference(prim_input("orbit")),))
    add("tile_entries-%d-%d" % PRIM_SIZES["tile_entries"], "prims", lambda ctx: ((ctx.prim_tile_entries(prim_input("tile_entries")),), {}),
        lambda: (P.tile_entries_reference(prim_input("tile_entries")),))
    for algo in (0, 1):
        def run_u(ctx, algo=algo):
            keys = prim_input("sort_u64")
            k, v = ctx.sort_pairs_u64(keys, np.arange(len(keys), dtype=np.uint32), algo)
            # the splitter sort is not stable: the keys in order, every value with its key, the values a permutation
            return (k, keys[v], np.sort(v)) if algo else (k, v), {}

        def want_u(algo=algo):
            keys = prim_input("sort_u64")
            if algo:
                return np.sort(keys), np.sort(keys), np.arange(len(keys), dtype=np.uint32)
            order = np.argsort(keys, kind="stable")
            return keys[order], order.astype(np.uint32)

        add("sort_pairs_u64-%d-algo%d" % (PRIM_SIZES["sort_u64"], algo), "prims", run_u, want_u)


def _tile_counts(cls):
    pad = np.zeros(-len(cls) % P.SEL_TILE, dtype=np.uint8)
    return (np.concatenate([cls, pad]).reshape(-1, P.SEL_TILE) == 1).sum(axis=1).astype(np.uint32)


_prim_cases()


# ---- blocks -------------------------------------------------------------------------------------------------------------------------
BLOCK = MiB + 777


@functools.lru_cache(maxsize=None)
def blocks_data():
    return T.gen_english(3 * MiB - 5000, 21).tobytes() + b"\x00\xff" * 2500


def _blocks_case():
    from tudocomp_amd import blocks as BL

    def run(ctx):
        """tdc_gpu_blocks_compress opens its workers' contexts itself: the second and third block of a worker find the leftovers of
        the block before them (what the shuffled test arranges by hand), and no fill reaches them.  What runs on `ctx`, and so on the
        filled arena, is the inverse: the container's blocks decoded one after another."""
        blob, st = T.blocks_compress(blocks_data(), BLOCK, threshold=2, flatten=1, devices=[0])
        parts = BL.unpack_container(blob)
        back = ctx.blocks_decompress(blob)
        return ([int(r) for r, _ in parts], [bytes(p) for _, p in parts], back), {"out_len": [s["out_len"] for s in st], "n": [s["n"] for s in st]}

    def want():
        data = blocks_data()
        parts = [data[o:o + BLOCK] for o in range(0, len(data), BLOCK)]
        return [len(p) for p in parts], [O.lcpcomp_huff_compress(O.escape(p), 2, 1)[0] for p in parts], data

    add("3MiB-in-blocks-of-MiB+777", "blocks", run, want)


_blocks_case()

FAMILIES = tuple(dict.fromkeys(c.family for c in CASES))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
