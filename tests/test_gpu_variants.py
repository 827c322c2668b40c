"""GPU tests of the lcpcomp paths off the default pair (pytest -m gpu): every strategy x coder pair and every host entry point at the
sizes where the large-text code runs, each stream against the oracle's (oracle.lcpcomp_compress_any) byte for byte.

  * a strategy x coder matrix at 3 MiB + 4321 bytes: the wide suffix sort, with its fused ISA / Phi / PLCP scatter on English (sa_mode 1)
    and the classic Phi behind doubling rounds on DNA (sa_mode 0), three super-tiles of orbit marking, more than 1024 encoder tiles;
    MaxHeapStrategy once on the wide path;
  * factors longer than a super-tile of orbit marking / ANSV (prim.hip mark_orbit_u32, lzss_lcp.hip), off and on a super-tile boundary;
  * the max_lcp level loop on structured multi-MB texts: G=64 kernels, pushes into more than SEG_INLINE target levels, skip-ahead probes;
  * lzss_lcp and one cell per non-default strategy and coder at 16 MiB;
  * compress_into (chunked pack with the early download), compress_keep + stream_fetch, compress_dev, compress_raw, the coder bounds,
    block mode and device decompression of deep (unflattened) sle / ascii streams.

Every test first asserts that its input reaches the edge it is named for, so that none of them can pass vacuously."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tudocomp_amd import blocks as B

pytestmark = pytest.mark.gpu

MiB = 1 << 20
ORB_SUPER = 1 << 20          # prim.hip / lzss_lcp.hip: entries per super-tile of orbit marking and ANSV
SEG_INLINE = 508             # factorize.hip: push-target descriptors that travel in the level's scalar read-back
N3 = (3 << 20) + 4321
N16 = (16 << 20) + 4321

# name -> (device coder, oracle coder, kmer)
CODERS = {"huff": (T.CODER_HUFF, "huff", 3), "arith": (T.CODER_ARITH, "arith", 3), "ascii": (T.CODER_ASCII, "ascii", 3)}
for _k in range(1, 8):
    CODERS["sle%d" % _k] = (T.CODER_SLE | (_k << 8), "sle", _k)
COMPS = {"arrays": T.COMP_ARRAYS, "plcppeaks": T.COMP_PLCPPEAKS, "max_lcp": T.COMP_MAXLCP, "heap": T.COMP_HEAP}


def _desc(b):
    return "%d bytes sha256 %s" % (len(b), hashlib.sha256(bytes(b)).hexdigest()[:16])


def _same(got, want, what):
    assert got == want, "%s: device %s, oracle %s" % (what, _desc(got), _desc(want))


def _versioned(n, seed=5, copies=20):
    """a versioned collection: `copies` copies of one document, each with 0.2 % point edits against the previous one"""
    rng = np.random.default_rng(seed)
    base = rng.integers(97, 123, n // copies + 1, dtype=np.uint8)
    out = []
    for _ in range(copies):
        v = base.copy()
        idx = rng.integers(0, len(v), max(1, len(v) // 500))
        v[idx] = rng.integers(97, 123, len(idx), dtype=np.uint8)
        out.append(v)
        base = v
    return np.concatenate(out)[:n].tobytes()


def _fibonacci(n):
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def _random_runs(n, seed=5):
    rng = np.random.default_rng(seed)
    k = n // 30 + 1
    return np.repeat(rng.integers(97, 100, k, dtype=np.uint8), rng.integers(1, 80, k))[:n].tobytes()


def _repeat_pair(rlen, tail=5000, seed=9):
    """R + R + tail with R random over 1..254 (nothing to escape): one factor of |R| bytes starting at |R|"""
    rng = np.random.default_rng(seed)
    r = rng.integers(1, 255, rlen, dtype=np.uint8).tobytes()
    return r + r + rng.integers(1, 255, tail, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def text_of(kind, n):
    """escaped, 0-terminated text of about n bytes (exactly n for the generators without 0x00 / 0xFF)"""
    gens = {"english": lambda: T.gen_english(n - 1, 17).tobytes(), "dna": lambda: T.gen_dna(n - 1, 19).tobytes(),
            "versioned": lambda: _versioned(n - 1), "fibonacci": lambda: _fibonacci(n - 1), "runs": lambda: _random_runs(n - 1)}
    return O.escape(gens[kind]())


@functools.lru_cache(maxsize=None)
def want(kind, n, comp, coder, thr, fl):
    """the oracle's stream (cached per module: several tests share cells)"""
    _, oc, k = CODERS[coder]
    return O.lcpcomp_compress_any(text_of(kind, n), thr, fl, oc, comp, kmer=k)


def _wide(st, n, fused=None):
    """the wide suffix sort ran (bit-packed keys; wsort_min = 2^20).  fused: ISA / Phi / PLCP came (1) from the fused scatter of the
    final suffix array -- where the wide sort separates every suffix without doubling rounds, as on the English generator -- or
    (0) from the classic Phi / PLCP kernels behind the doubling rounds (DNA, long repeats)"""
    got = {k: st[k] for k in ("n", "sa_key_words", "sa_mode")}
    assert st["n"] == n and st["sa_key_words"] >= 1, got
    if fused is not None:
        assert st["sa_mode"] == fused, got


# ---- 1. strategy x coder matrix at 3 MiB + 4321 --------------------------------------------------------------------------------
MATRIX_TEXTS = ("english", "dna")
MATRIX_COMPS = ("arrays", "max_lcp", "plcppeaks")
MATRIX_CODERS = ("huff", "arith", "ascii", "sle1", "sle3", "sle4", "sle7")


def _matrix_cell(ti, si, ci):
    """threshold and flatten of one cell: thr = (1, 2, 5)[(ci + si + ti) % 3], flatten = (ci + ti) % 2.  A coder meets all three
    thresholds over the three strategies of one text, and both flatten values over the two texts; a strategy meets every threshold
    and both flatten values over the seven coders of one text."""
    return (1, 2, 5)[(ci + si + ti) % 3], (ci + ti) % 2


MATRIX = [(t, s, c) + _matrix_cell(ti, si, ci) for ti, t in enumerate(MATRIX_TEXTS) for si, s in enumerate(MATRIX_COMPS)
          for ci, c in enumerate(MATRIX_CODERS)]


def cell(kind, comp, coder):
    """(threshold, flatten) of a matrix cell: the entry-point tests reuse the matrix cells, so the oracle runs once per stream"""
    return next((c[3], c[4]) for c in MATRIX if c[:3] == (kind, comp, coder))


def test_matrix_pattern_covers_every_strategy_and_coder():
    for key, idx in (("comp", 1), ("coder", 2)):
        for v in set(c[idx] for c in MATRIX):
            cells = [c for c in MATRIX if c[idx] == v]
            assert {c[4] for c in cells} == {0, 1} and 1 in {c[3] for c in cells}, (key, v)


@pytest.mark.parametrize("kind,comp,coder,thr,fl", MATRIX, ids=["%s-%s-%s-t%d-f%d" % c for c in MATRIX])
def test_matrix_3MiB(gpu_ctx, kind, comp, coder, thr, fl):
    text = text_of(kind, N3)
    assert len(text) == N3 and N3 > 3 * ORB_SUPER
    w, wst = want(kind, N3, comp, coder, thr, fl)
    got, st = gpu_ctx.lcpcomp_compress(text, thr, fl, CODERS[coder][0], COMPS[comp])
    _wide(st, N3, fused=int(kind == "english"))
    _same(got, w, "%s %s/%s t=%d flatten=%d" % (kind, comp, coder, thr, fl))
    assert st["factors"] == wst["factors"]


def test_narrow_sort_is_detected(gpu_ctx):
    """the wide-path assertion of the matrix fails where the wide sort is switched off (wsort_min above n); the stream stays right"""
    kind, comp, coder = "english", "plcppeaks", "sle4"
    thr, fl = cell(kind, comp, coder)
    with T.Context(0, options={"wsort_min": 1 << 23}) as ctx:
        got, st = ctx.lcpcomp_compress(text_of(kind, N3), thr, fl, CODERS[coder][0], COMPS[comp])
    assert st["sa_key_words"] == 0 and st["sa_mode"] == 0
    with pytest.raises(AssertionError):
        _wide(st, N3)
    _same(got, want(kind, N3, comp, coder, thr, fl)[0], "narrow sort")


def test_heap_on_the_wide_path(gpu_ctx):
    """MaxHeapStrategy (one device thread) once on a text above wsort_min"""
    n = MiB + 4097
    text = text_of("dna", n)
    w, _ = want("dna", n, "heap", "sle3", 3, 1)
    got, st = gpu_ctx.lcpcomp_compress(text, 3, 1, CODERS["sle3"][0], T.COMP_HEAP)
    _wide(st, n)
    _same(got, w, "dna heap/sle3")


# ---- 2. factors longer than a super-tile ----------------------------------------------------------------------------------------
LONG_TEXTS = {"off_boundary": MiB + (MiB >> 2) + 123, "on_boundary": 2 * MiB}     # |R|: the factor starts at |R|


@functools.lru_cache(maxsize=None)
def _long_text(name):
    return O.escape(_repeat_pair(LONG_TEXTS[name]))


@pytest.mark.parametrize("name", sorted(LONG_TEXTS))
@pytest.mark.parametrize("thr", (1, 3))
@pytest.mark.parametrize("comp", ("plcppeaks", "max_lcp", "arrays", "lzss_lcp"))
def test_factor_longer_than_a_super_tile(gpu_ctx, name, thr, comp):
    text = _long_text(name)
    rlen = LONG_TEXTS[name]
    assert (rlen % ORB_SUPER == 0) == (name == "on_boundary")
    if comp == "lzss_lcp":
        w, wst = O.lzss_lcp_huff_compress(text, thr)
        got, st = gpu_ctx.lzss_lcp_compress(text, thr)
        pos, src, ln = gpu_ctx.lzss_lcp_factorize(text, thr)
        start = int(pos[int(np.argmax(ln))])           # (a short factor in front may reach a few bytes into the second R)
        assert int(ln.max()) > ORB_SUPER and 0 <= start - rlen < 64 and (start % ORB_SUPER == 0) == (name == "on_boundary"), (start, rlen)
    else:
        w, wst = O.lcpcomp_compress_any(text, thr, 1, "huff", comp)
        got, st = gpu_ctx.lcpcomp_compress(text, thr, 1, T.CODER_HUFF, COMPS[comp])
        _wide(st, len(text))
    # one factor covers a whole super-tile: the walk over super-tiles skips at least one
    assert wst["flen_max"] > rlen - 64 > ORB_SUPER, wst["flen_max"]
    _same(got, w, "%s %s t=%d" % (name, comp, thr))


# ---- 3. the max_lcp level loop on structured multi-MB texts ---------------------------------------------------------------------
STRUCTURED = (("versioned", 3 * MiB + 11, 5), ("fibonacci", 2 * MiB + 13, 2), ("runs", 3 * MiB + 17, 2), ("versioned", 3 * MiB + 11, 2))


@pytest.fixture(scope="module")
def max_lcp_structured(gpu_ctx):
    out = {}
    for kind, n, thr in STRUCTURED:
        got, st = gpu_ctx.lcpcomp_compress(text_of(kind, n), thr, 1, T.CODER_HUFF, T.COMP_MAXLCP)
        out[(kind, n, thr)] = (got, st)
    return out


@pytest.mark.parametrize("kind,n,thr", STRUCTURED, ids=["%s-t%d" % (k, t) for k, _, t in STRUCTURED])
def test_max_lcp_structured(max_lcp_structured, kind, n, thr):
    got, st = max_lcp_structured[(kind, n, thr)]
    _wide(st, len(text_of(kind, n)))
    assert st["maxlcp"] >= 128 and st["levels"] > 0 and st["pushes"] > 0, {k: st[k] for k in ("maxlcp", "levels", "pushes")}
    _same(got, want(kind, n, "max_lcp", "huff", thr, 1)[0], "max_lcp %s t=%d" % (kind, thr))


def test_max_lcp_loop_branches_reached(max_lcp_structured):
    """over the structured texts: the G=64 kernels (levels >= 128), skip-ahead probes after dead levels, and a level whose pushes go
    to more than SEG_INLINE target levels (the segment list is read back separately)"""
    sts = [st for _, st in max_lcp_structured.values()]
    summary = [{k: st[k] for k in ("maxlcp", "levels", "pushes", "probes", "max_push_targets")} for st in sts]
    assert max(st["probes"] for st in sts) > 0, summary
    assert max(st["max_push_targets"] for st in sts) > SEG_INLINE, summary


# ---- 4. 16 MiB ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("english", "versioned"))
@pytest.mark.parametrize("thr", (1, 3))
def test_lzss_lcp_16MiB(gpu_ctx, kind, thr):
    text = text_of(kind, N16)
    w, _ = O.lzss_lcp_huff_compress(text, thr)
    got, st = gpu_ctx.lzss_lcp_compress(text, thr)
    assert st["n"] == len(text) > 16 * ORB_SUPER
    _same(got, w, "lzss_lcp %s t=%d" % (kind, thr))


BIG = (("english", "max_lcp", "huff", 2, 1), ("dna", "plcppeaks", "ascii", 3, 0), ("english", "arrays", "sle7", 2, 0),
       ("dna", "max_lcp", "arith", 1, 1))


@pytest.mark.parametrize("kind,comp,coder,thr,fl", BIG, ids=["%s-%s" % (c[1], c[2]) for c in BIG])
def test_16MiB_cell(gpu_ctx, kind, comp, coder, thr, fl):
    text = text_of(kind, N16)
    w, _ = O.lcpcomp_compress_any(text, thr, fl, CODERS[coder][1], comp, kmer=CODERS[coder][2])
    got, st = gpu_ctx.lcpcomp_compress(text, thr, fl, CODERS[coder][0], COMPS[comp])
    _wide(st, N16)
    _same(got, w, "16 MiB %s %s/%s" % (kind, comp, coder))


# ---- 5. entry points ---------------------------------------------------------------------------------------------------------
INTO = (("arrays", "ascii"), ("arrays", "arith"), ("arrays", "sle3"), ("max_lcp", "huff"))


@pytest.mark.parametrize("comp,coder", INTO, ids=["%s-%s" % c for c in INTO])
def test_compress_into(gpu_ctx, comp, coder):
    """into a buffer of bound(n, coder) bytes: the stream of lcpcomp_compress and of the oracle.  Except for SLE (its own pack
    in one pass) the front of the stream leaves in chunks while the pack still runs (d2h_early)."""
    text = text_of("english", N3)
    dc = CODERS[coder][0]
    thr, fl = cell("english", comp, coder)
    w, _ = want("english", N3, comp, coder, thr, fl)
    host, _ = gpu_ctx.lcpcomp_compress(text, thr, fl, dc, COMPS[comp])
    tb = T.PinnedBuffer(len(text))
    ob = T.PinnedBuffer(gpu_ctx.bound(len(text), dc))
    try:
        tb.a[:] = np.frombuffer(text, dtype=np.uint8)
        ln, st = gpu_ctx.lcpcomp_compress_into(tb, len(text), ob, thr, fl, dc, COMPS[comp])
        _wide(st, N3)
        if coder.startswith("sle"):
            assert st["d2h_early"] == 0
        else:
            assert 0 < st["d2h_early"] < ln, st["d2h_early"]
        got = ob.a[:ln].tobytes()
    finally:
        tb.free(); ob.free()
    _same(got, w, "compress_into %s/%s" % (comp, coder))
    _same(host, w, "compress %s/%s" % (comp, coder))


@pytest.mark.parametrize("comp,coder", INTO, ids=["%s-%s" % c for c in INTO])
def test_compress_into_one_byte_short(gpu_ctx, comp, coder):
    """a buffer one byte shorter than the stream: TDC_GPU_ERR_OOM, *out_len = the required size, nothing written behind the buffer"""
    thr, fl = cell("english", comp, coder)
    text = np.frombuffer(text_of("english", N3), dtype=np.uint8)
    w, _ = want("english", N3, comp, coder, thr, fl)
    guard = 1 << 16
    buf = np.full(len(w) - 1 + guard, 0xA5, dtype=np.uint8)
    L = T._native.load()
    ol, st = ctypes.c_size_t(), T.Stats()
    rc = L.tdc_gpu_lcpcomp_compress_into(gpu_ctx._h, text.ctypes.data_as(ctypes.c_void_p), len(text), thr, fl, CODERS[coder][0],
                                         COMPS[comp], buf.ctypes.data_as(ctypes.c_void_p), len(w) - 1, ctypes.byref(ol), ctypes.byref(st))
    assert rc == -5 and ol.value == len(w), (rc, ol.value, len(w))
    assert (buf[len(w) - 1:] == 0xA5).all()
    got, _ = gpu_ctx.lcpcomp_compress(text, thr, fl, CODERS[coder][0], COMPS[comp])      # the context is still usable
    _same(got, w, "after the refused call")


def test_compress_keep_and_fetch(gpu_ctx):
    for kind, coder in (("english", "sle3"), ("dna", "sle7")):
        text = text_of(kind, N3)
        thr, fl = cell(kind, "plcppeaks", coder)
        w, _ = want(kind, N3, "plcppeaks", coder, thr, fl)
        ln, st = gpu_ctx.lcpcomp_compress_keep(text, len(text), thr, fl, CODERS[coder][0], T.COMP_PLCPPEAKS)
        _wide(st, N3)
        assert ln == len(w)
        small = np.zeros(ln - 1, dtype=np.uint8)
        with pytest.raises(T.TdcGpuError):
            gpu_ctx.stream_fetch(small)
        out = np.zeros(ln + 8, dtype=np.uint8)
        assert gpu_ctx.stream_fetch(out) == ln
        _same(out[:ln].tobytes(), w, "keep + fetch %s/%s" % (kind, coder))
    # the NULL checks of the entry point: no length pointer, no text
    L = T._native.load()
    text = np.frombuffer(text_of("english", N3), dtype=np.uint8)
    tp, ol = text.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t()
    rc = L.tdc_gpu_lcpcomp_compress_keep(gpu_ctx._h, tp, len(text), 2, 1, T.CODER_HUFF, T.COMP_ARRAYS, None, None)
    assert rc == -2 and L.tdc_gpu_last_error(gpu_ctx._h) == b"out/out_len is NULL"
    rc = L.tdc_gpu_lcpcomp_compress_keep(gpu_ctx._h, None, len(text), 2, 1, T.CODER_HUFF, T.COMP_ARRAYS, ctypes.byref(ol), None)
    assert rc == -2 and L.tdc_gpu_last_error(gpu_ctx._h) == b"text is NULL"
    with pytest.raises(T.TdcGpuError):                  # (a refused call keeps no stream either)
        gpu_ctx.stream_fetch(np.zeros(8, dtype=np.uint8))


def test_compress_dev(gpu_ctx):
    """device buffers (hipMalloc through ctypes, as in test_gpu_blocks: no dependence on torch's device initialisation): every coder
    gives the host entry's stream; an out_cap that is too small is refused and nothing behind it is written"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    H2D, D2H = 1, 2
    text = np.frombuffer(text_of("english", N3), dtype=np.uint8)
    guard = 1 << 16
    cap = max(gpu_ctx.bound(len(text), CODERS[c][0]) for c in CODERS)
    pattern = np.full(cap + guard, 0xA5, dtype=np.uint8)
    d_text, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_text), len(text)) == 0
    assert hip.hipMalloc(ctypes.byref(d_out), cap + guard) == 0
    try:
        assert hip.hipMemcpy(d_text, text.ctypes.data_as(ctypes.c_void_p), len(text), H2D) == 0

        def fill():
            assert hip.hipMemcpy(d_out, pattern.ctypes.data_as(ctypes.c_void_p), cap + guard, H2D) == 0

        def read():
            back = np.empty(cap + guard, dtype=np.uint8)
            assert hip.hipMemcpy(back.ctypes.data_as(ctypes.c_void_p), d_out, cap + guard, D2H) == 0
            return back

        for coder in ("huff", "arith", "ascii", "sle1", "sle4"):
            dc = CODERS[coder][0]
            thr, fl = cell("english", "arrays", coder)
            bound = gpu_ctx.bound(len(text), dc)
            fill()
            ln, st = gpu_ctx.lcpcomp_compress_dev(d_text.value, len(text), d_out.value, bound, thr, fl, dc)
            _wide(st, N3, fused=1)
            back = read()
            got = back[:ln].tobytes()
            host, _ = gpu_ctx.lcpcomp_compress(text, thr, fl, dc)
            _same(got, host, "compress_dev vs compress %s" % coder)
            _same(got, want("english", N3, "arrays", coder, thr, fl)[0], "compress_dev %s" % coder)
            assert (back[bound:] == 0xA5).all(), coder
            fill()
            with pytest.raises(T.TdcGpuError):
                gpu_ctx.lcpcomp_compress_dev(d_text.value, len(text), d_out.value, ln // 2, thr, fl, dc)
            assert (read()[ln // 2:] == 0xA5).all(), coder
    finally:
        hip.hipFree(d_text)
        hip.hipFree(d_out)


@functools.lru_cache(maxsize=None)
def _escape_heavy(n, seed=23):
    """DNA with 0x00 / 0xFF sprinkled in: a third of the bytes need escaping, repeats survive"""
    rng = np.random.default_rng(seed)
    a = T.gen_dna(n, seed).copy()
    idx = rng.integers(0, n, n // 3)
    a[idx] = np.where(rng.integers(0, 2, len(idx)) == 0, 0, 255).astype(np.uint8)
    return (a.tobytes() * 2)[:n]


@pytest.mark.parametrize("coder,thr", (("arith", 3), ("ascii", 2), ("sle2", 2), ("sle5", 4)))
def test_compress_raw_escape_heavy(gpu_ctx, coder, thr):
    data = _escape_heavy(MiB + 333)
    esc = O.escape(data)
    assert len(esc) > len(data) + len(data) // 4
    w, _ = O.lcpcomp_compress_any(esc, thr, 1, CODERS[coder][1], "arrays", kmer=CODERS[coder][2])
    got, st = gpu_ctx.lcpcomp_compress_raw(data, thr, 1, CODERS[coder][0])
    _wide(st, len(esc))
    _same(got, w, "compress_raw %s" % coder)


def test_bound_coder_on_worst_inputs(gpu_ctx):
    """random bytes at threshold 1, a text of 0xFF only, one literal run: every coder's stream fits bound(n, coder)"""
    rng = np.random.default_rng(29)
    n = MiB + 5
    rnd = rng.integers(1, 255, n - 1, dtype=np.uint8).tobytes() + b"\0"
    cases = (("random t=1", rnd, 1), ("0xFF only", b"\xff" * (n - 1) + b"\0", 1), ("literal run", rnd, 1 << 30))
    for name, text, thr in cases:
        for coder in ("huff", "arith", "ascii", "sle1", "sle3", "sle7"):
            dc = CODERS[coder][0]
            got, st = gpu_ctx.lcpcomp_compress(text, thr, 1, dc)
            if name == "literal run":
                assert st["factors"] == 0
            assert len(got) <= gpu_ctx.bound(n, dc), (name, coder, len(got), gpu_ctx.bound(n, dc))
            _same(got, O.lcpcomp_compress_any(text, thr, 1, CODERS[coder][1], "arrays", kmer=CODERS[coder][2])[0], "%s %s" % (name, coder))
    assert len(O.lcpcomp_compress_any(rnd, 1 << 30, 1, "ascii", "arrays")[0]) > n        # ASCII streams can be larger than their text


@pytest.mark.parametrize("coder", ("arith", "ascii", "sle3", "sle6"))
def test_blocks_non_huff(gpu_ctx, coder):
    """ragged blocks around 2^20: every payload is the oracle stream of its block; ascii / sle round-trip; an arithmetic container
    is refused with TDC_GPU_ERR_UNSUPPORTED"""
    data = _escape_heavy(MiB // 2)[:300_000] + T.gen_english(3 * MiB, 31).tobytes()
    bs = MiB + 777
    dc, oc, k = CODERS[coder]
    blob, sts = T.blocks_compress(data, bs, 3, 1, dc, devices=[0])
    parts = B.unpack_container(blob)
    assert len(parts) == 4 and 0 < len(data) - 3 * bs < bs
    for i, (raw_len, payload) in enumerate(parts):
        block = data[i * bs:(i + 1) * bs]
        assert raw_len == len(block)
        _same(payload, O.lcpcomp_compress_any(O.escape(block), 3, 1, oc, "arrays", kmer=k)[0], "block %d %s" % (i, coder))
    if coder == "arith":
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.blocks_decompress(blob, dc)
        assert e.value.status == -6
    else:
        assert gpu_ctx.blocks_decompress(blob, dc) == data


DEEP = (("english", "max_lcp", "ascii"), ("english", "plcppeaks", "sle3"), ("dna", "max_lcp", "sle1"), ("dna", "plcppeaks", "sle4"))


@pytest.mark.parametrize("kind,comp,coder", DEEP, ids=["%s-%s-%s" % c for c in DEEP])
def test_decompress_deep_chains(gpu_ctx, kind, comp, coder):
    """unflattened streams (flatten=0: source chains through earlier factors) at 3 MiB decode on the device and in the oracle"""
    text = text_of(kind, N3)
    dc, oc, k = CODERS[coder]
    thr, fl = cell(kind, comp, coder)
    assert fl == 0
    _, fst = O.lcpcomp_compress_any(text, thr, 1, oc, comp, kmer=k)
    assert fst["num_flattened"] > 0 and fst["max_depth_lb"] >= 2, fst      # chains of references that flatten=1 would remove
    w, _ = want(kind, N3, comp, coder, thr, fl)
    got, st = gpu_ctx.lcpcomp_compress(text, thr, fl, dc, COMPS[comp])
    _same(got, w, "%s %s/%s flatten=0" % (kind, comp, coder))
    back, info = gpu_ctx.lcpcomp_decompress(w, dc)
    assert back == text
    assert (O.lcpcomp_ascii_decompress(w) if coder == "ascii" else O.lcpcomp_sle_decompress(w, k)) == text
