"""GPU tests of bwt over a batch of texts, both directions (tdc_gpu_bwt_compress_batch, tdc_gpu_bwt_decompress_batch,
tdc_gpu_suffix_array_batch; pytest -m gpu): every result is byte for byte what the single call returns for that text alone, every
status its code, and a refused text neither costs a neighbour anything nor has its range of `out` touched."""
import ctypes
import functools

import numpy as np
import pytest

import tudocomp_amd as T
from tests import bwt_batches as B
from tests.models import bwt as M
from tests.models import bwt_batch as MB

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_NO_SENTINEL, ERR_TOO_LARGE = 0, -2, -3, -4
CAP = 1 << 20


@functools.lru_cache(maxsize=None)
def single(ctx, text):
    """the single call on one text: the transform, or the negative status"""
    try:
        return ctx.bwt_compress(text)[0]
    except T.TdcGpuError as e:
        return e.status


@functools.lru_cache(maxsize=None)
def single_inverse(ctx, buf):
    try:
        return ctx.bwt_decompress(buf)[0]
    except T.TdcGpuError as e:
        return e.status


def forward_into(ctx, texts, fill=0xA5):
    """the batch call on a buffer full of `fill`: (list of ranges of out, statuses, stats)"""
    off = T._offsets([len(t) for t in texts])
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    out = np.full(max(len(data), 1), fill, dtype=np.uint8)
    status, st = ctx.bwt_compress_batch_into(data, off, out)
    return [out[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])], status.tolist(), st


def inverse_into(ctx, bufs, fill=0xA5):
    off = T._offsets([len(t) for t in bufs])
    data = np.frombuffer(b"".join(bufs), dtype=np.uint8)
    out = np.full(max(len(data), 1), fill, dtype=np.uint8)
    status, st = ctx.bwt_decompress_batch_into(data, off, out)
    return [out[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])], status.tolist(), st


def check_forward(ctx, texts):
    got, status, st = forward_into(ctx, texts)
    for k, (t, g, s) in enumerate(zip(texts, got, status)):
        want = single(ctx, t)
        if isinstance(want, int):
            assert s == want and g == b"\xa5" * len(t), (k, len(t), s, want)
        else:
            assert s == OK and g == want, (k, len(t), s)
            if len(t) < 2000:
                assert g == M.bwt_forward(t), (k, len(t))
    return got, status, st


def check_inverse(ctx, bufs):
    got, status, st = inverse_into(ctx, bufs)
    for k, (b, g, s) in enumerate(zip(bufs, got, status)):
        want = single_inverse(ctx, b)
        if isinstance(want, int):
            assert s == want and g == b"\xa5" * len(b), (k, len(b), s, want)
        elif len(b) <= 1:
            assert s == OK and want == b"" and g == b"\xa5" * len(b), (k, len(b), s)
        else:
            assert s == OK and g == want, (k, len(b), s)
    return got, status, st


@pytest.mark.parametrize("nature", B.NATURES)
def test_forward_and_round_trip_by_length(gpu_ctx, nature):
    texts = [B.text(nature, n) for n in B.LENGTHS]
    got, status, st = check_forward(gpu_ctx, texts)
    assert status == [OK] * len(texts) and st["len_rounds"] <= 18
    sas, sa_status, _ = gpu_ctx.suffix_array_batch(texts)
    assert sa_status == status
    for t, sa in zip(texts, sas):
        assert np.array_equal(sa, gpu_ctx.suffix_array(t)[0] if len(t) >= 2 else [0]), len(t)
    back, bstatus, _ = check_inverse(gpu_ctx, got)
    assert bstatus == [OK] * len(texts)
    assert [b for b, t in zip(back, texts) if len(t) >= 2] == [t for t in texts if len(t) >= 2]


def test_longest_run_of_a_17_bit_text(gpu_ctx):
    """a^131071 0: 2^17 bytes, the most rounds a 17-bit text takes (4 * 2^15 symbols reach it), within bits_for(n) + 1"""
    t = B.text("a_run", 1 << 17)
    got, status, st = check_forward(gpu_ctx, [b"b\x00", t, b"\x00"])
    assert status == [OK] * 3 and st["len_rounds"] == 15
    sas, _, _ = gpu_ctx.suffix_array_batch([t])
    assert np.array_equal(sas[0], np.arange((1 << 17) - 1, -1, -1, dtype=np.uint32))
    check_inverse(gpu_ctx, got)


def test_borders(gpu_ctx):
    a = B.text("random2", 5000, 5)
    long1, long2 = B.text("english", 30000, 6), B.text("fibonacci", 20000)
    pre, suf = a[:2000] + b"\x00", a[1234:]
    batch = [a, a, pre, a, suf, long1, b"\x00", long2, b"\x00", b"\x00", long1, pre, a[:-1][:4095] + b"\x00", a]
    got, status, _ = check_forward(gpu_ctx, batch)
    assert status == [OK] * len(batch)
    assert got[0] == got[1] == got[3] == got[-1]
    back, bstatus, _ = check_inverse(gpu_ctx, got)
    assert bstatus == [OK] * len(batch)


def test_refusals_stand_alone(gpu_ctx):
    good, good2 = B.text("english", 7000, 8), B.text("escapes", 3001, 2)
    too_long = B.text("english", CAP + 1, 3)
    batch = [good, b"ab\x00cd\x00", good2, b"abc", good, b"", good2, too_long, good, b"\x00\x00", b"\x00", b"a" * 300, good2]
    want = [OK, ERR_ARG, OK, ERR_NO_SENTINEL, OK, ERR_NO_SENTINEL, OK, ERR_TOO_LARGE, OK, ERR_ARG, OK, ERR_NO_SENTINEL, OK]
    got, status, st = forward_into(gpu_ctx, batch)
    assert status == want
    for t, g, s in zip(batch, got, status):
        if s == OK:
            assert g == single(gpu_ctx, t)
        else:
            assert g == b"\xa5" * len(t)                         # untouched
            assert len(t) > CAP or single(gpu_ctx, t) == s
    # the text of no bytes: the single call says "no sentinel" (api.hpp check_text_args: a length of 0 behind a pointer that is not NULL)
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.bwt_compress(np.zeros(1, dtype=np.uint8)[:0])
    assert e.value.status == ERR_NO_SENTINEL == status[5] and batch[5] == b""
    assert st["sa_sorted_elems"] < 40 * sum(len(t) for t, s in zip(batch, want) if s == OK)   # the long text was not sorted


def test_text_at_the_cap(gpu_ctx):
    t = B.text("english", CAP, 4)
    got, status, _ = forward_into(gpu_ctx, [b"x\x00", t])
    assert status == [OK, OK] and got[1] == single(gpu_ctx, t)
    back, bstatus, _ = inverse_into(gpu_ctx, got)
    assert bstatus == [OK, OK] and back[1] == t


def test_more_texts_than_the_grid(gpu_ctx):
    rng = np.random.default_rng(5)
    texts = [rng.integers(97, 100, int(n) - 1, dtype=np.uint8).tobytes() + b"\x00" for n in rng.integers(1, 41, 5000)]
    got, status, _ = forward_into(gpu_ctx, texts)
    assert status == [OK] * 5000
    sas, outs, _ = MB.forward(texts[:300])
    assert got[:300] == outs
    assert got == [M.bwt_forward(t) for t in texts]
    back, bstatus, _ = inverse_into(gpu_ctx, got)
    assert bstatus == [OK] * 5000
    assert all(b == t or len(t) == 1 for b, t in zip(back, texts))


def test_many_refused_texts_between_good_ones(gpu_ctx):
    """more runs of accepted neighbours than travel in copies of their own: the results go through one staging copy, and the ranges of
    the refused texts stay untouched all the same"""
    good = [B.text("english", 300 + k, k) for k in range(100)]
    batch = [t for k, g in enumerate(good) for t in (g, (b"no end", b"in\x00ner\x00", b"")[k % 3])]
    got, status, _ = check_forward(gpu_ctx, batch)
    assert status[::2] == [OK] * 100 and set(status[1::2]) == {ERR_NO_SENTINEL, ERR_ARG}
    sas, sa_status, _ = gpu_ctx.suffix_array_batch(batch)
    assert sa_status == status and all(np.array_equal(sa, M.suffix_array_naive(t)) for sa, t in zip(sas[::2], good))
    bufs = [b for k, g in enumerate(got[::2]) for b in (g, (b"\x00a", b"abc", b"x")[k % 3])]
    back, bstatus, _ = check_inverse(gpu_ctx, bufs)
    assert back[::2] == good and bstatus[1::2] == [ERR_ARG, ERR_ARG, OK] * 33 + [ERR_ARG]


@functools.lru_cache(maxsize=None)
def inverse_pool():
    """transforms and buffers that are none, each bad one between good ones"""
    good_t = [B.text("english", 9000, 9), B.text("ab", 4097), B.text("escapes", 700, 3), b"q\x00"]
    good = [M.bwt_from_sa(t, _sa(t)) for t in good_t]
    base = bytearray(M.bwt_from_sa(B.text("random255", 20001, 4), _sa(B.text("random255", 20001, 4))))
    rng = np.random.default_rng(11)
    swapped = None
    for _ in range(60):
        i, j = (int(x) for x in rng.integers(0, len(base), 2))
        if base[i] and base[j] and base[i] != base[j]:
            cand = bytearray(base)
            cand[i], cand[j] = cand[j], cand[i]
            rows = MB.cycle_rows(bytes(cand))
            if len(rows) == 2 and min(map(len, rows)) >= 4000:   # both cycles are long (the test asserts that each holds sampled heads)
                swapped = bytes(cand)
                break
    assert swapped is not None
    bad = [b"\x00a", b"a\x00b\x00c", b"abcabc", b"\x00\x00", b"ba\x00", swapped]
    bufs = []
    for k, b in enumerate(bad):
        bufs += [good[k % len(good)], b]
    bufs += [b"", b"a", b"\x00", bytes(base), good[0]]
    return tuple(bufs)


def _sa(t):
    """suffix array of a 0-terminated text without a 0 inside (numpy doubling; the tests' own, for texts too long for the naive model)"""
    a = np.frombuffer(t, dtype=np.uint8).astype(np.int64)
    n = len(a)
    rank, h = a.copy(), 1
    while True:
        second = np.concatenate([rank[h:] + 1, np.zeros(min(h, n), dtype=np.int64)])[:n]
        order = np.lexsort((second, rank))
        key = rank[order] * (n + 2) + second[order]
        new = np.zeros(n, dtype=np.int64)
        new[order] = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank = new
        if rank.max() == n - 1:
            return np.argsort(rank)
        h *= 2


def test_inverse_verdicts_stand_alone(gpu_ctx):
    bufs = list(inverse_pool())
    got, status, st = check_inverse(gpu_ctx, bufs)
    assert status.count(ERR_ARG) == 6 and status.count(OK) == len(bufs) - 6
    assert st["levels"] >= 1 and st["len_rounds"] >= 1
    # the swapped transform: two cycles, both long, and each holds rows that the default sampling over the call's rows makes heads
    k = 11
    first, n = sum(len(b) for b in bufs[:k]), sum(len(b) for b in bufs)
    rows = MB.cycle_rows(bufs[k])
    assert len(bufs[k]) == 20001 and status[k] == ERR_ARG and len(rows) == 2 and min(map(len, rows)) >= 4000
    T_ = M.head_threshold(n, M.DEFAULT_SAMPLE)
    for cyc in rows:
        assert sum(1 for r in cyc if r and M.mix(first + r, n) < T_) >= 4


def test_inverse_with_short_lists(gpu_ctx):
    """sample 4, steps 8: several launches of the first walk, appended heads, the same bytes"""
    bufs = list(inverse_pool())
    want = inverse_into(gpu_ctx, bufs)
    with T.Context(0, options={"bwt_batch_sample": 4, "bwt_batch_steps": 8}) as ctx:
        got = inverse_into(ctx, bufs)
    assert got[:2] == want[:2]
    assert got[2]["levels"] >= 2 and got[2]["entries"] > want[2]["entries"] and got[2]["flen_max"] <= 8


@pytest.mark.parametrize("fill", (0x00, 0x01, 0xFF))
def test_arena_state(fill):
    texts = [B.text("english", 5000, 2), b"ab\x00cd\x00", B.text("a_run", 4097), b"", b"\x00", B.text("random2", 65537), b"nope"]
    bufs = list(inverse_pool())
    with T.Context(0) as ctx:
        fwd, inv = forward_into(ctx, texts), inverse_into(ctx, bufs)
        sas = ctx.suffix_array_batch(texts)
        where = ctx.prim_arena_fill(fill)
        assert where[1] > 0
        fwd2 = forward_into(ctx, texts)
        ctx.prim_arena_fill(fill)
        sas2 = ctx.suffix_array_batch(texts)
        ctx.prim_arena_fill(fill)
        inv2 = inverse_into(ctx, bufs)
        assert ctx.prim_arena_fill() == where, "the arena moved or grew"
    assert fwd2[:2] == fwd[:2] and inv2[:2] == inv[:2] and sas2[1] == sas[1]
    assert all(np.array_equal(a, b) for a, b in zip(sas[0], sas2[0]))
    drop = ("ms_h2d", "ms_sa", "ms_encode", "ms_d2h", "ms_total", "arena_bytes")       # (arena_bytes: the high-water mark of the context)
    assert {k: v for k, v in fwd2[2].items() if k not in drop} == {k: v for k, v in fwd[2].items() if k not in drop}
    assert {k: v for k, v in inv2[2].items() if k not in drop} == {k: v for k, v in inv[2].items() if k not in drop}


def test_facades(gpu_ctx):
    rng = np.random.default_rng(3)
    raws = [b"", b"\x00", b"\xff\x00\xff", rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), bytes([0, 255] * 500), b"plain text " * 40]
    z = T.BWTCompressor(gpu_ctx)
    streams, status = z.compress_batch(raws)
    assert status == [OK] * len(raws)
    assert streams == [z.compress(r) for r in raws]
    back, bstatus = z.decompress_batch(streams + [b"\x00a"])
    assert bstatus == [OK] * len(raws) + [ERR_ARG]
    assert back == raws + [None]


def test_output_buffer_too_small(gpu_ctx):
    texts = [B.text("english", 500, 1), b"abc"]
    off = T._offsets([len(t) for t in texts])
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    out = np.full(100, 0xA5, dtype=np.uint8)
    for call in (gpu_ctx.bwt_compress_batch_into, gpu_ctx.bwt_decompress_batch_into):
        with pytest.raises(T.TdcGpuError) as e:
            call(data, off, out)
        assert e.value.status == -5 and e.value.required == 503 and bytes(out) == b"\xa5" * 100
    # the C calls: status is filled with what needs no device although nothing is written -- forward the lengths and the terminator,
    # inverse "accepted so far"; also with out == NULL
    L = T._native.load()
    texts = [B.text("english", 500, 1), b"abc", b"", B.text("ab", 90), b"a" * (CAP + 1)]
    off = T._offsets([len(t) for t in texts])
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for fn, want in ((L.tdc_gpu_bwt_compress_batch, [OK, ERR_NO_SENTINEL, ERR_NO_SENTINEL, OK, ERR_TOO_LARGE]),
                     (L.tdc_gpu_bwt_decompress_batch, [OK] * 5)):
        for dst, cap in ((ptr(out), 100), (None, 0), (None, 1 << 30)):
            status = np.full(5, 77, dtype=np.int32)
            assert fn(gpu_ctx._h, ptr(data), ptr(off), 5, dst, cap, ptr(status), None) == -5
            assert status.tolist() == want and bytes(out) == b"\xa5" * 100
    assert gpu_ctx.bwt_compress_batch([]) == ([], [], gpu_ctx.bwt_compress_batch([])[2])   # count = 0 is valid
