"""GPU tests of lzss over a batch of texts (tdc_gpu_lzss_sw_compress_batch; lzss_sw_batch.hip): every stream of a batch against the host
specification of its text alone -- M.encode(M.parse()) of tests/models/lzss_sw.py, for larger texts the host parse tdc_lzss_sw_factors
with the same fields (tests/lzss_sw_batches.py) -- at windows 1, 3, 16 and 4096, thresholds 0 and 3 and the four coders: text borders
against the match kernel's tiles, nothing reaching across a border, text-local widths under coder=bit, truncation per text, count 1 and
0, the refusals, and one larger batch that the batch decoder takes back to its texts."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import lzss_sw_batches as B
from tests.models import lzss_sw as M

pytestmark = pytest.mark.gpu

CODERS = M.CODERS
WT = [(w, t) for w in B.WINDOWS for t in B.THRESHOLDS]
KNOWN = [b"abcabcabcabc", b"", b"the cat sat on the mat, the cat sat"]


def run(ctx, texts, w, t, coder):
    """(streams, statuses, stats) through the caller-owned entry point; what holds for every call is asserted here"""
    lengths = [len(x) for x in texts]
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    cap = T.lzss_sw_batch_bound(lengths, w, B.CODER_ID[coder])
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    out_off, out_len, status, st = ctx.lzss_sw_compress_batch_into(data, off, out, w, t, B.CODER_ID[coder])
    assert out_off[0] == 0 and (out_off % 8 == 0).all() and (np.diff(out_off.astype(np.int64)) >= out_len.astype(np.int64)).all()
    assert int(out_off[-1]) <= cap and (out[int(out_off[-1]):] == 0xA5).all()
    assert st["n"] == sum(lengths) and st["out_len"] == int(out_off[-1])
    assert ((status == 0) | (out_len == 0)).all()
    return [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)], status.tolist(), st


def check(ctx, texts, w, t, coders=CODERS):
    for coder in coders:
        want_status, want = B.expected(texts, w, t, coder)
        got, status, _ = run(ctx, texts, w, t, coder)
        assert status == want_status, (coder, w, t)
        bad = [k for k in range(len(texts)) if got[k] != want[k]]
        assert not bad, (coder, w, t, bad[:5], len(bad))


def valid_after(ctx):
    """the context still works: a small batch through the facade, and the single call"""
    streams, status, _ = ctx.lzss_sw_compress_batch(KNOWN, 16, 3, T.CODER_GAMMA)
    assert status == [0, 0, 0] and streams == [M.encode(M.parse(x, 16, 3), "gamma", 16) for x in KNOWN]
    assert ctx.lzss_sw_compress(KNOWN[0], 16, 3, T.CODER_BIT)[0] == M.encode(M.parse(KNOWN[0], 16, 3), "bit", 16)


@pytest.mark.parametrize("w,t", WT)
@pytest.mark.parametrize("name", ("tile_edges", "three_tiles", "tiny", "empties", "only_empties"))
def test_borders_against_tiles(gpu_ctx, name, w, t):
    check(gpu_ctx, B.batch(name), w, t)


@pytest.mark.parametrize("w,t", WT)
def test_nothing_crosses_a_border(gpu_ctx, w, t):
    for name in ("copies", "lookahead"):
        check(gpu_ctx, B.batch(name), w, t)
    for coder in CODERS:
        got, status, _ = run(gpu_ctx, B.batch("copies"), w, t, coder)
        assert got[0] == got[1] == got[2] and status[0] == status[1] == status[2]       # no source in front of a text's start
    check(gpu_ctx, B.window_batch(w), w, t)                                             # w - 1, w, w + 1, 2w - 1, 2w, 2w + 1: L(p) per text
    if w > 1:
        check(gpu_ctx, B.window_batch(w) * 3, w, t)


@pytest.mark.parametrize("w,t", WT)
def test_bit_widths_are_text_local(gpu_ctx, w, t):
    texts = B.batch("widths")
    check(gpu_ctx, texts, w, t)
    if w == 16:
        _, status, st = run(gpu_ctx, texts, w, t, "bit")
        assert status == [0] * 40 and st["factors"] == sum(len(M.factors(x, w, t)) for x in texts)
        # matches throughout: factors whose distance takes every width from 3 bits (2 under threshold 0: no match of 3 bytes starts
        # at position 2 or 3) to 9 bits, while the global positions take up to 14
        for x in texts[:3]:
            pos = [p for p, _, _ in M.factors(x, w, t)]
            assert all(any(lo <= p < 2 * lo for p in pos) for lo in ((2,) if t == 0 else ()) + (4, 8, 16, 32, 64, 128, 256))


def test_truncation_is_per_text(gpu_ctx):
    texts = B.batch("truncation")
    for t in B.THRESHOLDS:
        got, status, _ = run(gpu_ctx, texts, 3, t, "bit")
        assert status == [0, B.ERR_UNSUPPORTED, 0] and got[1] == b""
        assert got[0] == M.encode(M.parse(texts[0], 3, t), "bit", 3) and got[2] == M.encode(M.parse(texts[2], 3, t), "bit", 3)
        for coder in ("gamma", "delta", "ascii"):
            got, status, _ = run(gpu_ctx, texts, 3, t, coder)
            assert status == [0, 0, 0] and got == [M.encode(M.parse(x, 3, t), coder, 3) for x in texts]
    streams, status, _ = gpu_ctx.lzss_sw_compress_batch(texts, 3, 3, T.CODER_BIT)        # the facade: b"" for the refused text
    assert status == [0, B.ERR_UNSUPPORTED, 0] and streams[1] == b"" and streams[0] and streams[2]
    with pytest.raises(T.TdcGpuError) as e:                                               # the single call's refusal of that text
        gpu_ctx.lzss_sw_compress(texts[1], 3, 3, T.CODER_BIT)
    assert e.value.status == B.ERR_UNSUPPORTED


@pytest.mark.parametrize("w,t", WT)
def test_count_one_and_count_zero(gpu_ctx, w, t):
    texts = B.batch("one")
    check(gpu_ctx, texts, w, t)
    for coder in CODERS:
        got, status, _ = run(gpu_ctx, texts, w, t, coder)
        try:
            single = (0, gpu_ctx.lzss_sw_compress(texts[0], w, t, B.CODER_ID[coder])[0])
        except T.TdcGpuError as e:
            single = (e.status, b"")
        assert (status[0], got[0]) == single
        out = np.full(16, 0xA5, dtype=np.uint8)
        out_off, out_len, status, st = gpu_ctx.lzss_sw_compress_batch_into(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), out, w, t,
                                                                          B.CODER_ID[coder])
        assert out_off.tolist() == [0] and len(out_len) == 0 and len(status) == 0 and (out == 0xA5).all() and st["out_len"] == 0
    assert gpu_ctx.lzss_sw_compress_batch([], w, t, T.CODER_BIT)[:2] == ([], [])


def test_refusals(gpu_ctx):
    texts = B.batch("tile_edges")
    lengths = [len(x) for x in texts]
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    for coder in CODERS:
        got, _, st = run(gpu_ctx, texts, 16, 3, coder)
        need = st["out_len"]
        for cap in (need - 1, 8, 0):                                                      # too small: the size, and nothing written
            out = np.full(max(cap, 1), 0xA5, dtype=np.uint8)[:cap]
            with pytest.raises(T.TdcGpuError) as e:
                gpu_ctx.lzss_sw_compress_batch_into(data, off, out, 16, 3, B.CODER_ID[coder])
            assert e.value.status == B.ERR_OOM and e.value.required == need and (out == 0xA5).all()
            valid_after(gpu_ctx)
        out = np.full(need, 0xA5, dtype=np.uint8)                                        # exactly enough
        out_off, out_len, _, _ = gpu_ctx.lzss_sw_compress_batch_into(data, off, out, 16, 3, B.CODER_ID[coder])
        assert [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)] == got
    out = np.full(64, 0xA5, dtype=np.uint8)
    small = np.zeros(64, dtype=np.uint8)
    for bad, want in (([0, 1 << 31, 0xFFFFFFFF], B.ERR_TOO_LARGE),                        # by the offsets alone, before any transfer
                      ([0, 1 << 33, 1 << 34], B.ERR_TOO_LARGE), ([0, 9, 8], B.ERR_ARG), ([1, 8, 9], B.ERR_ARG)):
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.lzss_sw_compress_batch_into(small, np.array(bad, dtype=np.uint64), out, 16, 3, T.CODER_BIT)
        assert e.value.status == want and (out == 0xA5).all()
        valid_after(gpu_ctx)
    for w, coder, want in ((0, T.CODER_BIT, B.ERR_ARG), (4097, T.CODER_BIT, B.ERR_UNSUPPORTED), (16, T.CODER_HUFF, B.ERR_UNSUPPORTED)):
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.lzss_sw_compress_batch_into(small, np.array([0, 8, 64], dtype=np.uint64), out, w, 3, coder)
        assert e.value.status == want and (out == 0xA5).all()
        valid_after(gpu_ctx)


@pytest.mark.parametrize("coder", CODERS)
def test_a_larger_batch_and_back(gpu_ctx, coder):
    texts = B.batch("english")
    want_status, want = B.expected(texts, 16, 3, coder)
    assert want_status == [0] * 512
    got, status, st = run(gpu_ctx, texts, 16, 3, coder)
    assert status == want_status
    bad = [k for k in range(512) if got[k] != want[k]]
    assert not bad, (bad[:5], len(bad))
    assert st["factors"] == sum(len(T.lzss_sw_factors(x, 16, 3)[0]) for x in texts)
    if coder != "ascii":
        back, status, st = gpu_ctx.lzss_sw_decompress_batch(got, B.CODER_ID[coder], 16)
        assert status == [0] * 512 and back == texts
        assert st["out_len"] == sum(len(x) for x in texts)
    z = T.LZSSSlidingWindowCompressor(gpu_ctx, coder, window=16, threshold=3, dec="gpu")       # the facade, on a part of the batch
    streams, status = z.compress_batch(texts[:40])
    assert streams == want[:40] and status == [0] * 40
    assert z.decompress_batch(streams) == (texts[:40], [0] * 40)
