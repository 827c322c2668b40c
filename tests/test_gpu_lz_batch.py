"""GPU tests of lzw / lz78 over a batch of texts, parsed on the device (tdc_gpu_lzw_compress_batch, tdc_gpu_lz78_compress_batch,
tdc_gpu_lz_parse_batch; lz_batch.hip).  Truth comes from code that is not under test (tests/lz_batches.py): the model of lzw, the
oracle's lz78, the host parses.  Every batch compares the parse -- exact integers -- and every stream byte for byte, then decodes each
accepted stream with the host loop.  The batches are named for the fork of the parse kernel they reach."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batches as B

pytestmark = pytest.mark.gpu

KNOWN = [b"abcabcabcabc", b"", b"the cat sat on the mat, the cat sat"]


def run(ctx, algo, texts, coder):
    """(streams, statuses, stats) through the caller-owned entry point; what holds for every call is asserted here"""
    lengths = [len(x) for x in texts]
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    cid = B.LZW_CODERS[coder]
    cap = (T.lzw_batch_bound if algo == "lzw" else T.lz78_batch_bound)(lengths, cid)
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    into = ctx.lzw_compress_batch_into if algo == "lzw" else ctx.lz78_compress_batch_into
    out_off, out_len, status, st = into(data, off, out, cid)
    assert out_off[0] == 0 and (out_off % 8 == 0).all() and (np.diff(out_off.astype(np.int64)) >= out_len.astype(np.int64)).all()
    assert int(out_off[-1]) <= cap and (out[int(out_off[-1]):] == 0xA5).all()
    assert st["n"] == sum(lengths) and st["out_len"] == int(out_off[-1])
    assert ((status == 0) | (out_len == 0)).all()
    return [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)], status.tolist(), st


def check(ctx, texts):
    """the parse, the streams, the statuses, the factor count and the way back, for lzw (bit, gamma) and lz78"""
    texts = list(texts)
    count = len(texts)
    # lzw
    items, chars, status = ctx.lz_parse_batch(texts, True)
    assert chars is None and status == [0] * count
    bad = [k for k in range(count) if not np.array_equal(items[k], B.lzw_codes(texts[k]))]
    assert not bad, ("lzw parse", bad[:5], len(bad))
    for coder in ("bit", "gamma"):
        got, status, st = run(ctx, "lzw", texts, coder)
        assert status == [0] * count
        bad = [k for k in range(count) if got[k] != B.lzw_stream(texts[k], coder)]
        assert not bad, ("lzw", coder, bad[:5], len(bad))
        assert st["factors"] == sum(len(B.lzw_codes(x)) for x in texts)
        assert all(B.lzw_decode(got[k], coder) == texts[k] for k in range(count))
    # lz78
    want_status = [B.lz78_status(x) for x in texts]
    items, chars, status = ctx.lz_parse_batch(texts, False)
    assert status == want_status
    bad = [k for k in range(count) if not np.array_equal(items[k], B.lz78_pairs(texts[k])[0]) or chars[k] != B.lz78_pairs(texts[k])[1]]
    assert not bad, ("lz78 parse", bad[:5], len(bad))
    got, status, st = run(ctx, "lz78", texts, "gamma")
    assert status == want_status
    bad = [k for k in range(count) if got[k] != B.lz78_stream(texts[k])]
    assert not bad, ("lz78", bad[:5], len(bad))
    assert st["factors"] == sum(len(B.lz78_pairs(x)[0]) for x, s in zip(texts, want_status) if not s)
    assert all(B.lz78_decode(got[k]) == texts[k] for k in range(count) if not want_status[k])


def singles(ctx):
    """the single calls on the same context: still the model and the oracle"""
    for x in KNOWN + [B.batch("mixed")[5]]:
        assert ctx.lzw_compress(x, T.CODER_BIT)[0] == B.lzw_stream(x, "bit")
        assert ctx.lzw_compress(x, T.CODER_GAMMA)[0] == B.lzw_stream(x, "gamma")
        assert ctx.lz78_compress(x)[0] == B.lz78_stream(x)


@pytest.mark.parametrize("name", B.NAMES)
def test_batch(gpu_ctx, name):
    check(gpu_ctx, B.batch(name))


@pytest.mark.parametrize("fill", (0x01, 0xFF))
@pytest.mark.parametrize("name", B.NAMES)
def test_batch_on_a_filled_arena(gpu_ctx, name, fill):
    """nothing depends on what the arena held: the tables are zeroed by the call"""
    gpu_ctx.prim_arena_fill(fill)
    check(gpu_ctx, B.batch(name))


def test_known_answers(gpu_ctx):
    texts = [x for x, _ in B.kats("lzw")]
    items, _, status = gpu_ctx.lz_parse_batch(texts, True)
    assert status == [0] * len(texts) and [a.tolist() for a in items] == [list(want) for _, want in B.kats("lzw")]
    texts = [x for x, _ in B.kats("lz78")]
    items, chars, _ = gpu_ctx.lz_parse_batch(texts, False)
    assert [tuple(zip(a.tolist(), c)) for a, c in zip(items, chars)] == [want for _, want in B.kats("lz78")]


def test_a_refused_text_disturbs_no_neighbour(gpu_ctx):
    texts = list(B.batch("leftover_7f_80"))
    got, status, _ = run(gpu_ctx, "lz78", texts, "gamma")
    assert status == [0, 0, 0, B.ERR_UNSUPPORTED, 0, B.ERR_UNSUPPORTED, 0]
    assert got[3] == b"" and got[5] == b"" and got[2] == B.lz78_stream(texts[2]) and got[4] == B.lz78_stream(texts[4])
    with pytest.raises(T.TdcGpuError) as e:                                               # the single call's refusal of that text
        gpu_ctx.lz78_compress(texts[3])
    assert e.value.status == B.ERR_UNSUPPORTED
    assert gpu_ctx.lz78_compress(texts[1])[0] == got[1]                                   # 0x7F is taken
    streams, status = T.LZ78Compressor(gpu_ctx).compress_batch(texts)                     # the facade: b"" for the refused texts
    assert streams == got and status[3] == B.ERR_UNSUPPORTED


def test_a_text_beyond_the_cap_is_refused_alone(gpu_ctx):
    texts = [KNOWN[0], bytes(B.TEXT_CAP + 1), KNOWN[2]]
    for lzw in (True, False):
        items, _, status = gpu_ctx.lz_parse_batch(texts, lzw)
        assert status == [0, B.ERR_TOO_LARGE, 0] and len(items[1]) == 0
        assert np.array_equal(items[0], B.lzw_codes(KNOWN[0]) if lzw else B.lz78_pairs(KNOWN[0])[0])
        assert np.array_equal(items[2], B.lzw_codes(KNOWN[2]) if lzw else B.lz78_pairs(KNOWN[2])[0])
    for algo, coder in (("lzw", "bit"), ("lzw", "gamma"), ("lz78", "gamma")):
        got, status, st = run(gpu_ctx, algo, texts, coder)
        assert status == [0, B.ERR_TOO_LARGE, 0] and got[1] == b""
        assert [got[0], got[2]] == [B.lzw_stream(x, coder) if algo == "lzw" else B.lz78_stream(x) for x in (KNOWN[0], KNOWN[2])]


def test_identical_texts_yield_identical_streams(gpu_ctx):
    texts = list(B.batch("identical64"))
    for algo, coder in (("lzw", "bit"), ("lzw", "gamma"), ("lz78", "gamma")):
        got, status, _ = run(gpu_ctx, algo, texts, coder)
        assert status == [0] * 64 and len(set(got)) == 1                                  # no table leaks into the next


def test_few_hash_bits_same_ids():
    """every node in 16 homes: long probe runs, foreign words under a lane's own tag -- the ids rest on the key compare alone"""
    with T.Context(0) as ctx:
        ctx.set_option("lz_batch_hash_bits", 4)
        check(ctx, B.batch("mixed"))
        check(ctx, B.batch("capacity_sigma2")[:3])
        ctx.set_option("lz_batch_hash_bits", 1)
        check(ctx, B.batch("ends") + B.batch("lzw_kats"))
        ctx.set_option("lz_batch_hash_bits", 0)
        check(ctx, B.batch("mixed"))
        singles(ctx)


def test_out_cap_one_byte_short(gpu_ctx):
    texts = list(B.batch("mixed"))
    lengths = [len(x) for x in texts]
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    for algo, coder in (("lzw", "bit"), ("lzw", "gamma"), ("lz78", "gamma")):
        into = gpu_ctx.lzw_compress_batch_into if algo == "lzw" else gpu_ctx.lz78_compress_batch_into
        got, _, st = run(gpu_ctx, algo, texts, coder)
        need = st["out_len"]
        for cap in (need - 1, 8, 0):                                                      # too small: the size, and nothing written
            out = np.full(max(cap, 1), 0xA5, dtype=np.uint8)[:cap]
            with pytest.raises(T.TdcGpuError) as e:
                into(data, off, out, B.LZW_CODERS[coder])
            assert e.value.status == B.ERR_OOM and e.value.required == need and (out == 0xA5).all()
        out = np.full(need, 0xA5, dtype=np.uint8)                                        # exactly enough
        out_off, out_len, _, _ = into(data, off, out, B.LZW_CODERS[coder])
        assert int(out_off[-1]) == need
        assert [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)] == got
    singles(gpu_ctx)


def test_refusals_with_a_context(gpu_ctx):
    out, small = np.full(64, 0xA5, dtype=np.uint8), np.zeros(64, dtype=np.uint8)
    for into, bad_coder in ((gpu_ctx.lzw_compress_batch_into, T.CODER_DELTA), (gpu_ctx.lz78_compress_batch_into, T.CODER_BIT)):
        for bad, want in (([0, 1 << 31, 0xFFFFFFFF], B.ERR_TOO_LARGE), ([0, 1 << 33, 1 << 34], B.ERR_TOO_LARGE), ([0, 9, 8], -2), ([1, 8, 9], -2)):
            with pytest.raises(T.TdcGpuError) as e:
                into(small, np.array(bad, dtype=np.uint64), out, T.CODER_GAMMA)
            assert e.value.status == want and (out == 0xA5).all()
        with pytest.raises(T.TdcGpuError) as e:
            into(small, np.array([0, 8, 64], dtype=np.uint64), out, bad_coder)
        assert e.value.status == B.ERR_UNSUPPORTED and (out == 0xA5).all()
    singles(gpu_ctx)


def test_into_pinned_buffers(gpu_ctx):
    texts = list(B.batch("capacity_sigma256"))
    lengths = [len(x) for x in texts]
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    src = T.PinnedBuffer(sum(lengths))
    src.a[:] = np.frombuffer(b"".join(texts), dtype=np.uint8)
    for algo, coder in (("lzw", "bit"), ("lzw", "gamma"), ("lz78", "gamma")):
        cap = (T.lzw_batch_bound if algo == "lzw" else T.lz78_batch_bound)(lengths, B.LZW_CODERS[coder])
        dst = T.PinnedBuffer(cap)
        into = gpu_ctx.lzw_compress_batch_into if algo == "lzw" else gpu_ctx.lz78_compress_batch_into
        out_off, out_len, status, _ = into(src, off, dst, B.LZW_CODERS[coder])
        got = [dst.a[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)]
        want = [B.lzw_stream(x, coder) if algo == "lzw" else B.lz78_stream(x) for x in texts]
        assert got == want and status.tolist() == [B.lz78_status(x) if algo == "lz78" else 0 for x in texts]
        dst.free()
    src.free()


def test_single_calls_around_a_batch(gpu_ctx):
    singles(gpu_ctx)
    z = T.LZWCompressor(gpu_ctx, "gamma")
    streams, status = z.compress_batch(KNOWN)
    assert status == [0, 0, 0] and streams == [B.lzw_stream(x, "gamma") for x in KNOWN]
    assert z.last_stats["factors"] == sum(len(B.lzw_codes(x)) for x in KNOWN)
    assert [z.decompress(s) for s in streams] == KNOWN
    streams, status, _ = gpu_ctx.lzw_compress_batch(KNOWN)                                # the default coder: bit
    assert streams == [B.lzw_stream(x, "bit") for x in KNOWN]
    assert gpu_ctx.lzw_compress_batch([])[:2] == ([], []) and gpu_ctx.lz78_compress_batch([])[:2] == ([], [])
    singles(gpu_ctx)
