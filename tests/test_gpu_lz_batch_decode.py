"""GPU tests of the batch decoders of lzw and lz78 streams (tdc_gpu_lzw_decompress_batch, tdc_gpu_lz78_decompress_batch;
lz_batch_decode.hip: the items of all streams as one forest), lzw under bit and gamma, lz78 under gamma: the streams that the models
and the oracle make of the batches of tests/lz_batches.py back to their texts, any alignment, items counted from their own stream's
first one, damaged streams in one batch against the specification's verdict on each alone, claims above the format's limit, the
caller's buffer, the scratch arena's contents, and the context after every refusal."""
import hashlib

import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batch_decode_cases as C
from tests import lz_batches as LB
from tests import lzw_damage

pytestmark = pytest.mark.gpu

ALGOS = C.ALGOS


def into(ctx, algo):
    return ctx.lz78_decompress_batch_into if algo == "lz78" else ctx.lzw_decompress_batch_into


def decode(ctx, streams, algo, align=8):
    """(texts, statuses, stats) through the caller-owned entry point: the sizes with out = NULL, then the call"""
    blob, s_off, s_len = C.pack(streams, align)
    with pytest.raises(T.TdcGpuError) as e:
        into(ctx, algo)(blob, s_off, s_len, None, C.CODER_ID[algo])
    assert e.value.status == C.ERR_OOM
    need, sizes, verdicts = e.value.required, e.value.out_off.copy(), e.value.statuses.copy()
    assert int(sizes[-1]) == need and sizes[0] == 0
    out = np.full(need + 8, 0xA5, dtype=np.uint8)
    out_off, status, st = into(ctx, algo)(blob, s_off, s_len, out, C.CODER_ID[algo])
    assert (out_off == sizes).all() and (status == verdicts).all() and (out[need:] == 0xA5).all()
    assert st["n"] == int(s_len.sum()) and st["out_len"] == need
    assert ctx._L.tdc_gpu_ctx_last_decode_on_device(ctx._h) == 1
    return [out[int(a):int(b)].tobytes() for a, b in zip(out_off[:-1], out_off[1:])], status.tolist(), st


def valid_after(ctx):
    for algo in ALGOS:
        streams, want = C.expected(C.KNOWN, algo)
        got = ctx.lz78_decompress_batch(streams) if algo == "lz78" else ctx.lzw_decompress_batch(streams, C.CODER_ID[algo])
        assert got[:2] == (list(C.KNOWN), [0, 0, 0]) == (want, [0, 0, 0])


def round_trip(ctx, texts, algo, align=8):
    streams, want = C.expected(texts, algo)
    if not streams:                                                           # count = 0: nothing to size
        blob, s_off, s_len = C.pack(streams)
        out_off, status, _ = into(ctx, algo)(blob, s_off, s_len, np.zeros(8, dtype=np.uint8), C.CODER_ID[algo])
        assert out_off.tolist() == [0] and len(status) == 0
        return None
    got, status, st = decode(ctx, streams, algo, align)
    assert status == [0] * len(texts)
    bad = [k for k in range(len(texts)) if got[k] != want[k]]
    assert not bad, (algo, bad[:5], len(bad))
    return st


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", LB.NAMES)
def test_round_trips(gpu_ctx, name, algo):
    texts = LB.batch(name)
    st = round_trip(gpu_ctx, texts, algo)
    if st is not None:
        assert st["factors"] == C.items_of(texts, algo)


@pytest.mark.parametrize("algo", ALGOS)
def test_any_alignment(gpu_ctx, algo):
    texts = LB.batch("mixed") + LB.batch("ends") + LB.batch("one_two_bytes")
    round_trip(gpu_ctx, texts, algo, align=1)                                 # streams back to back: every byte alignment
    round_trip(gpu_ctx, texts, algo, align=4)                                 # 0xEE between the streams


@pytest.mark.parametrize("algo", ALGOS)
def test_empty_streams(gpu_ctx, algo):
    (good,), _ = C.expected([C.KNOWN[0]], algo)
    got, status, _ = decode(gpu_ctx, [b"", good, b"", b"\x00", good, b""], algo)          # no byte at all, and the terminator alone
    assert status == [0] * 6 and got == [b"", C.KNOWN[0], b"", b"", C.KNOWN[0], b""]
    got, status, st = decode(gpu_ctx, [b"", b"\x00"], algo)
    assert status == [0, 0] and got == [b"", b""] and st["factors"] == 0
    got, status, _ = decode(gpu_ctx, [good, b"\x06", b"\x07", good], algo, align=1)        # a cut-off terminator
    assert status == [0, C.ERR_ARG, C.ERR_ARG, 0] and got == [C.KNOWN[0], b"", b"", C.KNOWN[0]]


@pytest.mark.parametrize("algo", ALGOS)
def test_items_are_counted_from_their_own_stream(gpu_ctx, algo):
    for streams, statuses, texts in C.own_stream_cases(algo):
        for align in (8, 1):
            got, status, _ = decode(gpu_ctx, streams, algo, align)
            assert status == statuses and got == texts
        valid_after(gpu_ctx)


@pytest.mark.parametrize("coder", ("bit", "gamma"))
def test_damaged_lzw_streams_in_one_batch(gpu_ctx, coder):
    algo = "lzw-" + coder
    data, base = lzw_damage.base_stream(coder)
    streams = [base] + lzw_damage.damaged_streams(coder) + [base]
    verdicts = [C.host(s, algo) for s in streams]
    assert len(streams) == 152 and verdicts[0] == verdicts[-1] == (0, data)
    got, status, _ = decode(gpu_ctx, streams, algo, align=1)
    for k, (rc, text) in enumerate(verdicts):                                 # every stream, the two undamaged ones among them
        assert (status[k], got[k]) == (rc, text), k
    valid_after(gpu_ctx)


def test_damaged_lz78_streams_in_one_batch(gpu_ctx):
    data, base = C.lz78_base()
    streams = [base] + list(C.lz78_damaged()) + [base]
    verdicts = [[0, len(data), hashlib.sha256(data).hexdigest()]] + C.lz78_damage_verdicts() + [[0, len(data), hashlib.sha256(data).hexdigest()]]
    assert len(streams) == len(verdicts) == 152
    got, status, _ = decode(gpu_ctx, streams, "lz78", align=1)
    assert got[0] == got[-1] == data
    for k, want in enumerate(verdicts):
        assert [status[k], len(got[k]), hashlib.sha256(got[k]).hexdigest()] == want, k
    valid_after(gpu_ctx)


@pytest.mark.parametrize("algo", ALGOS)
def test_oversized_claims(algo):
    (small,), _ = C.expected([C.KNOWN[2]], algo)
    with T.Context(0) as ctx:                                                 # (its own context: the arena's size is part of the test)
        got, status, _ = decode(ctx, [small, C.claim_stream(algo, C.OVER), small], algo)
        assert status == [0, C.ERR_TOO_LARGE, 0] and got == [C.KNOWN[2], b"", C.KNOWN[2]]
        # three streams of 2^31 bytes each: every one is fine alone, the batch is above 2^32 - 2 bytes
        half = C.claim_stream(algo, C.HALF)
        blob, s_off, s_len = C.pack([half, half, half])
        out = np.full(64, 0xA5, dtype=np.uint8)
        for buf in (None, out):                                               # the sizes alone, and the call
            with pytest.raises(T.TdcGpuError) as e:
                into(ctx, algo)(blob, s_off, s_len, buf, C.CODER_ID[algo])
            assert e.value.status == C.ERR_TOO_LARGE and e.value.statuses.tolist() == [0, 0, 0] and (out == 0xA5).all()
            assert e.value.out_off.tolist() == [k * (2**31 + 2**15) for k in range(4)]
        assert 0 < ctx.prim_arena_fill(None)[1] < 2**29                       # nothing text-sized was allocated on the way
        valid_after(ctx)


@pytest.mark.parametrize("algo", ALGOS)
def test_callers_buffer(gpu_ctx, algo):
    texts = LB.batch("mixed")
    streams, want = C.expected(texts, algo)
    total = sum(len(x) for x in want)
    offs = np.cumsum([0] + [len(x) for x in want]).tolist()
    blob, s_off, s_len = C.pack(streams)
    short = np.full(total - 1, 0xA5, dtype=np.uint8)                          # one byte short: the sizes, and nothing written
    with pytest.raises(T.TdcGpuError) as e:
        into(gpu_ctx, algo)(blob, s_off, s_len, short, C.CODER_ID[algo])
    assert e.value.status == C.ERR_OOM and e.value.required == total and (short == 0xA5).all()
    assert e.value.out_off.tolist() == offs and e.value.statuses.tolist() == [0] * len(texts)
    valid_after(gpu_ctx)
    guarded = np.full(total + 8, 0xA5, dtype=np.uint8)                        # the exact size, 8 guard bytes behind it
    out_off, status, st = into(gpu_ctx, algo)(blob, s_off, s_len, guarded[:total], C.CODER_ID[algo])
    assert guarded[:total].tobytes() == b"".join(want) and (guarded[total:] == 0xA5).all()
    assert out_off.tolist() == offs and status.tolist() == [0] * len(texts)
    assert (st["n"], st["out_len"], st["factors"]) == (sum(len(s) for s in streams), total, C.items_of(texts, algo))


@pytest.mark.parametrize("algo", ALGOS)
def test_scratch_independence(algo):
    texts = LB.batch("mixed") + LB.batch("depth_2211") + LB.batch("ends")
    streams, want = C.expected(texts, algo)
    with T.Context(0) as ctx:
        first = decode(ctx, streams, algo, align=1)[:2]
        assert first == (want, [0] * len(texts))
        for b in (0x00, 0x01, 0xFF):
            assert ctx.prim_arena_fill(b)[1] > 0
            assert decode(ctx, streams, algo, align=1)[:2] == first, b


@pytest.mark.parametrize("algo", ALGOS)
def test_arena_moves_for_the_text(algo):
    """a fresh context sizes its arena by the stream bytes; 12 000 items that claim 72 MB of text make it move behind the sizes, with the
    factor list alive"""
    (small,), _ = C.expected([C.KNOWN[2]], algo)
    with T.Context(0) as ctx:
        got, status, st = decode(ctx, [small, C.claim_stream(algo, C.DEEP), small], algo, align=1)
        assert status == [0, 0, 0] and got[0] == got[2] == C.KNOWN[2]
        assert got[1] == b"a" * (C.DEEP * (C.DEEP + 1) // 2) and st["arena_bytes"] > 5 * len(got[1])
        valid_after(ctx)


def test_arena_moves_for_the_items():
    """gamma codes of one bit each: eight items per stream byte, more than the arena a fresh context sizes by the stream bytes holds"""
    (small,), _ = C.expected([C.KNOWN[2]], "lzw-gamma")
    with T.Context(0) as ctx:
        got, status, st = decode(ctx, [small, C.zeros_stream(), small], "lzw-gamma", align=1)
        assert status == [0, 0, 0] and got == [C.KNOWN[2], bytes(C.ZEROS), C.KNOWN[2]]
        assert st["factors"] == C.ZEROS + C.items_of([C.KNOWN[2]] * 2, "lzw-gamma") and st["arena_bytes"] > 36 * C.ZEROS
        valid_after(ctx)


def test_other_coders(gpu_ctx):
    for algo in ALGOS:
        streams, _ = C.expected(C.KNOWN, algo)
        blob, s_off, s_len = C.pack(streams)
        out = np.full(64, 0xA5, dtype=np.uint8)
        others = (T.CODER_HUFF, T.CODER_ASCII, T.CODER_DELTA, 99) + ((T.CODER_BIT,) if algo == "lz78" else ())
        for coder in others:
            with pytest.raises(T.TdcGpuError) as e:
                into(gpu_ctx, algo)(blob, s_off, s_len, out, coder)
            assert e.value.status == C.ERR_UNSUPPORTED and (out == 0xA5).all()
            valid_after(gpu_ctx)


@pytest.mark.parametrize("name", ("mixed", "one_mib"))
def test_batch_against_the_batch_compressor(gpu_ctx, name):
    texts = list(LB.batch(name))
    for coder in (T.CODER_BIT, T.CODER_GAMMA):
        streams, status, _ = gpu_ctx.lzw_compress_batch(texts, coder)
        assert status == [0] * len(texts)
        assert gpu_ctx.lzw_decompress_batch(streams, coder)[:2] == (texts, [0] * len(texts))
    streams, status, _ = gpu_ctx.lz78_compress_batch(texts)
    want = [b"" if s else x for x, s in zip(texts, status)]
    assert gpu_ctx.lz78_decompress_batch(streams)[:2] == (want, [0] * len(texts))
    z = T.LZWCompressor(gpu_ctx, coder="gamma")
    assert z.decompress_batch(z.compress_batch(texts)[0]) == (texts, [0] * len(texts)) and z.last_stats["out_len"] == sum(len(x) for x in texts)
    z = T.LZ78Compressor(gpu_ctx)
    assert z.decompress_batch(z.compress_batch(texts)[0]) == (want, [0] * len(texts)) and z.last_stats["out_len"] == sum(len(x) for x in want)
