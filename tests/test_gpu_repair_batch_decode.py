"""GPU tests of the batch decoder of repair streams (tdc_gpu_repair_decompress_batch; repair_batch_decode.hip: the grammars of all streams
as one forest) under bit, gamma and delta: the streams that the models and the host loop make of the batches of tests/lz_batches.py back
to their texts, foreign grammars on both sides of every index width, streams long enough to refill a wave's window, any alignment and
order, indices checked against their own stream, damaged streams in one batch against the specification's verdict on each alone, the
height cap, claims above the format's limit, the caller's buffer, the scratch arena's contents and size, more streams than the walks
have workgroups, and the context after every refusal."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batches as LB
from tests import many_texts as MT
from tests import repair_batch_decode_cases as C
from tests.models import repair as M

pytestmark = pytest.mark.gpu

CODERS = C.CODERS
ROUND_TRIPS = tuple(n for n in LB.NAMES if n != "one_mib")               # (the host loop's grammar of a MiB takes minutes: the batch compressor's, below)


def decode(ctx, streams, coder, align=8, order=None):
    """(texts, statuses, stats) through the caller-owned entry point: the sizes with out = NULL, then the call"""
    blob, s_off, s_len = C.pack(streams, align, order)
    with pytest.raises(T.TdcGpuError) as e:
        ctx.repair_decompress_batch_into(blob, s_off, s_len, None, C.CODER_ID[coder])
    assert e.value.status == C.ERR_OOM
    need, sizes, verdicts = e.value.required, e.value.out_off.copy(), e.value.statuses.copy()
    assert int(sizes[-1]) == need and sizes[0] == 0
    out = np.full(need + 8, 0xA5, dtype=np.uint8)
    out_off, status, st = ctx.repair_decompress_batch_into(blob, s_off, s_len, out, C.CODER_ID[coder])
    assert (out_off == sizes).all() and (status == verdicts).all() and (out[need:] == 0xA5).all()
    assert st["n"] == int(s_len.sum()) and st["out_len"] == need
    assert ctx._L.tdc_gpu_ctx_last_decode_on_device(ctx._h) == 1
    return [out[int(a):int(b)].tobytes() for a, b in zip(out_off[:-1], out_off[1:])], status.tolist(), st


def valid_after(ctx):
    for coder in CODERS:
        assert ctx.repair_decompress_batch(C.known(coder), C.CODER_ID[coder])[:2] == (list(C.KNOWN), [0, 0, 0])


def round_trip(ctx, texts, streams, coder, align=8, order=None):
    got, status, st = decode(ctx, streams, coder, align, order)
    assert status == [0] * len(texts)
    bad = [k for k in range(len(texts)) if got[k] != texts[k]]
    assert not bad, (coder, bad[:5], len(bad))
    return st


@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("name", ROUND_TRIPS)
def test_round_trips(gpu_ctx, name, coder):
    texts = list(LB.batch(name))
    if not texts:                                                             # count = 0: nothing to size
        blob, s_off, s_len = C.pack([])
        out_off, status, _ = gpu_ctx.repair_decompress_batch_into(blob, s_off, s_len, np.zeros(8, dtype=np.uint8), C.CODER_ID[coder])
        assert out_off.tolist() == [0] and len(status) == 0
        return
    streams = [C.stream_of(x, coder) for x in texts]
    st = round_trip(gpu_ctx, texts, streams, coder)
    assert st["rules"] == sum(len(M.parse(s, coder)[0]) for s in streams)


@pytest.mark.parametrize("coder", CODERS)
def test_rule_counts_at_every_width_border(gpu_ctx, coder):
    pairs = [C.foreign_stream(nr, coder) for nr in C.RULE_COUNTS]
    st = round_trip(gpu_ctx, [t for _, t in pairs], [s for s, _ in pairs], coder, align=1)
    assert st["rules"] == sum(C.RULE_COUNTS)


@pytest.mark.parametrize("coder", CODERS)
def test_window_refills(gpu_ctx, coder):
    """streams above 5 KiB -- literals, indices, an ordinary grammar -- at all four byte offsets from a word border: the refills of the
    wave's window fall at other bits of the tokens every time"""
    pairs = C.long_streams(coder)
    for lead in range(4):
        streams = ([b"\xEE" * lead] if lead else []) + [s for s, _ in pairs]      # (what the lead is read as does not matter)
        got, status, _ = decode(gpu_ctx, streams, coder, align=1)
        assert status[-len(pairs):] == [0] * len(pairs) and got[-len(pairs):] == [t for _, t in pairs], lead


@pytest.mark.parametrize("coder", CODERS)
def test_any_alignment_and_order(gpu_ctx, coder):
    texts = list(LB.batch("mixed") + LB.batch("ends") + LB.batch("one_two_bytes"))
    streams = [C.stream_of(x, coder) for x in texts]
    for align in (8, 4, 1):
        round_trip(gpu_ctx, texts, streams, coder, align)
    order = np.random.default_rng(3).permutation(len(streams)).tolist()
    round_trip(gpu_ctx, texts, streams, coder, 4, order)                       # 0xEE between the streams, the blob in another order
    round_trip(gpu_ctx, texts, streams, coder, 1, order)


@pytest.mark.parametrize("coder", CODERS)
def test_empty_and_minimal_streams(gpu_ctx, coder):
    good = C.known(coder)[2]
    streams = [good]
    for s, _ in C.minimal(coder):
        streams += [s, good]
    got, status, _ = decode(gpu_ctx, streams, coder, align=1)
    assert status == [0] + [v for _, want in C.minimal(coder) for v in (want, 0)]
    assert got == [C.KNOWN[2]] + [x for _ in C.minimal(coder) for x in (b"", C.KNOWN[2])]
    only = [s for s, _ in C.minimal(coder)]                                    # no good stream at all
    got, status, _ = decode(gpu_ctx, only, coder)
    assert got == [b""] * 4 and status == [want for _, want in C.minimal(coder)]


@pytest.mark.parametrize("coder", CODERS)
def test_own_stream(gpu_ctx, coder):
    streams, want_status, want = C.own_stream_batch(coder)
    got, status, _ = decode(gpu_ctx, streams, coder, align=1)
    assert (got, status) == (want, want_status)
    for k in (1, 3, 5):                                                        # each is refused alone
        assert decode(gpu_ctx, [streams[k]], coder)[:2] == ([b""], [C.ERR_ARG])
    valid_after(gpu_ctx)


@pytest.mark.parametrize("coder", CODERS)
def test_damaged_streams_in_one_batch(gpu_ctx, coder):
    streams, want_status, want, excepted = C.damaged(coder)
    assert len(streams) == C.DAMAGED[coder] + 2
    assert excepted <= C.EXCEPTED_MOST * len(streams) and (coder != "bit" or excepted == 0)
    got, status, _ = decode(gpu_ctx, streams, coder, align=1)
    bad = [k for k in range(len(streams)) if status[k] != want_status[k] or got[k] != want[k]]
    assert not bad, (coder, len(bad), bad[:8], [status[k] for k in bad[:8]], [want_status[k] for k in bad[:8]])
    valid_after(gpu_ctx)


@pytest.mark.parametrize("coder", CODERS)
def test_height_cap(coder):
    streams, texts, at_d, below = C.depth_batch(coder)
    with T.Context(0) as ctx:
        for cap, want in ((C.DEPTH, at_d), (C.DEPTH - 1, below)):
            ctx.set_option("repair_dec_rounds", cap)
            first = decode(ctx, streams, coder, align=1)[:2]
            assert first == ([b"" if v else x for v, x in zip(want, texts)], want), cap
            for b in (0x00, 0x01, 0xFF):                                       # the verdict is a function of the stream and the option alone
                assert ctx.prim_arena_fill(b)[1] > 0
                assert decode(ctx, streams, coder, align=1)[:2] == first, (cap, b)
        ctx.set_option("repair_dec_rounds", 1024)
        assert decode(ctx, streams, coder)[:2] == (texts, at_d)


@pytest.mark.parametrize("coder", CODERS)
def test_oversized_claims(coder):
    small = C.known(coder)[2]
    with T.Context(0) as ctx:                                                 # (its own context: the arena's size is part of the test)
        got, status, _ = decode(ctx, [small, C.doubling(30, [30, 30], coder), small], coder)
        assert status == [0, C.ERR_TOO_LARGE, 0] and got == [C.KNOWN[2], b"", C.KNOWN[2]]
        got, status, _ = decode(ctx, [small, C.bad_and_large(coder), small], coder)
        assert status == [0, C.ERR_ARG, 0] and got == [C.KNOWN[2], b"", C.KNOWN[2]]
        # three streams of 2^31 bytes each: every one is fine alone, the batch is above 2^32 - 2 bytes
        blob, s_off, s_len = C.pack([C.doubling(30, [30], coder)] * 3)
        out = np.full(4096, 0xA5, dtype=np.uint8)
        for buf in (None, out):
            with pytest.raises(T.TdcGpuError) as e:
                ctx.repair_decompress_batch_into(blob, s_off, s_len, buf, C.CODER_ID[coder])
            assert e.value.status == C.ERR_TOO_LARGE and e.value.statuses.tolist() == [0, 0, 0] and (out == 0xA5).all()
            assert e.value.out_off.tolist() == [0, 2**31, 2**32, 3 * 2**31]
        assert 0 < ctx.prim_arena_fill(None)[1] < 2**29                       # nothing text-sized was allocated on the way
        valid_after(ctx)


@pytest.mark.parametrize("coder", CODERS)
def test_callers_buffer(gpu_ctx, coder):
    texts = list(LB.batch("mixed"))
    streams = [C.stream_of(x, coder) for x in texts]
    blob, s_off, s_len = C.pack(streams)
    total = sum(len(x) for x in texts)
    out = np.full(total + 8, 0xA5, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:                                    # one byte short
        gpu_ctx.repair_decompress_batch_into(blob, s_off, s_len, out[:total - 1], C.CODER_ID[coder])
    assert e.value.status == C.ERR_OOM and e.value.required == total and (out == 0xA5).all()
    assert np.diff(e.value.out_off.astype(np.int64)).tolist() == [len(x) for x in texts] and e.value.statuses.tolist() == [0] * len(texts)
    out_off, status, _ = gpu_ctx.repair_decompress_batch_into(blob, s_off, s_len, out[:total], C.CODER_ID[coder])      # the exact size
    assert out[:total].tobytes() == b"".join(texts) and (out[total:] == 0xA5).all() and status.tolist() == [0] * len(texts)


@pytest.mark.parametrize("coder", CODERS)
def test_arena_moves_for_the_text(coder):
    """a fresh context sizes its arena by the stream bytes; a doubling stream of some 50 bytes that stands for 4 MiB makes it move
    behind the sizes, with the grammar alive (2 MiB still fits the slack)"""
    small = C.known(coder)[2]
    n = 2 << C.MOVE_TOP
    with T.Context(0) as ctx:
        assert decode(ctx, [small, C.doubling(C.MOVE_TOP - 1, [C.MOVE_TOP - 1], coder), small], coder)[0][1] == b"a" * (n // 2)
        before = ctx.prim_arena_fill(None)[1]
        got, status, st = decode(ctx, [small, C.doubling(C.MOVE_TOP, [C.MOVE_TOP], coder), small], coder, align=1)
        assert status == [0, 0, 0] and got[0] == got[2] == C.KNOWN[2] and got[1] == b"a" * n
        assert ctx.prim_arena_fill(None)[1] > before and st["arena_bytes"] > 5 * n
        valid_after(ctx)


def test_arena_moves_for_the_tokens():
    """gamma tokens of two bits each, the rule 0 as no encoder writes it: four tokens per stream byte, more than the arena a fresh context
    sizes by the stream bytes holds"""
    small = C.known("gamma")[2]
    n = 1 << 20
    with T.Context(0) as ctx:
        assert decode(ctx, [small], "gamma")[0] == [C.KNOWN[2]]
        before = ctx.prim_arena_fill(None)[1]
        stream = C.two_bit_tokens(n)
        got, status, st = decode(ctx, [small, stream, small], "gamma", align=1)
        assert status == [0, 0, 0] and got == [C.KNOWN[2], b"ab" * n, C.KNOWN[2]]
        # sized by the stream bytes alone the arena has 40 bytes per stream byte and 48 MiB; moved, it has 29 per token on top
        assert ctx.prim_arena_fill(None)[1] > max(before, (3 << 24) + 60 * len(stream)) and st["rules"] == 1 + 2 * len(M.parse(small, "gamma")[0])
        valid_after(ctx)


@pytest.mark.parametrize("coder", CODERS)
def test_scratch_independence(coder):
    texts = list(LB.batch("mixed") + LB.batch("one_two_bytes"))
    streams = [C.stream_of(x, coder) for x in texts] + [s for s, _ in C.minimal(coder)] + [C.foreign_stream(257, coder)[0]]
    with T.Context(0) as ctx:
        first = decode(ctx, streams, coder, align=1)[:2]
        assert first[0][:len(texts)] == texts and first[1][:len(texts)] == [0] * len(texts)
        for b in (0x00, 0x01, 0xFF):
            assert ctx.prim_arena_fill(b)[1] > 0
            assert decode(ctx, streams, coder, align=1)[:2] == first, b


# ---- more streams than the walks have workgroups -----------------------------------------------------------------------------------------
def many(ctx, coder, streams, want_status, want_texts, index):
    blob, s_off, s_len = MT.take(streams, index, align=8)
    want_len = want_texts.len[index]
    total = int(want_len.sum())
    out = np.full(total + 8, 0xA5, dtype=np.uint8)
    out_off, status, st = ctx.repair_decompress_batch_into(blob, s_off[:-1].astype(np.uint64), s_len.astype(np.uint64), out, C.CODER_ID[coder])
    bad = np.flatnonzero(np.asarray(status) != want_status[index])
    assert len(bad) == 0, (coder, len(bad), bad[:8].tolist())
    assert out_off[0] == 0 and (np.diff(out_off.astype(np.int64)) == want_len).all()
    assert (out[total:] == 0xA5).all() and st["n"] == int(s_len.sum()) and st["out_len"] == total
    bad = MT.differing(out, out_off[:-1], want_len, want_texts, index)
    assert len(bad) == 0, (coder, len(bad), bad[:8].tolist())
    return st


@pytest.mark.parametrize("coder", ("bit", "gamma"))
def test_three_trips(gpu_ctx, coder):
    """2 * 2^16 + 4099 streams of the pool of tests/many_texts.py -- what the batch compressor makes of its texts --: a wave of the walks
    takes a second and a third stream"""
    index = MT.trips3()
    st = many(gpu_ctx, coder, MT.repair_streams(coder), np.zeros(len(MT.pool()), dtype=np.int32), MT.text_pool(), index)
    assert st["rules"] == int(MT.repair_rules().len[index].sum())


@pytest.mark.parametrize("coder", ("bit", "gamma"))
@pytest.mark.parametrize("count", (2049, 4097))
def test_every_fourth_damaged(gpu_ctx, coder, count):
    good = MT.repair_streams(coder)
    npool = len(MT.pool())
    extra = [(s, v, x) for s, v, x in zip(*C.damaged(coder)[:3]) if v][:7]
    streams = MT.Ragged([good[j].tobytes() for j in range(npool)] + [s for s, _, _ in extra])
    status = np.array([0] * npool + [v for _, v, _ in extra], dtype=np.int32)
    texts = MT.Ragged(MT.texts() + [x for _, _, x in extra])
    index = MT.border(count).copy()
    index[3::4] = npool + np.arange(len(index[3::4])) % len(extra)
    many(gpu_ctx, coder, streams, status, texts, index)


# ---- against the batch compressor and the facades -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS)
@pytest.mark.parametrize("name", ("mixed", "one_mib"))
def test_against_the_batch_compressor(gpu_ctx, name, coder):
    """repair_compress_batch -> repair_decompress_batch, through the caller-owned entry point and through the facade.  The MiB is
    compressed with max_rules = 256: one workgroup builds its grammar, a walk over the text per rule, and without the cap that takes
    minutes; the decoder then meets a start sequence of several hundred thousand symbols."""
    texts = list(LB.batch(name))
    z = T.RePairCompressor(gpu_ctx, coder=coder, max_rules=256 if name == "one_mib" else 0)
    streams, status = z.compress_batch(texts)
    assert status == [0] * len(texts)
    round_trip(gpu_ctx, texts, streams, coder)
    assert z.decompress_batch(streams) == (texts, [0] * len(texts))
    assert z.last_stats["out_len"] == sum(len(x) for x in texts)


def test_other_coders_are_refused(gpu_ctx):
    blob, s_off, s_len = C.pack(C.known("bit"))
    out = np.full(64, 0xA5, dtype=np.uint8)
    for coder in (T.CODER_HUFF, T.CODER_ASCII, 99):
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.repair_decompress_batch_into(blob, s_off, s_len, out, coder)
        assert e.value.status == C.ERR_UNSUPPORTED and (out == 0xA5).all()
    with pytest.raises(T.TdcGpuError) as e:
        T.RePairCompressor(gpu_ctx, coder="ascii").decompress_batch([b"0:"])
    assert e.value.status == C.ERR_UNSUPPORTED
    valid_after(gpu_ctx)
