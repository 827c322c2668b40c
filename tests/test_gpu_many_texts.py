"""GPU tests of the batch calls on more texts than their kernels have workgroups (tests/many_texts.py): 2 * 2^16 + 4099 texts, so that a
workgroup of lz_batch.hip, lz_batch_decode.hip, lzss_sw_batch.hip and of repair's coder kernels takes a second and a third text, and
repair's round kernel (2048 workgroups) some sixty; and counts at the caps, one above, and one above twice the cap.  What a workgroup
leaves behind for its next text -- a verdict, a flag, LDS words, a missing barrier -- shows as a wrong byte or a wrong status of one text
among a hundred thousand, so EVERY text of every batch is compared with what its pool entry must yield, with numpy.  The truth is
computed once per pool entry by code that is not under test; tests/test_many_texts_cli.py checks it, and the counts against the caps in
the sources, on the CPU."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batch_decode_cases as LC
from tests import lz_batches as LB
from tests import lzss_sw_batches as SB
from tests import many_texts as MT
from tests import repair_batches as RB

pytestmark = pytest.mark.gpu

LZ = (("lzw", "bit"), ("lzw", "gamma"), ("lz78", "gamma"))
LZ_ALGOS = LC.ALGOS                                                     # lzw-bit, lzw-gamma, lz78


def none_differs(what, flat, starts, lens, want, index):
    bad = MT.differing(flat, starts, lens, want, index)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), [MT.pool()[index[k]][0] if index[k] < len(MT.pool()) else "damaged" for k in bad[:8]])


def same_statuses(what, got, want):
    bad = np.flatnonzero(np.asarray(got) != want)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), want[bad[:8]].tolist())


def compressed(what, call, bound, index, want_status, want_streams):
    """one compress call on the texts of `index` through the caller-owned entry point: every status, every stream byte for byte, and the
    placement -- stream k at the next multiple of 8 behind stream k - 1, nothing behind the last.  Returns the stats."""
    data, off, lens = MT.take(MT.text_pool(), index)
    cap = bound(lens)
    assert cap > 0
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    out_off, out_len, status, st = call(data, off.astype(np.uint64), out)
    want = want_status[index]
    same_statuses(what, status, want)
    assert (out_len[want != 0] == 0).all()                                # a refused text: the empty stream
    slots = (out_len.astype(np.int64) + 7) // 8 * 8
    assert out_off[0] == 0 and (np.diff(out_off.astype(np.int64)) == slots).all(), what       # 8-aligned and increasing, no gap
    assert int(out_off[-1]) <= cap and (out[int(out_off[-1]):] == 0xA5).all(), what
    assert st["n"] == int(lens.sum()) and st["out_len"] == int(out_off[-1])
    none_differs(what, out, out_off[:-1], out_len, want_streams, index)
    return st


def decompressed(what, call, streams, want_status, want_texts, index):
    """one decompress call on the streams of `index`, each at a multiple of 8: every status -- the single decoder's verdict on the stream
    alone --, every text byte for byte, and the placement: text k right behind text k - 1.  Returns the stats."""
    blob, s_off, s_len = MT.take(streams, index, align=8)
    want_len = want_texts.len[index]
    total = int(want_len.sum())
    out = np.full(total + 8, 0xA5, dtype=np.uint8)
    out_off, status, st = call(blob, s_off[:-1].astype(np.uint64), s_len.astype(np.uint64), out)
    same_statuses(what, status, want_status[index])
    assert out_off[0] == 0 and (np.diff(out_off.astype(np.int64)) == want_len).all(), what
    assert (out[total:] == 0xA5).all() and st["n"] == int(s_len.sum()) and st["out_len"] == total
    none_differs(what, out, out_off[:-1], want_len, want_texts, index)
    return st


# ---- lzw and lz78 --------------------------------------------------------------------------------------------------------------------------
def lz_compress(ctx, algo, coder, index):
    cid = LB.LZW_CODERS[coder]
    if algo == "lzw":
        st = compressed(("lzw", coder), lambda d, o, out: ctx.lzw_compress_batch_into(d, o, out, cid), lambda n: T.lzw_batch_bound(n, cid), index,
                        np.zeros(len(MT.pool()), dtype=np.int32), MT.lzw_streams(coder))
        assert st["factors"] == int(MT.lzw_items().len[index].sum())
    else:
        status = MT.lz78_statuses()
        st = compressed("lz78", lambda d, o, out: ctx.lz78_compress_batch_into(d, o, out, cid), lambda n: T.lz78_batch_bound(n, cid), index,
                        status, MT.lz78_streams())
        assert st["factors"] == int(np.where(status == 0, MT.lz78_ids().len, 0)[index].sum())     # the items of the accepted texts


def lz_parse(ctx, lzw, index):
    items, chars, status = ctx.lz_parse_batch(MT.texts_of(index), lzw)
    same_statuses(("parse", lzw), status, (np.zeros(len(MT.pool()), dtype=np.int32) if lzw else MT.lz78_statuses())[index])
    none_differs(("items", lzw), *MT.flatten(items, np.uint32), MT.lzw_items() if lzw else MT.lz78_ids(), index)
    if lzw:
        assert chars is None
    else:
        none_differs("chars", *MT.flatten(chars, np.uint8), MT.lz78_chars(), index)


def lz_decompress(ctx, algo, streams, status, texts, index):
    into = ctx.lz78_decompress_batch_into if algo == "lz78" else ctx.lzw_decompress_batch_into
    return decompressed(algo, lambda b, so, sl, out: into(b, so, sl, out, LC.CODER_ID[algo]), streams, status, texts, index)


@pytest.mark.parametrize("algo,coder", LZ)
def test_lz_compress_three_trips(gpu_ctx, algo, coder):
    lz_compress(gpu_ctx, algo, coder, MT.trips3())


@pytest.mark.parametrize("lzw", (True, False))
def test_lz_parse_three_trips(gpu_ctx, lzw):
    lz_parse(gpu_ctx, lzw, MT.trips3())


@pytest.mark.parametrize("count", MT.BORDERS16)
def test_lz_compress_at_the_cap(gpu_ctx, count):
    for algo, coder in LZ:
        lz_compress(gpu_ctx, algo, coder, MT.border(count))


@pytest.mark.parametrize("count", MT.BORDERS16)
def test_lz_parse_at_the_cap(gpu_ctx, count):
    lz_parse(gpu_ctx, True, MT.border(count))
    lz_parse(gpu_ctx, False, MT.border(count))


@pytest.mark.parametrize("algo", LZ_ALGOS)
def test_lz_decompress_three_trips(gpu_ctx, algo):
    """damaged streams between valid ones, and valid ones between damaged ones, on one workgroup's three trips"""
    lz_decompress(gpu_ctx, algo, *MT.decode_batch(algo))


@pytest.mark.parametrize("count", MT.BORDERS16)
def test_lz_decompress_at_the_cap(gpu_ctx, count):
    for algo in LZ_ALGOS:
        streams, texts = MT.valid_streams(algo)
        st = lz_decompress(gpu_ctx, algo, streams, np.zeros(len(MT.pool()), dtype=np.int32), MT.Ragged(texts), MT.border(count))
        items = MT.lz78_ids().len if algo == "lz78" else MT.lzw_items().len          # (no short text is one that lz78 refuses)
        assert st["factors"] == int(items[MT.border(count)].sum())


# ---- lzss ----------------------------------------------------------------------------------------------------------------------------------
def lzss_compress(ctx, coder, index):
    cid = SB.CODER_ID[coder]
    status, streams = MT.lzss_truth(coder)
    compressed(("lzss", coder), lambda d, o, out: ctx.lzss_sw_compress_batch_into(d, o, out, MT.WINDOW, MT.THRESHOLD, cid),
               lambda n: T.lzss_sw_batch_bound(n, MT.WINDOW, cid), index, status, streams)


def lzss_decompress(ctx, coder, streams, status, texts, index):
    cid = SB.CODER_ID[coder]
    decompressed(("lzss", coder), lambda b, so, sl, out: ctx.lzss_sw_decompress_batch_into(b, so, sl, out, cid, MT.WINDOW), streams, status, texts,
                 index)


@pytest.mark.parametrize("coder", MT.LZSS_CODERS)
def test_lzss_compress_three_trips(gpu_ctx, coder):
    """(tile-based: the slots, the scans and the terminators above 2^16 texts)"""
    lzss_compress(gpu_ctx, coder, MT.trips3())


@pytest.mark.parametrize("coder", MT.LZSS_CODERS)
def test_lzss_decompress_three_trips(gpu_ctx, coder):
    """one wave per stream; damaged streams between valid ones and the other way round on one wave's three trips"""
    lzss_decompress(gpu_ctx, coder, *MT.decode_batch("lzss-" + coder))


@pytest.mark.parametrize("count", MT.BORDERS16)
def test_lzss_at_the_cap(gpu_ctx, count):
    for coder in MT.LZSS_CODERS:
        lzss_compress(gpu_ctx, coder, MT.border(count))
        streams, texts = MT.valid_streams("lzss-" + coder)
        lzss_decompress(gpu_ctx, coder, streams, np.zeros(len(MT.pool()), dtype=np.int32), MT.Ragged(texts), MT.border(count))


# ---- repair --------------------------------------------------------------------------------------------------------------------------------
def repair_grammars(ctx, index, max_rules=0):
    rules, start, status = ctx.repair_grammar_batch(MT.texts_of(index), max_rules)
    same_statuses("grammar", status, np.zeros(len(index), dtype=np.int32))
    none_differs(("rules", max_rules), *MT.flatten(rules, np.uint64), MT.repair_rules(max_rules), index)
    none_differs(("start", max_rules), *MT.flatten(start, np.uint32), MT.repair_starts(max_rules), index)


def repair_compress(ctx, coder, index, max_rules=0):
    cid = RB.CID[coder]
    st = compressed(("repair", coder, max_rules), lambda d, o, out: ctx.repair_compress_batch_into(d, o, out, max_rules, cid),
                    lambda n: T.repair_batch_bound(n, cid), index, np.zeros(len(MT.pool()), dtype=np.int32), MT.repair_streams(coder, max_rules))
    assert st["rules"] == int(MT.repair_rules(max_rules).len[index].sum())
    assert st["replaced"] == int((MT.text_pool().len - MT.repair_starts(max_rules).len)[index].sum())
    return st


def test_repair_grammars_three_trips(gpu_ctx):
    repair_grammars(gpu_ctx, MT.trips3())


@pytest.mark.parametrize("coder", ("bit", "gamma"))
def test_repair_compress_three_trips(gpu_ctx, coder):
    st = repair_compress(gpu_ctx, coder, MT.trips3())
    assert st["tie_rounds"] > 0


@pytest.mark.parametrize("count", MT.REPAIR_BORDERS)
def test_repair_at_the_round_kernels_cap(gpu_ctx, count):
    """run, no repeated pair, English and the tie text at every length: what a workgroup's previous text left is not what the next needs"""
    index = MT.repair_border(count)
    repair_grammars(gpu_ctx, index)
    for coder in MT.REPAIR_CODERS:
        st = repair_compress(gpu_ctx, coder, index)
        assert st["tie_rounds"] > 0


def test_repair_one_round_per_launch():
    """repair_batch_rounds = 1: a launch performs one round per text and leaves the state, so every workgroup is relaunched over its
    three or four texts as often as the longest grammar has rules"""
    index = MT.repair_border(MT.REPAIR_BORDERS[3])
    with T.Context(0) as ctx:
        ctx.set_option("repair_batch_rounds", 1)
        repair_grammars(ctx, index)
        st = repair_compress(ctx, "bit", index)
        most = int(MT.repair_rules().len[index].max())
        assert most >= 4                                                  # a^40: aa, AA, BB, CC
        assert st["len_rounds"] >= most and st["tie_rounds"] > 0


def test_repair_max_rules_1(gpu_ctx):
    """the cap of one rule: a text is finished after its first round, next to texts that never had one"""
    repair_grammars(gpu_ctx, MT.trips3(), 1)
    repair_compress(gpu_ctx, "delta", MT.trips3(), 1)


# ---- the arena -----------------------------------------------------------------------------------------------------------------------------
def test_three_trips_on_a_filled_arena(gpu_ctx):
    """nothing depends on what the arena held, for the texts of a later trip either (the session's context: the tests above have made
    the arena as large as these calls need it)"""
    gpu_ctx.prim_arena_fill(0xFF)
    lz_compress(gpu_ctx, "lz78", "gamma", MT.trips3())
    gpu_ctx.prim_arena_fill(0xFF)
    lz_decompress(gpu_ctx, "lzw-bit", *MT.decode_batch("lzw-bit"))
    gpu_ctx.prim_arena_fill(0xFF)
    lzss_decompress(gpu_ctx, "gamma", *MT.decode_batch("lzss-gamma"))
    gpu_ctx.prim_arena_fill(0xFF)
    repair_compress(gpu_ctx, "bit", MT.trips3())
