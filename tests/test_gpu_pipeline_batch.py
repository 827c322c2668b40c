"""GPU tests of chains over a batch of texts (pytest -m gpu; DESIGN.md section 5.3 "Batches"): tdc_gpu_pipeline_compress_batch for chains
of bwt, rle, mtf and encode(huff).  The truth is never the code under test: stream k is compared with ctx.pipeline_compress(stages,
text k), the single call that tests/test_gpu_bytestages.py holds against the model and the reference's vectors; short texts also with
tests/models/bwtzip.py, and every accepted stream is decoded back to its text by the host decoders and ctx.bwt_decompress."""
import os
import re

import numpy as np
import pytest

import tudocomp_amd as T
from tests import bwt_batches as B
from tests import many_texts as MT
from tests.models import bwtzip as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BWT, RLE, MTF, HUFF = T.STAGE_BWT, T.STAGE_RLE, T.STAGE_MTF, T.STAGE_HUFF
CHAINS = {
    "rle": [(RLE, 0)], "rle200": [(RLE, 200)], "mtf": [MTF], "huff": [HUFF], "rle:mtf": [(RLE, 0), MTF],
    "rle:mtf:huff": [(RLE, 0), MTF, HUFF], "bwtzip": [BWT, (RLE, 0), MTF, HUFF],
}
BWTZIP, BYTES3 = CHAINS["bwtzip"], CHAINS["rle:mtf:huff"]
CAP = 1 << 20
ERR_ARG, ERR_NO_SENTINEL, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -3, -4, -5, -6

_single = {}


def single(ctx, name, text):
    """(status, stream, pipe_len) of the single call on one text, computed once.  (The empty view under a leading bwt is the C call's
    TDC_GPU_ERR_NO_SENTINEL; Context.pipeline_compress passes no pointer for it, which is refused as a NULL argument before that.)"""
    key = (name, text)
    if text == b"" and CHAINS[name][0] == BWT:
        return (ERR_NO_SENTINEL, b"", None)
    if key not in _single:
        try:
            out, st = ctx.pipeline_compress(CHAINS[name], text)
            _single[key] = (0, out, [int(x) for x in st["pipe_len"]])
        except T.TdcGpuError as e:
            _single[key] = (e.status, b"", None)
    return _single[key]


def decode(ctx, name, stream):
    """the text of a stream, stage by stage backwards through the host decoders; a leading bwt through the device.  None: the
    Huffman decoder refuses the stream -- the reference's header holds the alphabet size in eight bits, so a stage input with all 256
    byte values has no decodable stream, from the single call either"""
    x = stream
    for stage in reversed(CHAINS[name]):
        kind, param = (stage, 0) if isinstance(stage, int) else stage
        if kind == HUFF:
            try:
                x = T.huff_decode_literals(x)
            except T.TdcGpuError:
                return None
        elif kind == MTF:
            x = T.mtf_decode(x)
        elif kind == RLE:
            x = T.rle_decode(x, param)
        else:
            x = ctx.bwt_decompress(x)[0]
    return x


def model(name, text):
    """the model's stream for the chains that end before huff (None: no model)"""
    x = text
    for stage in CHAINS[name]:
        kind, param = (stage, 0) if isinstance(stage, int) else stage
        if kind == RLE:
            x = M.rle_encode(x, param)
        elif kind == MTF:
            x = M.mtf_encode(x)
        else:
            return None
    return bytes(x)


def check_batch(ctx, name, texts, cap_status=True):
    """the batch call on `texts` against the single call on each, the model and the decoders; returns (streams, statuses, stats)"""
    streams, status, st = ctx.pipeline_compress_batch(CHAINS[name], texts)
    assert len(streams) == len(status) == len(texts)
    for k, text in enumerate(texts):
        if cap_status and len(text) > CAP:
            assert status[k] == ERR_TOO_LARGE and streams[k] == b"", (name, k)
            continue
        rc, want, _ = single(ctx, name, text)
        assert status[k] == rc, (name, k, len(text), status[k], rc)
        assert streams[k] == want, (name, k, len(text), len(streams[k]), len(want))
        if rc == 0:
            if len(text) < 2000 and model(name, text) is not None:
                assert streams[k] == model(name, text), (name, k)
            if len(text) > 1 or CHAINS[name][0] != BWT:              # (the transform of the view "\0" inverts to nothing)
                back = decode(ctx, name, streams[k])
                assert back == text or (back is None and len(set(text)) >= 255), (name, k, len(text))
    return streams, status, st


# ---- 1: by length, per nature ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nature", B.NATURES)
@pytest.mark.parametrize("name", list(CHAINS))
def test_by_length(gpu_ctx, name, nature):
    texts = [B.text(nature, n) for n in B.LENGTHS]
    if CHAINS[name][0] != BWT:
        texts += [t[:-1] for t in texts] + [b""]
    _, status, _ = check_batch(gpu_ctx, name, texts)
    assert status == [0] * len(texts)


# ---- 2: borders of the kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", (262143, 262144, 262145))
@pytest.mark.parametrize("name", ("rle:mtf:huff", "bwtzip", "mtf", "rle200"))
def test_kernel_borders(gpu_ctx, name, big):
    """text starts on, one before and one behind a border of RLE_TILE = HUFF_TILE = 4096 and of MTF_CHUNK = 1024 in the concatenation,
    one text around MTF_TILE, and one text at many offsets mod 16"""
    x = B.text("english", 5003, 9)
    texts = []
    for filler in (4095, 4096, 4097, 1023, 1025, 7, 3, 1):
        texts += [B.text("random2", filler, filler), x]
    for m, r in ((4096, 4095), (4096, 0), (4096, 1), (1024, 1023), (1024, 0), (1024, 1)):      # a filler that puts x at r mod m
        pos = sum(len(t) for t in texts)
        texts += [B.text("random2", (r - pos) % m or m, m + r), x]
    texts += [B.text("english", big, 3), x, B.text("ab", 4097), x]
    starts = np.cumsum([0] + [len(t) for t in texts])[:-1]
    assert {int(s) % 4096 for s in starts} >= {0, 1, 4095} and {int(s) % 1024 for s in starts} >= {0, 1, 1023}
    assert len({int(s) % 16 for s, t in zip(starts, texts) if t is x}) >= 6
    streams, status, _ = check_batch(gpu_ctx, name, texts)
    assert status == [0] * len(texts)
    copies = {streams[k] for k, t in enumerate(texts) if t is x}
    assert len(copies) == 1


# ---- 3: nothing crosses a border ---------------------------------------------------------------------------------------------------
def test_rle_runs_end_with_their_text(gpu_ctx):
    texts = [b"aaa", b"aaa", b"a", b"\xff\xff", b"\xff", b"", b"aa"]
    for name in ("rle", "rle200"):
        streams, status, _ = check_batch(gpu_ctx, name, texts)
        assert status == [0] * 7
        assert streams == [M.rle_encode(t, CHAINS[name][0][1]) for t in texts]
    streams, _, _ = gpu_ctx.pipeline_compress_batch(CHAINS["rle"], texts)
    assert streams[0] == streams[1] == b"aa\x01" and streams[2] == b"a" and streams[6] == b"aa\x00"
    assert streams[3] == b"\xff\xff\x00" and streams[4] == b"\xff" and streams[5] == b""      # no `c vbyte(offset)` for a text's first byte


def test_mtf_starts_every_text_from_the_identity(gpu_ctx):
    texts = [b"zzzz", b"z", b"\x00", b"az"]
    streams, status, _ = check_batch(gpu_ctx, "mtf", texts)
    assert status == [0] * 4
    assert streams == [b"\x7a\x00\x00\x00", b"\x7a", b"\x00", b"\x61\x7a"]


def test_huff_tables_are_per_text(gpu_ctx):
    e1, e2 = B.text("english", 3001, 4)[:-1], B.text("english", 5000, 5)[:-1]
    low, high = bytes(range(1, 40)) * 9, bytes(range(200, 256)) * 5
    texts = [e1, b"q" * 700, e2, low, high, b"q", b""]
    for name in ("huff", "rle:mtf:huff"):
        streams, status, _ = check_batch(gpu_ctx, name, texts)
        assert status == [0] * len(texts)
    streams, _, _ = gpu_ctx.pipeline_compress_batch(CHAINS["huff"], texts)
    assert len(streams[1]) == 701                                    # sigma = 1: the flag bit, eight raw bits per byte, the terminator
    for k in (3, 4):                                                 # the header lists the text's own symbols and no other
        table = gpu_ctx.pipeline_compress(CHAINS["huff"], texts[k])[0]
        assert streams[k] == table and T.huff_decode_literals(streams[k]) == texts[k]
    assert len(streams[3]) < len(low) and len(streams[4]) < len(high)


# ---- 4: refusals stand alone ---------------------------------------------------------------------------------------------------------
def refusal_texts():
    good = [B.text("english", 3000, 6), B.text("fibonacci", 257), B.text("escapes", 4097)]
    big = B.text("ab", CAP + 1)
    return [good[0], b"ab\x00cd\x00", good[1], b"abc", b"", big, good[2], b"\x00"]


def test_refusals_stand_alone(gpu_ctx):
    ctx = gpu_ctx
    texts = refusal_texts()
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    off = T._offsets([len(t) for t in texts])
    for name, want in (("bwtzip", [0, ERR_ARG, 0, ERR_NO_SENTINEL, ERR_NO_SENTINEL, ERR_TOO_LARGE, 0, 0]),
                       ("rle:mtf:huff", [0, 0, 0, 0, 0, ERR_TOO_LARGE, 0, 0])):
        streams, status, _ = check_batch(ctx, name, texts)
        assert status == want, (name, status)
        for k in range(len(texts)):
            if k != 5:
                assert status[k] == single(ctx, name, texts[k])[0]
        with pytest.raises(T.TdcGpuError) as e:
            ctx.pipeline_compress_batch_into(CHAINS[name], data, off, None)
        required = e.value.required
        out = np.full(required + 64, 0xA5, dtype=np.uint8)
        out_off, out_len, st, _ = ctx.pipeline_compress_batch_into(CHAINS[name], data, off, out)
        assert st.tolist() == want and int(out_off[-1]) == required
        assert all(int(o) % 8 == 0 for o in out_off)
        assert required == sum(-(-int(x) // 8) * 8 for x in out_len)  # the ranges, each rounded up to 8, are all that is used
        assert (out[required:] == 0xA5).all()
        for k in range(len(texts)):
            assert out[int(out_off[k]):int(out_off[k]) + int(out_len[k])].tobytes() == streams[k]
            assert (int(out_len[k]) == 0) == (want[k] != 0)


# ---- 5: the sizes pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("bwtzip", "rle:mtf:huff", "rle", "mtf"))
def test_sizes_pass(gpu_ctx, name):
    ctx = gpu_ctx
    texts = [t for t in refusal_texts() if len(t) <= CAP] + [B.text("thue_morse", 65537)]
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    off = T._offsets([len(t) for t in texts])
    full = np.full(1 << 20, 0xA5, dtype=np.uint8)
    out_off, out_len, status, _ = ctx.pipeline_compress_batch_into(CHAINS[name], data, off, full)
    required = int(out_off[-1])
    assert 0 < required < full.size
    for out in (None, np.full(required - 1, 0xA5, dtype=np.uint8)):
        with pytest.raises(T.TdcGpuError) as e:
            ctx.pipeline_compress_batch_into(CHAINS[name], data, off, out)
        assert e.value.status == ERR_OOM and e.value.required == required
        o2, l2, s2 = e.value.sizes
        assert np.array_equal(o2, out_off) and np.array_equal(l2, out_len) and np.array_equal(s2, status)
        assert out is None or (out == 0xA5).all()
    exact = np.full(required, 0xA5, dtype=np.uint8)
    o3, l3, s3, _ = ctx.pipeline_compress_batch_into(CHAINS[name], data, off, exact)
    assert np.array_equal(o3, out_off) and np.array_equal(l3, out_len) and np.array_equal(s3, status)
    assert np.array_equal(exact, full[:required])
    # count = 0
    o0, l0, s0, st0 = ctx.pipeline_compress_batch_into(CHAINS[name], np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), full)
    assert o0.tolist() == [0] and len(l0) == 0 and len(s0) == 0
    assert ctx.pipeline_compress_batch(CHAINS[name], []) == ([], [], st0)


# ---- 6: stats --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("bwtzip", "rle:mtf:huff", "rle:mtf"))
def test_stats(name):
    texts = refusal_texts() + [B.text("english", 65537), B.text("a_run", 4096)]
    with T.Context(0) as ctx:
        streams, status, st = ctx.pipeline_compress_batch(CHAINS[name], texts)
        k = len(CHAINS[name])
        assert st["pipe_stages"] == k and st["n"] == sum(len(t) for t in texts)
        assert st["out_len"] == sum(-(-len(s) // 8) * 8 for s in streams) and st["arena_bytes"] > 0 and st["ms_total"] > 0
        want = [0] * k
        for t, rc in zip(texts, status):
            if rc == 0:
                want = [a + b for a, b in zip(want, single(ctx, name, t)[2])]
        assert [int(x) for x in st["pipe_len"]] == want
        assert all(x == 0 for x in st["pipe_ms"])
        ctx.set_option("pipe_log", 1)
        streams2, status2, st2 = ctx.pipeline_compress_batch(CHAINS[name], texts)
        ctx.set_option("pipe_log", 0)
        assert streams2 == streams and status2 == status
        assert all(x >= 0 for x in st2["pipe_ms"]) and sum(st2["pipe_ms"]) > 0
        assert [int(x) for x in st2["pipe_len"]] == want
        for threads in (1, 3, 16):                                   # the table build on any number of host threads: the same bytes
            ctx.set_option("pipe_batch_threads", threads)
            assert ctx.pipeline_compress_batch(CHAINS[name], texts)[:2] == (streams, status)


# ---- 7: arena state --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("bwtzip", "rle:mtf:huff"))
def test_arena_state(name):
    texts = refusal_texts() + [b"aaa", b"aaa", b"a", b"\xff\xff", b"\xff", b"", b"aa", b"zzzz", b"z", b"\x00", b"az", b"q" * 700,
                               B.text("english", 70001, 8), bytes(range(200, 256)) * 5 + b"\x00"]
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    off = T._offsets([len(t) for t in texts])
    with T.Context(0) as ctx:
        first = ctx.pipeline_compress_batch(CHAINS[name], texts)[:2]
        for k, t in enumerate(texts):
            if len(t) <= CAP:
                assert (first[1][k], first[0][k]) == single(ctx, name, t)[:2]
        out = np.zeros(sum(-(-len(s) // 8) * 8 for s in first[0]), dtype=np.uint8)
        ref = None
        for fill in (0x00, 0x01, 0xFF):
            where = ctx.prim_arena_fill(fill)
            assert where[1] > 0
            out_off, out_len, status, _ = ctx.pipeline_compress_batch_into(CHAINS[name], data, off, out)
            assert ctx.prim_arena_fill() == where                    # (a call that reallocated would prove nothing)
            got = (out_off.tolist(), out_len.tolist(), status.tolist(),
                   [out[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(out_off[:-1], out_len)])
            assert list(got[2:]) == [first[1], first[0]], fill
            ref = ref or got
            assert got == ref, fill


# ---- 8: more tiles than a grid -----------------------------------------------------------------------------------------------------------
def test_more_tiles_than_workgroups(gpu_ctx):
    """Every kernel of bytestages_batch.hip that gives a workgroup to a tile or a thread to a text is launched with at most
    BSB_MAX_BLOCKS = 2^16 workgroups and goes on with `+= gridDim.x` (bytestages_batch.hpp).  A batch of 2^16 + 2^13 + 1 short texts has
    more tiles than that -- every text that is not empty is a tile of rle, a chunk of mtf and a tile of encode(huff) --, so workgroups
    take a second tile; the per-text kernels take 256 texts per workgroup and stay below the cap at any count a test can run."""
    ctx = gpu_ctx
    src = open(os.path.join(ROOT, "tudocomp_amd", "csrc", "bytestages_batch.hpp")).read()
    cap = 1 << int(re.search(r"constexpr u32 BSB_MAX_BLOCKS = 1u << (\d+);", src).group(1))
    assert cap == MT.CAP16
    count = cap + cap // 8 + 1
    index = MT.border(count)
    texts = MT.texts_of(index)
    assert sum(1 for t in texts if t) > cap + 256
    want = MT.Ragged([single(ctx, "rle:mtf:huff", t)[1] for t in MT.texts()])
    assert all(single(ctx, "rle:mtf:huff", t)[0] == 0 for t in MT.texts() if len(t) <= 40)
    data, off, _ = MT.take(MT.text_pool(), index)
    with pytest.raises(T.TdcGpuError) as e:
        ctx.pipeline_compress_batch_into(BYTES3, data, off.astype(np.uint64), None)
    out = np.empty(e.value.required, dtype=np.uint8)
    out_off, out_len, status, _ = ctx.pipeline_compress_batch_into(BYTES3, data, off.astype(np.uint64), out)
    assert not status.any()
    bad = MT.differing(out, out_off[:-1], out_len, want, index)
    assert len(bad) == 0, bad[:10]


# ---- 9: facades --------------------------------------------------------------------------------------------------------------------------
def test_facades(gpu_ctx):
    ctx = gpu_ctx
    datas = [b"", b"\x00", b"\xff", b"a\x00b\xff\xfe\x00\x00", T.gen_english(5000, 3).tobytes(), bytes(range(256)) * 4,
             b"\xff" * 300 + b"\x00" * 300, b"abracadabra"]
    for spec in ("bwt:rle:mtf:encode(huff)", "rle:mtf:encode(huff)", "mtf:rle(offset=3)"):
        comp = T.ChainCompressor(ctx, spec)
        streams, status = comp.compress_batch(datas)
        assert status == [0] * len(datas)
        assert streams == [comp.compress(d) for d in datas], spec
        assert [comp.decompress(s) for s in streams] == datas, spec
        assert comp.last_stats["pipe_stages"] == len(comp.stages)
    for comp in (T.RunLengthEncoder(ctx, 5), T.MTFCompressor(ctx), T.LiteralEncoder(ctx, coder="huff")):
        streams, status = comp.compress_batch(datas)
        assert status == [0] * len(datas) and streams == [comp.compress(d) for d in datas]
    with pytest.raises(T.TdcGpuError) as e:
        T.LiteralEncoder(ctx, coder="sle").compress_batch(datas)
    assert e.value.status == ERR_UNSUPPORTED
