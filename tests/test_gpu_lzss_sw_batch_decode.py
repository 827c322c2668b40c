"""GPU tests of the batch decoder of lzss streams (tdc_gpu_lzss_sw_decompress_batch; lzss_sw_batch.hip, one wave per stream), coders bit,
gamma and delta: the streams that the host specification makes of the batches of tests/lzss_sw_batches.py back to their texts,
overlapping copies, damaged streams in one batch against the host loop's verdict on each alone (tdc_lzss_sw_decode), references that
would leave their own text, the sizes pass, and the context after every refusal."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import lzss_sw_batches as B
from tests import lzss_sw_damage as D
from tests.models import lzss_sw as M
from tests.models import lzss_sw_decode as MD

pytestmark = pytest.mark.gpu

CODERS = MD.CODERS
WT = [(w, t) for w in B.WINDOWS for t in B.THRESHOLDS]
KNOWN = [b"abcabcabcabc", b"", b"the cat sat on the mat, the cat sat"]


def pack(streams, align=8):
    """the streams in one blob, each at a multiple of `align`, 0xEE in between: (blob, s_off, s_len)"""
    s_off, pos = [], 0
    for s in streams:
        s_off.append(pos)
        pos += -(-len(s) // align) * align if align > 1 else len(s)
    blob = np.full(max(pos, 1), 0xEE, dtype=np.uint8)
    for o, s in zip(s_off, streams):
        blob[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return blob, np.array(s_off, dtype=np.uint64), np.array([len(s) for s in streams], dtype=np.uint64)


def decode(ctx, streams, coder, w, align=8):
    """(texts, statuses, stats) through the caller-owned entry point: the sizes pass with out = NULL, then the call"""
    blob, s_off, s_len = pack(streams, align)
    with pytest.raises(T.TdcGpuError) as e:
        ctx.lzss_sw_decompress_batch_into(blob, s_off, s_len, None, B.CODER_ID[coder], w)
    assert e.value.status == B.ERR_OOM
    need, sizes, verdicts = e.value.required, e.value.out_off.copy(), e.value.statuses.copy()
    assert int(sizes[-1]) == need and sizes[0] == 0
    out = np.full(need + 8, 0xA5, dtype=np.uint8)
    out_off, status, st = ctx.lzss_sw_decompress_batch_into(blob, s_off, s_len, out, B.CODER_ID[coder], w)
    assert (out_off == sizes).all() and (status == verdicts).all() and (out[need:] == 0xA5).all()
    assert st["n"] == int(s_len.sum()) and st["out_len"] == need
    return [out[int(a):int(b)].tobytes() for a, b in zip(out_off[:-1], out_off[1:])], status.tolist(), st


def host(stream, coder, w):
    try:
        return 0, T.lzss_sw_decode(stream, B.CODER_ID[coder], w)
    except T.TdcGpuError as e:
        return e.status, b""


def valid_after(ctx):
    for coder in CODERS:
        streams = [M.encode(M.parse(x, 16, 3), coder, 16) for x in KNOWN]
        assert ctx.lzss_sw_decompress_batch(streams, B.CODER_ID[coder], 16)[:2] == (KNOWN, [0, 0, 0])


def round_trip(ctx, texts, w, t, align=8):
    for coder in CODERS:
        want_status, streams = B.expected(texts, w, t, coder)                 # (b"" where bit would truncate: the empty stream)
        want = [x if s == 0 else b"" for x, s in zip(texts, want_status)]
        got, status, _ = decode(ctx, streams, coder, w, align)
        assert status == [0] * len(texts), (coder, w, t)
        bad = [k for k in range(len(texts)) if got[k] != want[k]]
        assert not bad, (coder, w, t, bad[:5], len(bad))


@pytest.mark.parametrize("w,t", WT)
@pytest.mark.parametrize("name", ("tile_edges", "three_tiles", "tiny", "empties", "only_empties", "copies", "lookahead", "widths", "truncation",
                                  "one"))
def test_round_trips(gpu_ctx, name, w, t):
    round_trip(gpu_ctx, B.batch(name), w, t)


@pytest.mark.parametrize("w", B.WINDOWS)
def test_round_trips_of_the_window_batches_at_any_alignment(gpu_ctx, w):
    round_trip(gpu_ctx, B.window_batch(w) * 3, w, 3, align=1)                 # streams back to back: every byte alignment
    round_trip(gpu_ctx, B.batch("lookahead") + B.batch("truncation"), w, 0, align=1)


def test_empty_streams(gpu_ctx):
    for coder in CODERS:
        good = M.encode(M.parse(KNOWN[0], 16, 3), coder, 16)
        got, status, _ = decode(gpu_ctx, [b"", good, b"", b"\x00", good, b""], coder, 16)     # no byte at all, and the terminator alone
        assert status == [0] * 6 and got == [b"", KNOWN[0], b"", b"", KNOWN[0], b""]
        got, status, _ = decode(gpu_ctx, [b"", b""], coder, 16)
        assert status == [0, 0] and got == [b"", b""]
        assert gpu_ctx.lzss_sw_decompress_batch([], B.CODER_ID[coder], 16)[:2] == ([], [])


@pytest.mark.parametrize("coder", CODERS)
def test_overlapping_copies(gpu_ctx, coder):
    """distance < length: a run, period 2 and period 3, parsed at windows 1, 2 and 3 (factors of up to 2w - 1 bytes at distances up to
    w), and hand-made copies far longer than a wave is wide.  coder=bit: the length field is as wide as the DECODER's window says, so
    the streams are written and read with 4096 there; the parse is the small window's."""
    fw = 4096
    texts = [b"a" * 500, b"ab" * 300, b"abc" * 200, b"a" * 7 + b"ab" * 9 + b"abc" * 11 + b"b" * 64, b"aab" * 100]
    streams, want, overlaps = [], [], 0
    for w in (1, 2, 3):
        for t in (1, 2):
            for x in texts:
                toks = M.parse(x, w, t)
                overlaps += sum(1 for p, s, j in toks if s is not None and p - s < j)
                streams.append(M.encode(toks, coder, fw))
                want.append(x)
    assert overlaps >= 400
    unit = bytes(range(33, 97))
    for dist, ln in ((1, 5000), (2, 777), (3, 1000), (63, 64 * 5), (64, 65), (64, 64 * 40 + 1), (5, 64), (64, 64)):
        toks = [(i, None, unit[i]) for i in range(64)] + [(64, 64 - dist, ln), (64 + ln, None, 33), (65 + ln, 64, ln)]
        streams.append(M.encode(toks, coder, 1 << 13))
        want.append(MD.text_of(toks))
    got, status, _ = decode(gpu_ctx, streams[:len(want) - 8], coder, fw)
    assert status == [0] * (len(want) - 8) and got == want[:-8]
    got, status, _ = decode(gpu_ctx, streams[-8:], coder, 1 << 13)
    assert status == [0] * 8 and got == want[-8:]


@pytest.mark.parametrize("coder", CODERS)
def test_damaged_streams_in_one_batch(gpu_ctx, coder):
    w = D.WINDOW
    damaged = D.damaged_streams(coder)
    good = damaged[-1][1]
    streams = []
    for _, s in damaged:                                                      # every damaged stream between two undamaged ones
        streams += [good, s]
    streams.append(good)
    verdicts = [host(s, coder, w) for s in streams]
    accepted = sum(1 for (rc, _), k in zip(verdicts, range(len(streams))) if k % 2 and rc == 0)
    assert accepted >= 10 and len(damaged) - accepted >= 10                   # both verdicts occur, as the host loop gives them
    for align in (8, 1):
        got, status, _ = decode(gpu_ctx, streams, coder, w, align)
        for k, (rc, text) in enumerate(verdicts):
            if k % 2 == 0:
                assert (status[k], got[k]) == (0, D.TEXT), k                  # the neighbours decode intact
            elif coder != "bit" and MD.over_cap(streams[k], coder, w) and status[k] == B.ERR_ARG:
                assert got[k] == b""                                          # a field above a device cap: the documented refusal
            else:
                assert (status[k], got[k]) == (rc, text), (damaged[k // 2][0], status[k], rc)
    valid_after(gpu_ctx)


@pytest.mark.parametrize("coder", CODERS)
def test_a_reference_out_of_its_own_text(gpu_ctx, coder):
    first = b"abcabcabcabcabcabc"
    good = M.encode(M.parse(first, 16, 3), coder, 16)
    at_start = M.encode([(0, -1, 3)], coder, 16)                              # the first token a factor: distance 1 at position 0
    beyond = M.encode([(0, None, 97), (1, None, 98), (2, -1, 2), (4, None, 99)], coder, 16)      # distance 3 at position 2
    inside = M.encode([(0, None, 97), (1, None, 98), (2, 0, 2), (4, None, 99)], coder, 16)       # distance 2 at position 2: allowed
    for bad in (at_start, beyond):
        assert host(bad, coder, 16)[0] == B.ERR_ARG
        got, status, _ = decode(gpu_ctx, [good, bad, good, inside], coder, 16, align=1)
        assert status == [0, B.ERR_ARG, 0, 0] and got == [first, b"", first, b"ababc"]
        valid_after(gpu_ctx)


def test_sizes_pass_and_short_buffers(gpu_ctx):
    texts = B.batch("widths")
    total = sum(len(x) for x in texts)
    for coder in CODERS:
        _, streams = B.expected(texts, 16, 3, coder)
        blob, s_off, s_len = pack(streams)
        with pytest.raises(T.TdcGpuError) as e:                               # out = NULL: the sizes alone
            gpu_ctx.lzss_sw_decompress_batch_into(blob, s_off, s_len, None, B.CODER_ID[coder], 16)
        assert e.value.status == B.ERR_OOM and e.value.required == total
        assert e.value.out_off.tolist() == [300 * k for k in range(41)] and e.value.statuses.tolist() == [0] * 40
        short = np.full(total - 1, 0xA5, dtype=np.uint8)                      # one byte short: the same, and nothing written
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.lzss_sw_decompress_batch_into(blob, s_off, s_len, short, B.CODER_ID[coder], 16)
        assert e.value.status == B.ERR_OOM and e.value.required == total and (short == 0xA5).all()
        assert e.value.out_off.tolist() == [300 * k for k in range(41)]
        valid_after(gpu_ctx)
        exact = np.full(total, 0xA5, dtype=np.uint8)
        out_off, status, st = gpu_ctx.lzss_sw_decompress_batch_into(blob, s_off, s_len, exact, B.CODER_ID[coder], 16)
        assert exact.tobytes() == b"".join(texts) and status.tolist() == [0] * 40
        assert st["factors"] == sum(MD.factor_tokens(x, coder, 16) for x in streams)


def test_refusals(gpu_ctx):
    good = M.encode(M.parse(KNOWN[0], 16, 3), "gamma", 16)
    blob, s_off, s_len = pack([good, good])
    out = np.full(64, 0xA5, dtype=np.uint8)
    for coder, w, want in ((T.CODER_ASCII, 16, B.ERR_UNSUPPORTED), (T.CODER_HUFF, 16, B.ERR_UNSUPPORTED), (99, 16, B.ERR_UNSUPPORTED),
                           (T.CODER_BIT, 0, B.ERR_ARG)):
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.lzss_sw_decompress_batch_into(blob, s_off, s_len, out, coder, w)
        assert e.value.status == want and (out == 0xA5).all()
        valid_after(gpu_ctx)
    assert gpu_ctx.lzss_sw_decompress_batch([good], T.CODER_GAMMA, 0)[:2] == ([KNOWN[0]], [0])      # only bit reads the window
    for coder in ("gamma", "delta"):
        # one stream above the format's limit: its own verdict, as the host loop's; the neighbours decode
        big = M.encode([(0, None, 97)] + [(1 + (i << 31), (i << 31), 1 << 31) for i in range(3)], coder, 16)
        small = M.encode(M.parse(KNOWN[2], 16, 3), coder, 16)
        assert host(big, coder, 16)[0] == B.ERR_TOO_LARGE
        got, status, _ = decode(gpu_ctx, [small, big, small], coder, 16)
        assert status == [0, B.ERR_TOO_LARGE, 0] and got == [KNOWN[2], b"", KNOWN[2]]
        # three streams of 2^31 bytes each: every one is fine, the batch is above 2^32 - 2 bytes
        half = M.encode([(0, None, 97), (1, 0, (1 << 31) - 1)], coder, 16)
        blob, s_off, s_len = pack([half, half, half])
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.lzss_sw_decompress_batch_into(blob, s_off, s_len, out, B.CODER_ID[coder], 16)
        assert e.value.status == B.ERR_TOO_LARGE and (out == 0xA5).all() and e.value.statuses.tolist() == [0, 0, 0]
        valid_after(gpu_ctx)
