"""GPU tests of the encode(huff) stage decoder (csrc/bytestages_decode.hip: code_exit_kernel, code_walk_kernel, tile_exits, dx_entries)
on crafted tables of up to 255 bits (pytest -m gpu).  The streams come from tests/huff_tables.py, which
tests/test_huff_tables.py checks on the CPU: every entry offset 0 .. longest - 1, deepest codes across tile, chunk and group borders,
codes that the 12-bit table rejects and that end behind bit 64, 128 and 192.  The host decoder is the specification: every comparison is
equality of (status, bytes) with it, and pipe_dev says that the device took the stage wherever the host accepts."""
import time

import numpy as np
import pytest

import tudocomp_amd as T
from tests import huff_tables as H
from tests.test_gpu_bytestage_decode import HUFF, MTF, RLE, host_stage

pytestmark = pytest.mark.gpu

TABLES = {t.name: t for t in H.tables()}
SWEEPABLE = [n for n, t in TABLES.items() if len(t.deepest) >= 2]
assert len(SWEEPABLE) == len(TABLES) - 1 and "chain(129)-sigma100" not in SWEEPABLE      # (its deepest codes are the ones sigma cuts off)
ONE_TILE_SHORT_OF_A_CHUNK = H.HD_CH - H.HD_T
ABOUT_600_TILES = 600 * H.HD_T + 777


@pytest.fixture(scope="module")
def dev():
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def dev_seg():
    with T.Context(0, options={"dec_parse": 2, "dec_seg": 1 << 20}) as ctx:
        yield ctx


def same_as_host(ctx, s, note):
    """the device's (status, bytes) of the stream equal the host decoder's; refused: nothing written.  Returns the host's pair."""
    want = host_stage(HUFF, s)
    out = np.full(len(want[1]) + 64 if want[0] == 0 else 1 << 16, 0xA5, dtype=np.uint8)
    try:
        n, st = ctx.pipeline_decompress_stats([HUFF], np.frombuffer(bytes(s), dtype=np.uint8), out[:len(out) - 64] if want[0] == 0 else out)
    except T.TdcGpuError as e:
        assert (e.status, None) == want, note
        assert bool((out == 0xA5).all()), note
        return want
    assert want[0] == 0 and n == len(want[1]) and out[:n].tobytes() == want[1], note
    assert bool((out[n:] == 0xA5).all()) and st["pipe_dev"] == 1, note
    return want


@pytest.mark.parametrize("name", SWEEPABLE)
def test_border_sweep(dev, name):
    t = TABLES[name]
    idx = H.border_sweep(t, max(2 * t.longest, 520))
    s = H.table_stream(t, idx)[0]
    assert same_as_host(dev, s, name) == (0, t.bytes_of(idx))


@pytest.mark.parametrize("name", list(TABLES))
def test_uniform_sequences(dev, dev_seg, name):
    t = TABLES[name]
    rng = np.random.default_rng(t.longest + 1)
    for nbits in (ONE_TILE_SHORT_OF_A_CHUNK, ABOUT_600_TILES):
        idx = H.uniform(t, nbits, rng)
        s, hb, total, _ = H.table_stream(t, idx)
        assert (total - hb + H.HD_T - 1) // H.HD_T == (nbits + H.HD_T - 1) // H.HD_T
        for ctx in (dev, dev_seg):
            assert same_as_host(ctx, s, (name, nbits)) == (0, t.bytes_of(idx))


@pytest.mark.parametrize("name", ["chain(255)", "bushy(200,32)"])
def test_stream_ends(dev, name):
    t = TABLES[name]
    L = t.longest
    rng = np.random.default_rng(L + 2)
    short = int(t.symbols[0])
    assert t.length[short] == 1
    # the last code is a deepest one and ends exactly at total, for every total % 8 (the terminator in the last byte or behind it)
    seen = set()
    base = H.uniform(t, 3 * H.HD_T, rng)
    for k in range(8):
        for which in (0, 1):
            idx = np.concatenate([np.full(k, short), base, t.deepest[which:which + 1]])
            s, hb, total, starts = H.table_stream(t, idx)
            assert starts[-1] + L == total
            seen.add(total % 8)
            assert same_as_host(dev, s, (name, k, which)) == (0, t.bytes_of(idx))
    assert seen == set(range(8))
    # the body is one deepest code
    for which in (0, 1):
        s, hb, total, _ = H.table_stream(t, t.deepest[which:which + 1])
        assert total - hb == L and same_as_host(dev, s, (name, "one code", which)) == (0, t.bytes_of(t.deepest[which:which + 1]))
    # the last tile holds fewer than L bits: the end of a deepest code, or short codes alone
    for r in (1, 5, L - 1):
        fill = np.full(3 * H.HD_T + r - L, short)
        for idx in (np.concatenate([fill, t.deepest[1:2]]), np.full(3 * H.HD_T + r, short)):
            s, hb, total, _ = H.table_stream(t, idx)
            assert total - hb == 3 * H.HD_T + r and same_as_host(dev, s, (name, "last tile", r)) == (0, t.bytes_of(idx))
    # cut at 64 byte lengths around tile and chunk borders: behind the end the host reads zeros, and 0^L is a code
    idx = H.uniform(t, 21 * H.HD_T, rng)
    s, hb, total, _ = H.table_stream(t, idx)
    cuts = [(hb + tile * H.HD_T) // 8 + d for tile in (3, 8, 16, 20) for d in range(-8, 8)]
    assert len(set(cuts)) == 64 and max(cuts) < len(s)
    status = {}
    for c in cuts:
        rc, got = same_as_host(dev, s[:c], (name, "cut", c))
        status[rc] = status.get(rc, 0) + 1
        if rc == 0:                                                               # whole codes in front of the cut are the ones put in
            whole = int(np.searchsorted(np.cumsum(t.length[idx]), 8 * (c - 2) - hb, side="right"))
            assert got[:whole] == t.bytes_of(idx[:whole])
    print("stream ends %s: statuses of the 64 cuts %s" % (name, sorted(status.items())))
    assert status.get(0, 0) >= 32


def test_refusals(dev):
    cases = H.refusal_streams(np.random.default_rng(5))
    assert len(cases) == 8
    for name, bad, good in cases:
        assert same_as_host(dev, bad, name) == (-2, None), name
        assert same_as_host(dev, good, name + ", then a good stream")[0] == 0


def fresh_call(stages, s, want):
    """the call on a context of its own that has done nothing before: its arena is what this one call reserves"""
    out = np.full(len(want), 0xA5, dtype=np.uint8)
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        t0 = time.perf_counter()
        n, st = ctx.pipeline_decompress_stats(stages, np.frombuffer(s, dtype=np.uint8), out)
        dt = time.perf_counter() - t0
    print("fresh context, %d stage(s): %d -> %d bytes, arena %d bytes (%.2f x the stream), %.1f ms wall, pipe_dev %s" %
          (len(stages), len(s), n, st["arena_bytes"], st["arena_bytes"] / len(s), dt * 1e3, bin(st["pipe_dev"])))
    assert n == len(want) and out.tobytes() == want
    return st


def test_arena_of_a_fresh_context_at_255_states():
    """chain(255) under about two bits a code: the tile tables of 255 states take about twice the stream, the output four times.  A
    first attempt reserves for an output of three times the stream; the second must hold the tables beside the output it has learnt."""
    t = H.chain(255)
    t = H.Table(t.name, t.numl, (np.arange(256) + 1) % 256)      # the code of l bits stands for byte l (the last deepest one for byte 0)
    rng = np.random.default_rng(255)
    idx = H.geometric(t, 33_500_000, rng)
    idx[idx >= 255] = 0
    s = H.table_stream(t, idx)[0]
    ranks = t.bytes_of(idx)
    assert 8_200_000 <= len(s) <= 8_600_000 and 2.3 <= len(ranks) / len(s) <= 8
    assert T.huff_decode_literals(s) == ranks
    st = fresh_call([HUFF], s, ranks)
    assert st["pipe_dev"] == 1
    # [rle, mtf, huff] around it, composed by hand: no rank is 0, so the text has no two equal neighbours and is its own rle stream
    text = T.mtf_decode(ranks)
    a = np.frombuffer(text, dtype=np.uint8)
    assert int(np.frombuffer(ranks, dtype=np.uint8).min()) >= 1 and bool((a[1:] != a[:-1]).all()) and T.rle_decode(text, 0) == text
    st = fresh_call([(RLE, 0), MTF, HUFF], s, text)
    assert st["pipe_dev"] == 0b111
