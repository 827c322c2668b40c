"""GPU tests of encode(sle) as a pipeline stage, both directions (pytest -m gpu).

Encoder: tdc_gpu_pipeline_compress([(STAGE_SLE, k)]) equals the model (tests/models/sle_literals.py, pinned to the oracle by
tests/test_sle_literals_model.py) byte for byte.  The fill scan works in tiles of 2048 positions and 2048 is a multiple of neither 3
nor 7, so on b"abc" * N and on a period-7 text fired k-mers straddle tile borders; the random alphabets take every class-code branch and
both eta rules.  Decoder: with dec_parse = 2 the device decodes every such stream to the input and reports the stage in pipe_dev, with
dec_parse = 0 the host loop gives the same bytes; on damaged streams the device gives the host loop's outcome."""
import hashlib
import random

import numpy as np
import pytest

import tudocomp_amd as T
from tests.models import bwtzip as BZ
from tests.models import sle_literals as M

pytestmark = pytest.mark.gpu

SLE = T.STAGE_SLE
KMERS = (1, 2, 3, 4, 7)
BIG = (1 << 20) + 3
ALPHABETS = (2, 8, 9, 17, 33, 65, 129, 256)
NAMES = ["one-byte", "abc", "period7", "english", "dna"] + ["random%d" % d for d in ALPHABETS]


def lengths(k):
    return sorted({0, 1, k - 1, k, k + 1, 2047, 2048, 2049, 4095, 4096, 4097, BIG})


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(5)
    out = {"one-byte": b"z" * BIG, "abc": (b"abc" * (BIG // 3 + 1))[:BIG], "period7": (b"abcdefg" * (BIG // 7 + 1))[:BIG],
           "english": T.gen_english(BIG, 42).tobytes(), "dna": T.gen_dna(BIG, 7).tobytes()}
    for d in ALPHABETS:
        out["random%d" % d] = (rng.integers(0, d, BIG, dtype=np.int64) * (256 // d)).astype(np.uint8).tobytes()
    return out


@pytest.fixture(scope="module")
def dev():
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def hostctx():
    with T.Context(0, options={"dec_parse": 0}) as ctx:
        yield ctx


def decode(ctx, stages, stream, cap):
    """(status, bytes, pipe_dev) of tdc_gpu_pipeline_decompress_stats"""
    out = np.empty(max(cap, 1), dtype=np.uint8)
    try:
        n, st = ctx.pipeline_decompress_stats(stages, stream, out)
    except T.TdcGpuError as e:
        return e.status, None, None
    return 0, out[:n].tobytes(), st["pipe_dev"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("k", KMERS)
def test_encoder_equals_the_model_and_both_decoders_invert_it(dev, hostctx, texts, k, name):
    for n in lengths(k):
        data = texts[name][:n]
        want = M.encode(data, k)
        got, st = dev.pipeline_compress([(SLE, k)], data)
        assert got == want, (k, name, n)
        assert st["pipe_len"][0] == len(want) and len(got) <= T.pipeline_bound([(SLE, k)], n)
        assert decode(dev, [(SLE, k)], got, n) == (0, data, 1), (k, name, n)
        assert decode(hostctx, [(SLE, k)], got, n) == (0, data, 0), (k, name, n)


def test_kmer_zero_means_three(dev):
    data = T.gen_english(5000, 1).tobytes()
    got, _ = dev.pipeline_compress([SLE], data)
    assert got == M.encode(data, 3) and dev.pipeline_decompress([SLE], got) == data


@pytest.mark.parametrize("k", (1, 3, 7))
def test_damaged_streams_device_gives_the_host_loops_outcome(dev, hostctx, k):
    rng = random.Random(k)
    gen = np.random.default_rng(k)
    short = M.encode(b"abracadabra" * 9, k)
    assert len(short) < 400
    cases = [(short, [short[:i] for i in range(len(short))])]                  # truncated at every byte of a short stream
    for d in (17, 65, 129):
        data = gen.integers(0, d, 3000, dtype=np.int64).astype(np.uint8).tobytes()
        z = M.encode(data, k)
        table, _, hb = M.parse_ranking(M.open_stream(z), k)
        flips = [rng.randrange(hb) for _ in range(40)] + [rng.randrange(hb, len(z) * 8) for _ in range(40)]      # header, payload
        cases.append((z, [z[:i >> 3] + bytes([z[i >> 3] ^ (0x80 >> (i & 7))]) + z[(i >> 3) + 1:] for i in flips]))
    seen = set()
    for base, damaged in cases:
        cap = 8 * 7 * len(base)                                                # (a one-bit code may stand for seven bytes)
        for s in damaged:
            want = decode(hostctx, [(SLE, k)], s, cap)
            got = decode(dev, [(SLE, k)], s, cap)
            assert got[:2] == want[:2], (k, s.hex())
            assert want[0] in (0, -2) and (want[0] or (got[2], want[2]) == (1, 0))
            seen.add(want[0])
        assert decode(dev, [(SLE, k)], base, cap)[0] == 0                      # the context is usable afterwards
    assert seen == {0, -2}
    w_data = T.gen_english(70000, k).tobytes()
    assert dev.pipeline_decompress([(SLE, k)], dev.pipeline_compress([(SLE, k)], w_data)[0]) == w_data


def test_chain_bwt_rle_mtf_sle_on_english(dev, hostctx):
    text = T.gen_english(1 << 20, 42).tobytes() + b"\x00"
    stages = T.parse_chain("bwt:rle:mtf:encode(sle)")
    b = dev.bwt_compress(text)[0]
    r = BZ.rle_encode_np(b)
    m = BZ.mtf_encode(r)
    want = M.encode(m, 3)
    got, st = dev.pipeline_compress(stages, text)
    assert got == want and st["pipe_len"] == [len(b), len(r), len(m), len(want)]
    assert len(got) <= T.pipeline_bound(stages, len(text))
    assert decode(dev, stages, got, len(text)) == (0, text, 0b1111)
    assert decode(hostctx, stages, got, len(text)) == (0, text, 0b0001)        # (the inverse bwt always runs on the device)
    c = T.ChainCompressor(dev, "bwt:rle:mtf:encode(sle)")
    data = T.gen_english(200_000, 3).tobytes() + b"\x00\xff" * 20
    assert c.decompress(c.compress(data)) == data
    for enc in (T.LiteralEncoder(dev, coder="sle", kmer=2), T.LiteralEncoder(dev, coder="sle", kmer=2, dec="host")):
        z = enc.compress(data)
        assert z == M.encode(data, 2) and enc.decompress(z) == data


def test_buffers_and_invalid_stages(dev):
    data = T.gen_english(100_000, 4).tobytes()
    want = M.encode(data, 3)
    exact = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
    n, _ = dev.pipeline_compress_into([(SLE, 3)], data, len(data), exact[:len(want)])
    assert n == len(want) and exact[:n].tobytes() == want and bool((exact[n:] == 0xA5).all())
    small = np.full(4096, 0xA5, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        dev.pipeline_compress_into([(SLE, 3)], data, len(data), small[:1024])
    assert e.value.status == -5 and e.value.required == len(want) and bool((small == 0xA5).all())
    with pytest.raises(T.TdcGpuError) as e:
        dev.pipeline_decompress_into([(SLE, 3)], want, small[:100])
    assert e.value.status == -5 and e.value.required == len(data) and bool((small == 0xA5).all())
    for stages in ([5], [(SLE, 8)], [(5, 3)], [T.STAGE_MTF, (SLE, 9)]):
        assert T.pipeline_bound(stages, 100) == 0
        with pytest.raises(T.TdcGpuError) as e:
            dev.pipeline_compress(stages, data)
        assert e.value.status == -2, stages
        with pytest.raises(T.TdcGpuError) as e:
            dev.pipeline_decompress(stages, want)
        assert e.value.status == -2, stages
    assert dev.pipeline_compress([(SLE, 3)], data)[0] == want
    with T.Context(0, options={"pipe_log": 1, "dec_parse": 2}) as ctx:
        got, st = ctx.pipeline_compress([(SLE, 3)], data)
        assert got == want and st["pipe_ms"][0] > 0
        out = np.empty(len(data), dtype=np.uint8)
        n, st = ctx.pipeline_decompress_stats([(SLE, 3)], got, out)
        assert out[:n].tobytes() == data and st["pipe_dev"] == 1 and st["pipe_ms"][0] > 0


def test_bit_offsets_pass_2_32(dev):
    """384 MiB of uniform random bytes over 256 symbols at kmer = 3: 256 k-mers join, sigma_bits = 9, and all but the 40 first ranks
    cost 3 + 9 = 12 bits -- about 11 bits per byte on average, so the stream passes 2^32 bits = 2^29 bytes.  Encoded and decoded on
    the device; no model here, the SHA-256 of the output must be that of the input."""
    n = 384 << 20
    pin_in, pin_z, pin_back = T.PinnedBuffer(n), T.PinnedBuffer(T.pipeline_bound([(SLE, 3)], n)), T.PinnedBuffer(n)
    try:
        rng = np.random.default_rng(2)
        for lo in range(0, n, 64 << 20):
            pin_in.a[lo:lo + (64 << 20)] = rng.integers(0, 256, 64 << 20, dtype=np.uint8)
        want = hashlib.sha256(pin_in.a).hexdigest()
        zn, st = dev.pipeline_compress_into([(SLE, 3)], pin_in, n, pin_z)
        assert zn > (1 << 29) and zn * 8 > (1 << 32)
        m, st = dev.pipeline_decompress_stats([(SLE, 3)], pin_z, pin_back, zn)
        assert m == n and st["pipe_dev"] == 1
        assert hashlib.sha256(pin_back.a).hexdigest() == want
    finally:
        pin_in.free(); pin_z.free(); pin_back.free()
