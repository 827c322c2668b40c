"""GPU tests of the device decoders of rle, mtf and encode(huff) and of the device-resident decompress driver (pytest -m gpu; DESIGN.md
section 5.3).  The host decoders are the specification: the device path (option dec_parse = 2) must return their bytes or refuse what
they refuse; pipe_dev of tdc_gpu_pipeline_decompress_stats says which path a stage took."""
import ctypes
import os
import random
import subprocess
import time

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.models import bwtzip as M
from tests.util import sha256

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
BWT, RLE, MTF, HUFF = T.STAGE_BWT, T.STAGE_RLE, T.STAGE_MTF, T.STAGE_HUFF
BWTZIP = [BWT, RLE, MTF, HUFF]
# the project's cap for one adversarial call of 2^24 B (BOUNDED_CAP_S of tests/test_gpu_bytestages.py: 20 x its slowest compress call)
BOUNDED_CAP_S = 0.65
STAGE_MAX = (1 << 32) - 2


@pytest.fixture(scope="module")
def dev():
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def dev_seg():
    with T.Context(0, options={"dec_parse": 2, "dec_seg": 1 << 20}) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def hostctx():
    with T.Context(0, options={"dec_parse": 0}) as ctx:
        yield ctx


def mask(stages):
    return (1 << len(stages)) - 1


def host_stage(stage, s):
    """(status, bytes) of the host decoder of one stage; measured first, a stage above 2^32 - 2 bytes is refused like malformed input"""
    L = T._native.load()
    a = np.frombuffer(bytes(s), dtype=np.uint8)
    p = a.ctypes.data_as(ctypes.c_void_p) if len(a) else None
    n = ctypes.c_size_t()
    if stage == MTF:
        return 0, T.mtf_decode(s)
    if stage == HUFF:
        rc = L.tdc_huff_decode_literals(p, len(a), None, 0, ctypes.byref(n))
        return (rc, None) if rc or n.value > STAGE_MAX else (0, T.huff_decode_literals(s))
    rc = L.tdc_rle_decode(p, len(a), ctypes.c_uint64(stage[1]), None, 0, ctypes.byref(n))
    return (-2, None) if rc or n.value > STAGE_MAX else (0, T.rle_decode(s, stage[1]))


def device(ctx, stages, s, cap):
    """(status, bytes, stats) of pipeline_decompress_stats into a buffer of cap bytes"""
    out = np.full(max(cap, 1), 0xA5, dtype=np.uint8)
    try:
        n, st = ctx.pipeline_decompress_stats(stages, np.frombuffer(bytes(s), dtype=np.uint8) if len(s) else np.zeros(0, dtype=np.uint8), out)
    except T.TdcGpuError as e:
        return e.status, None, None
    return 0, out[:n].tobytes(), st


def generated():
    rng = random.Random(4)
    return [T.gen_english(3 << 20, 7).tobytes(), T.gen_dna(2 << 20, 8).tobytes(), corpus.run_rich(1 << 20, rng),
            (b"\x80" * 700 + b"\xff" * 900 + b"ab") * 900, bytes(range(256)) * 5000, corpus.fib_word(27)[:1 << 20]]


def test_each_decoder_alone_and_in_chains(dev, dev_seg, hostctx):
    small = [d for _, d in corpus.small_corpus() + corpus.random_small(40, 21)] + [b"a", b"\x80" * 9, b"\xff" * 5, bytes(range(256)) * 3]
    with T.Context(0) as default:
        for data in small + generated():
            for stages in ([(RLE, 0)], [(RLE, 3)], [MTF], [HUFF], [(RLE, 200), MTF, HUFF], [MTF, (RLE, 0)]):
                if HUFF in stages and (len(set(data)) == 256 or not data):
                    continue                                            # (256 symbols of one length: no decoder reads that header)
                z, _ = dev.pipeline_compress(stages, data)
                if len(stages) == 1:
                    assert host_stage(stages[0], z) == (0, data)
                for ctx in (dev, dev_seg):
                    rc, got, st = device(ctx, stages, z, len(data))
                    assert rc == 0 and got == data and st["pipe_dev"] == mask(stages), (stages, len(data))
                    assert st["out_len"] == len(data) and st["n"] == len(z) and st["pipe_len"][-1] == len(z)
                rc, got, st = device(hostctx, stages, z, len(data))
                assert rc == 0 and got == data and st["pipe_dev"] == 0
                rc, got, st = device(default, stages, z, len(data))
                assert rc == 0 and got == data and st["pipe_dev"] == (mask(stages) if len(z) >= 1 << 20 else 0), (stages, len(z))
            if data and len(data) <= 3 << 20:
                text = T.escape(data)
                z, cst = dev.pipeline_compress(BWTZIP, text)
                for ctx, want_dev in ((dev, 0b1111), (dev_seg, 0b1111), (hostctx, 0b0001)):
                    rc, got, st = device(ctx, BWTZIP, z, len(text))
                    assert rc == 0 and got == text and st["pipe_dev"] == want_dev and st["pipe_len"] == cst["pipe_len"]


def test_tile_and_chunk_borders(dev):
    rng = np.random.default_rng(3)
    for n in (1023, 1024, 1025, 4095, 4096, 4097, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 26) - 1, 1 << 26, (1 << 26) + 1):
        ranks = np.minimum(rng.geometric(0.08, n) - 1, 255).astype(np.uint8).tobytes()
        rc, got, st = device(dev, [MTF], ranks, n)
        assert rc == 0 and st["pipe_dev"] == 1 and sha256(np.frombuffer(got, dtype=np.uint8)) == sha256(np.frombuffer(T.mtf_decode(ranks), dtype=np.uint8)), n
    # the last code ends 0 .. 7 bits in front of the terminator, which is OR-ed into the last byte (& 7 < 6) or takes a byte of its own
    forms = set()
    for k in range(0, 64):
        data = b"ab" * 700 + b"c" * 300 + b"ab"[:k % 2] + b"a" * (k // 2)
        z = O.huff_encode_literals(data)
        forms.add((z[-1] & 7) >= 6)
        rc, got, st = device(dev, [HUFF], z, len(data))
        assert rc == 0 and got == data == T.huff_decode_literals(z) and st["pipe_dev"] == 1, k
    assert forms == {False, True}
    for n in (511, 512, 513, 4096 * 8 - 1, 4096 * 8, 4096 * 8 + 1):     # rle: input tiles of 512 bytes, 64 per workgroup
        data = (rng.integers(0, 3, n, dtype=np.uint8) * 0x40 + 0x40).astype(np.uint8).tobytes()
        z = M.rle_encode_np(data, 0)
        for cut in (len(z), min(len(z), 512), min(len(z), 513), min(len(z), 32768)):
            want = host_stage((RLE, 0), z[:cut])
            rc, got, _ = device(dev, [(RLE, 0)], z[:cut], len(data))
            assert (rc, got) == want, (n, cut)


def damaged(base, kind, i, rng):
    s = bytearray(base)
    if kind == "flip":
        for _ in range(1 + i % 3):
            s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
    elif kind == "cut":
        del s[rng.randrange(0, len(s)):]
    elif kind in ("vbyte10", "vbyte11"):                                # a pair somewhere, then a vbyte stretched to 10 / 11 bytes
        p = rng.randrange(0, len(s))
        tail = bytes([0x80 | rng.randrange(128)] * (9 if kind == "vbyte10" else 10)) + bytes([rng.randrange(2)])
        s[p:p] = bytes([0x61, 0x61]) + tail
    return bytes(s)


@pytest.mark.parametrize("stage", [(RLE, 0), (RLE, 3), MTF, HUFF], ids=["rle0", "rle3", "mtf", "huff"])
def test_differential_fuzz(dev, stage):
    """every damaged stream: the device's status equals the host decoder's, and its bytes when both accept -- none left out"""
    rng = random.Random(77)
    text = T.gen_english(20000, 5).tobytes() + corpus.run_rich(4000, rng) + b"\x80\x80\xff\xff" * 50
    base = dev.pipeline_compress([stage], text)[0]
    kinds = ["flip", "cut"] + (["vbyte10", "vbyte11", "offset"] if stage not in (MTF, HUFF) else [])
    counts = {}
    for kind in kinds:
        for i in range(150):
            st = stage
            if kind == "offset":                                         # an offset above every vbyte of the stream
                st = (RLE, rng.choice([1 << 20, 1 << 40, (1 << 62) - i, 24001 + i]))
                s = base if i % 2 else damaged(base, "flip", i, rng)
            else:
                s = damaged(base, kind, i, rng)
            want = host_stage(st, s)
            rc, got, _ = device(dev, [st], s, len(want[1]) if want[0] == 0 else 1 << 16)
            assert (rc, got) == (want[0], want[1]), (kind, i, s[:32].hex())
            counts[(kind, rc)] = counts.get((kind, rc), 0) + 1
    print("fuzz %s: %s" % (stage, sorted(counts.items())))
    assert dev.pipeline_decompress([stage], base) == text               # the context works on


def test_claimed_output_above_the_limit(dev):
    bomb = b"aa" + b"\xff" * 9 + b"\x01"
    assert device(dev, [(RLE, 0)], bomb, 64)[0] == -2
    big = b"aa" + M.vbyte((1 << 32) - 3)                                # 2^32 - 1 bytes: one above the limit
    assert device(dev, [(RLE, 0)], big, 64)[0] == -2 and host_stage((RLE, 0), big)[0] == -2
    assert dev.pipeline_decompress([(RLE, 0)], b"aa\x03b") == b"aaaaab"


def test_buffers(dev):
    data = T.gen_english(1 << 20, 9).tobytes() + b"z" * 70000
    text = T.escape(data)
    for stages, plain in ((BWTZIP, text), ([(RLE, 0), MTF, HUFF], data)):
        z = dev.pipeline_compress(stages, plain)[0]
        exact = np.full(len(plain) + 64, 0xA5, dtype=np.uint8)
        n, st = dev.pipeline_decompress_stats(stages, z, exact[:len(plain)])
        assert n == len(plain) and exact[:n].tobytes() == plain and bool((exact[n:] == 0xA5).all()) and st["pipe_dev"] == mask(stages)
        assert dev.pipeline_decompress_into(stages, z, exact[:len(plain)]) == len(plain)
        small = np.full(4096, 0xA5, dtype=np.uint8)
        for fn in (dev.pipeline_decompress_into, dev.pipeline_decompress_stats):
            with pytest.raises(T.TdcGpuError) as e:
                fn(stages, z, small[:100])
            assert e.value.status == -5 and e.value.required == len(plain) and bool((small == 0xA5).all())
        pin_in, pin_out = T.PinnedBuffer(len(z)), T.PinnedBuffer(len(plain))
        try:
            pin_in.a[:] = np.frombuffer(z, dtype=np.uint8)
            n, st = dev.pipeline_decompress_stats(stages, pin_in, pin_out)
            assert n == len(plain) and pin_out.a.tobytes() == plain and st["pipe_dev"] == mask(stages)
        finally:
            pin_in.free(); pin_out.free()


def test_bounded_work(dev):
    """2^24 B of adversarial input, second call on the context, wall clock of the whole call"""
    n = 1 << 24
    a, b = b"b", b"a"
    while len(b) < n:
        a, b = b, b + a
    fib = b[:n]
    cases = [("rle", "61^n", [(RLE, 0)], b"a" * n), ("rle", "80^n", [(RLE, 0)], b"\x80" * n), ("rle", "ff^n", [(RLE, 0)], b"\xff" * n),
             ("rle", "(ab)^k", [(RLE, 0)], b"ab" * (n // 2)), ("mtf", "ranks 255", [MTF], bytes(range(256)) * (n // 256)),
             ("huff", "sigma 1", [HUFF], b"a" * n), ("huff", "sigma 2", [HUFF], b"ab" * (n // 2)), ("huff", "fibonacci", [HUFF], fib)]
    slowest = 0.0
    for kind, name, stages, data in cases:
        for st, plain in ((stages, data), (BWTZIP, data[:n - 1].replace(b"\x00", b"\x01") + b"\x00")):
            z = dev.pipeline_compress(st, plain)[0]
            out = np.empty(len(plain), dtype=np.uint8)
            dev.pipeline_decompress_stats(st, z, out)
            t0 = time.perf_counter()
            m, stats = dev.pipeline_decompress_stats(st, z, out)
            dt = time.perf_counter() - t0
            print("bounded decode: %-5s %-10s %-6s %9d -> %9d bytes %8.4f s" % (kind, name, "chain" if st is BWTZIP else "alone", len(z), m, dt))
            slowest = max(slowest, dt)
            assert m == len(plain) and sha256(out) == sha256(np.frombuffer(plain, dtype=np.uint8)) and stats["pipe_dev"] == mask(st)
            assert dt < BOUNDED_CAP_S, (kind, name, dt)
    print("bounded decode: slowest %.4f s" % slowest)


@pytest.mark.parametrize("kind", ["english", "dna"])
def test_device_against_host_loops_256MiB(gpu_ctx, kind):
    """same context, both paths warmed, pinned buffers: the device chain takes at most one fifth of the host loops' time.  (The session's
    context: its arena is the one large allocation of a test run; a second context of that size may not fit beside it.)"""
    N = 1 << 28
    h_text, h_z, h_back = T.PinnedBuffer(N + 1), T.PinnedBuffer(N + 1), T.PinnedBuffer(N + 1)
    try:
        (T.gen_english if kind == "english" else T.gen_dna)(N, 42, out=h_text.a)
        h_text.a[N] = 0
        want = sha256(h_text.a)
        ctx = gpu_ctx
        try:
            zlen, cst = ctx.pipeline_compress_into(BWTZIP, h_text, N + 1, h_z)
            times = {}
            for mode in (2, 0):
                ctx.set_option("dec_parse", mode)
                for rep in range(2):
                    h_back.a[:4096] = 0
                    t0 = time.perf_counter()
                    n, st = ctx.pipeline_decompress_stats(BWTZIP, h_z, h_back, zlen)
                    times[mode] = time.perf_counter() - t0
                    assert n == N + 1 and st["pipe_dev"] == (0b1111 if mode else 0b0001) and st["pipe_len"] == cst["pipe_len"]
                assert sha256(h_back.a) == want
        finally:
            ctx.set_option("dec_parse", 1)
        print("decode %s 256 MiB: device %.1f ms, host loops %.1f ms, ratio %.1f" % (kind, times[2] * 1e3, times[0] * 1e3, times[0] / times[2]))
        assert times[2] * 5 <= times[0]
    finally:
        h_text.free(); h_z.free(); h_back.free()


def test_full_size_2e9(gpu_ctx):
    dev = gpu_ctx            # default options: a stream of this size takes the device path
    N = 2_000_000_000
    n = N + 1
    h_text, h_out = T.PinnedBuffer(n), T.PinnedBuffer(N)
    try:
        T.gen_english(N, 42, out=h_text.a)
        h_text.a[N] = 0
        want = sha256(h_text.a)
        zlen, cst = dev.pipeline_compress_into(BWTZIP, h_text, n, h_out)
        h_text.a[:] = 0
        t0 = time.perf_counter()
        m, st = dev.pipeline_decompress_stats(BWTZIP, h_out, h_text, zlen)
        dt = time.perf_counter() - t0
        print("2e9 decode: %.1f ms wall, %.1f ms in the call, lengths %s, arena %.1f GB (the host loops took 26.3 s)" %
              (dt * 1e3, st["ms_total"], st["pipe_len"], st["arena_bytes"] / 1e9))
        assert m == n and sha256(h_text.a) == want and st["pipe_dev"] == 0b1111 and st["pipe_len"] == cst["pipe_len"]
    finally:
        h_text.free(); h_out.free()


def test_facades(dev, tmp_path):
    data = b"\x00\xffab\xff\xfe\x00" * 500 + T.gen_english(2 << 20, 8).tobytes() + bytes(range(255)) * 20 + b"\xff\xff"
    with T.Context(0) as ctx:
        for comp in (T.ChainCompressor(ctx, "bwt:rle:mtf:encode(huff)"), T.RunLengthEncoder(ctx, 3), T.MTFCompressor(ctx), T.LiteralEncoder(ctx)):
            assert comp.decompress(comp.compress(data)) == data
    src = tmp_path / "in.bin"
    src.write_bytes(data)
    env = dict(os.environ, TDC_GPU_DEBUG_KNOBS="1", TDC_GPU_PIPE_LOG="1", TDC_GPU_DEC_LOG="1")
    for algo in ("rle", "rle(offset=3)", "mtf", "encode(huff)"):
        z, back = tmp_path / "z.tdc", tmp_path / "back.bin"
        r = subprocess.run([TDC, "-a", algo, "-f", "-o", str(z), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert z.stat().st_size > 1 << 20
        r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(z)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data
        assert "(device)" in r.stderr and "(host)" not in r.stderr, r.stderr
