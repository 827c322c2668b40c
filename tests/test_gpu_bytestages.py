"""GPU tests of rle, mtf, encode(huff) and their chains behind bwt (pytest -m gpu): every stage byte for byte
against the model (tests/models/bwtzip.py) or the oracle's literal encoder, the chain against their composition over the oracle's suffix
array, bounded work on adversarial inputs, buffers and errors, the facades and the command line, and 2*10^9 B through the chain and back."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.models import bwt as MB
from tests.models import bwtzip as M
from tests.util import sha256

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
BWT, RLE, MTF, HUFF = T.STAGE_BWT, T.STAGE_RLE, T.STAGE_MTF, T.STAGE_HUFF
BWTZIP = [BWT, RLE, MTF, HUFF]
# kernel geometry (csrc/bytestages.hpp): rle and huff work on 16 bytes per thread and 4096 per workgroup, mtf on 1024 per thread and
# 256 KiB per workgroup, and its summaries are scanned in groups of 256 workgroups (64 MiB)
BORDERS = (16, 4096, 1024, 1 << 18)

# Wall-clock cap of one adversarial input of 2^24 B through one call (second call on the context).  One run of the slowest of them --
# (ab)^k through the whole chain -- took 0.0324 s on an MI355X; the slowest single stage was ff^n through rle with 0.0224 s, and
# (00 .. ff) repeated through mtf, every byte at rank 255, took 0.0205 s (all figures: DESIGN.md section 5.3).  The cap is 20 x the
# slowest, the rule of STRUCTURED_CAP_S in tests/test_gpu_bwt.py.  It catches a loop that is not bounded, it does not rate speed.
BOUNDED_CAP_S = 0.65


def want_bwt(text):
    return MB.bwt_from_sa(text, O.suffix_array(text))


def model(stage, data):
    if stage == MTF:
        return M.mtf_encode(data)
    if stage == HUFF:
        return O.huff_encode_literals(data)
    return M.rle_encode_np(data, stage[1])


def small_inputs():
    rng = np.random.default_rng(11)
    out = [d for _, d in corpus.small_corpus() + corpus.random_small(200, 815)]
    out += [b"", b"a", b"\x80", b"\xff", b"ab", b"aa", b"\xff\xff", b"\x80\x80", bytes(range(256)), bytes(range(256)) * 3]
    for c in (0x7F, 0x80, 0xFF):
        for k in (2, 3, 129, 130, 5000):
            out += [bytes([c]) * k, b"x" + bytes([c]) * k, bytes([c]) * k + b"x", b"ab" * 7 + bytes([c]) * k]
    for b in BORDERS[:3]:
        for k in (1, 2, 5):
            for d in (-1, 0, 1):
                n = b * k + d
                out.append(rng.integers(97, 101, n, dtype=np.uint8).tobytes())             # short runs over four letters
                out.append((rng.integers(0, 2, n, dtype=np.uint8) * 0x80 + 0x7F).astype(np.uint8).tobytes())   # 7f / ff
    out.append(b"q" * 70000)
    out.append(b"q" * 4095 + b"r" * 4098 + b"\x90" * 4097 + b"s")
    return out


def test_each_stage_alone_on_small_inputs(gpu_ctx):
    for data in small_inputs():
        for stage in ((RLE, 0), (RLE, 1), (RLE, 200), MTF, HUFF):
            got, st = gpu_ctx.pipeline_compress([stage], data)
            assert got == model(stage, data), (stage, len(data), data[:16])
            assert st["pipe_len"] == [len(got)] and st["n"] == len(data) and st["out_len"] == len(got)


def test_rle_matches_the_python_loop_too(gpu_ctx):
    for data in small_inputs()[::7]:
        for off in (0, 3, 1 << 40):
            assert gpu_ctx.pipeline_compress([(RLE, off)], data)[0] == M.rle_encode(data, off)


def test_tile_borders_of_mtf(gpu_ctx):
    rng = np.random.default_rng(12)
    for k in (1, 2):
        for d in (-1, 0, 1):
            n = (1 << 18) * k + d
            for data in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), (np.arange(n) % 251).astype(np.uint8).tobytes()):
                for stage in (MTF, (RLE, 0), HUFF):
                    assert gpu_ctx.pipeline_compress([stage], data)[0] == model(stage, data), (stage, n)


def fib_weighted(n_syms=40):
    """byte values with Fibonacci counts: Huffman codes of up to n_syms - 1 bits, code words wider than 32 bits"""
    fib = [1, 1]
    while len(fib) < n_syms:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(13)
    a = np.repeat(np.arange(n_syms, dtype=np.uint8) + 100, fib)
    rng.shuffle(a)
    return a.tobytes()


def test_huff_sigma_one_and_deep_codes(gpu_ctx):
    fibtext = fib_weighted(35)                                   # 24 MB
    for data in (b"z" * 100000, b"\x00" * 4097, fibtext, corpus.deep_code_text(34)):
        want = O.huff_encode_literals(data)
        assert gpu_ctx.pipeline_compress([HUFF], data)[0] == want
    C = np.bincount(np.frombuffer(fibtext, dtype=np.uint8), minlength=256).astype(np.uint32)
    assert T.huffman_table(C)["longest"] > 32
    assert gpu_ctx.pipeline_decompress([HUFF], O.huff_encode_literals(fibtext[:1 << 20] + fibtext[-4096:])) == fibtext[:1 << 20] + fibtext[-4096:]


TEXTS = [("english", 42, 1 << 20), ("dna", 7, 1 << 20), ("english", 5, 1 << 24), ("dna", 9, 1 << 24)]


def gen_text(gen, seed, n):
    data = (T.gen_english if gen == "english" else T.gen_dna)(n, seed)
    return np.concatenate([data, np.zeros(1, dtype=np.uint8)]).tobytes()


@pytest.fixture(scope="module")
def texts():
    """(text, its transform from the oracle's suffix array) per entry of TEXTS"""
    out = {}
    for key in TEXTS:
        text = gen_text(*key)
        out[key] = (text, want_bwt(text))
    return out


@pytest.mark.parametrize("key", TEXTS, ids=lambda k: "%s-%d" % (k[0], k[2]))
def test_stages_and_chain_on_generated_texts(gpu_ctx, texts, key):
    text, b = texts[key]
    for data in (text[:-1], b):
        for stage in ((RLE, 0), MTF, HUFF):
            assert gpu_ctx.pipeline_compress([stage], data)[0] == model(stage, data), (key, stage)
    # the chain = the models composed over the oracle's transform = the four single-stage device calls composed
    r = M.rle_encode_np(b)
    m = M.mtf_encode(r)
    want = O.huff_encode_literals(m)
    got, st = gpu_ctx.pipeline_compress(BWTZIP, text)
    assert got == want
    assert st["pipe_len"] == [len(b), len(r), len(m), len(want)] and st["sa_rounds"] > 0
    x = gpu_ctx.bwt_compress(text)[0]
    assert x == b                                                # (bwt_compress itself is unchanged by the pipeline's hook)
    for stage in ((RLE, 0), MTF, HUFF):
        x = gpu_ctx.pipeline_compress([stage], x)[0]
    assert x == got
    assert gpu_ctx.pipeline_decompress(BWTZIP, got) == text
    # sub-chains
    got2, _ = gpu_ctx.pipeline_compress([BWT, MTF, HUFF], text)
    assert got2 == O.huff_encode_literals(M.mtf_encode(b))
    assert gpu_ctx.pipeline_decompress([BWT, MTF, HUFF], got2) == text
    got3, _ = gpu_ctx.pipeline_compress([(RLE, 0), MTF], text)
    assert got3 == M.mtf_encode(M.rle_encode_np(text))
    assert gpu_ctx.pipeline_decompress([(RLE, 0), MTF], got3) == text


def adversarial():
    n = 1 << 24
    return [("61^n", b"\x61" * n), ("80^n", b"\x80" * n), ("ff^n", b"\xff" * n), ("(00..ff)*", bytes(range(256)) * (n // 256)),
            ("(ab)^k", b"ab" * (n // 2))]


def test_bounded_work_on_adversarial_inputs(gpu_ctx):
    gpu_ctx.pipeline_compress([(RLE, 0), MTF, HUFF], gen_text("english", 1, 1 << 24))       # first call: the arena
    slowest = 0.0
    for name, data in adversarial():
        chain_in = data.replace(b"\x00", b"\x01").replace(b"\xff", b"\xfe")[:-1] + b"\x00"   # a valid view for the leading bwt
        for stages, inp in (([(RLE, 0)], data), ([MTF], data), (BWTZIP, chain_in)):
            t0 = time.perf_counter()
            got, st = gpu_ctx.pipeline_compress(stages, inp)
            dt = time.perf_counter() - t0
            print("bounded: %-10s %-24s %8.4f s -> %d bytes" % (name, stages, dt, len(got)))
            slowest = max(slowest, dt)
            assert dt < BOUNDED_CAP_S, (name, stages, dt)
            if stages == [(RLE, 0)]:
                assert got == M.rle_encode_np(data)
            elif stages == [MTF]:
                period = 256 if name == "(00..ff)*" else 2
                assert got[:4096] == M.mtf_encode(data[:4096]) and got[-period:] == got[4096:4096 + period] and len(got) == len(data)
                assert T.mtf_decode(got[:1 << 20]) == data[:1 << 20] and gpu_ctx.pipeline_decompress([MTF], got) == data
            else:
                assert gpu_ctx.pipeline_decompress(BWTZIP, got) == inp
    print("bounded: slowest %.4f s" % slowest)


def test_buffers_and_errors(gpu_ctx):
    text = T.escape(T.gen_english(300_000, 4).tobytes() + b"\x00\xff" * 50)
    want, _ = gpu_ctx.pipeline_compress(BWTZIP, text)
    assert 0 < T.pipeline_bound(BWTZIP, len(text)) and len(want) <= T.pipeline_bound(BWTZIP, len(text))
    exact = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
    n, st = gpu_ctx.pipeline_compress_into(BWTZIP, text, len(text), exact[:len(want)])
    assert n == len(want) and exact[:n].tobytes() == want and bool((exact[n:] == 0xA5).all())
    small = np.full(4096, 0xA5, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.pipeline_compress_into(BWTZIP, text, len(text), small[:1024])
    assert e.value.status == -5 and e.value.required == len(want) and bool((small == 0xA5).all())
    pin_in, pin_out, pin_back = T.PinnedBuffer(len(text)), T.PinnedBuffer(len(want) + 10), T.PinnedBuffer(len(text))
    try:
        pin_in.a[:] = np.frombuffer(text, dtype=np.uint8)
        n, _ = gpu_ctx.pipeline_compress_into(BWTZIP, pin_in, len(text), pin_out)
        assert pin_out.a[:n].tobytes() == want
        assert gpu_ctx.pipeline_decompress_into(BWTZIP, pin_out, pin_back, n) == len(text) and pin_back.a.tobytes() == text
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.pipeline_decompress_into(BWTZIP, want, small[:100])
        assert e.value.status == -5 and e.value.required == len(text) and bool((small == 0xA5).all())
        r = gpu_ctx.pipeline_compress([(RLE, 0), MTF], text)[0]
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.pipeline_decompress_into([(RLE, 0), MTF], r, small[:100])
        assert e.value.status == -5 and e.value.required == len(text) and bool((small == 0xA5).all())
    finally:
        pin_in.free(); pin_out.free(); pin_back.free()
    # invalid pipelines
    for stages, status in (([], -2), ([MTF] * 9, -2), ([7], -2), ([(RLE, 1 << 63)], -2), ([MTF, BWT], -3), ([BWT, BWT], -3)):
        assert T.pipeline_bound(stages, 100) == 0
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.pipeline_compress(stages, text)
        assert e.value.status == status, stages
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.pipeline_decompress(stages, want)
        assert e.value.status == status, stages
    with pytest.raises(T.TdcGpuError) as e:                     # missing sentinel
        gpu_ctx.pipeline_compress(BWTZIP, text[:-1])
    assert e.value.status == -3
    with pytest.raises(T.TdcGpuError) as e:                     # a 0 inside the text
        gpu_ctx.pipeline_compress(BWTZIP, b"ab\x00cd\x00")
    assert e.value.status == -2
    for bad in (want[:len(want) // 2], b"", b"\x80"):          # malformed streams are refused, not trusted
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.pipeline_decompress(BWTZIP, bad)
        assert e.value.status == -2
    assert gpu_ctx.pipeline_compress(BWTZIP, text)[0] == want   # the context works on
    with T.Context(0, options={"pipe_log": 1}) as ctx:
        got, st = ctx.pipeline_compress(BWTZIP, text)
        assert got == want and len(st["pipe_ms"]) == 4 and all(t > 0 for t in st["pipe_ms"])
        assert ctx.pipeline_decompress(BWTZIP, got) == text


def test_facades(gpu_ctx, tmp_path):
    data = b"\x00\xffab\xff\xfe\x00" * 500 + T.gen_english(100_000, 8).tobytes() + bytes(range(256)) * 20 + b"\xff\xff"
    c = T.ChainCompressor(gpu_ctx, "bwt:rle:mtf:encode(huff)")
    z = c.compress(data)
    assert len(z) < len(data) and c.last_stats["pipe_stages"] == 4
    assert c.decompress(z) == data
    assert c.compress(b"") and c.decompress(c.compress(b"")) == b""
    for comp, want in ((T.RunLengthEncoder(gpu_ctx, 3), M.rle_encode(data, 3)), (T.MTFCompressor(gpu_ctx), M.mtf_encode(data)),
                       (T.LiteralEncoder(gpu_ctx), O.huff_encode_literals(data))):
        z = comp.compress(data)
        assert z == want and comp.decompress(z) == data
    with pytest.raises(RuntimeError):
        T.ChainCompressor(gpu_ctx, "bwt:lz4")
    src = tmp_path / "in.bin"
    src.write_bytes(data)
    for algo, payload in (("rle", M.rle_encode(data)), ("rle(offset=3)", M.rle_encode(data, 3)), ("mtf", M.mtf_encode(data)),
                          ("encode(huff)", O.huff_encode_literals(data))):
        z, back = tmp_path / "z.tdc", tmp_path / "back.bin"
        r = subprocess.run([TDC, "-a", algo, "-f", "-o", str(z), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert z.read_bytes().endswith(payload) and z.read_bytes().split(b"%", 1)[1] == payload
        r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(z)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data


def test_chain_2e9_end_to_end(gpu_ctx):
    """64-bit offsets, arena and tiling at scale: 2*10^9 B of English through bwt:rle:mtf:encode(huff) into pinned memory and back"""
    N = 2_000_000_000
    n = N + 1
    h_text = T.PinnedBuffer(n)
    h_out = T.PinnedBuffer(N)
    try:
        T.gen_english(N, 42, out=h_text.a)
        h_text.a[N] = 0
        want = sha256(h_text.a)
        out_len, st = gpu_ctx.pipeline_compress_into(BWTZIP, h_text, n, h_out)
        print("2e9: lengths %s, %.1f ms" % (st["pipe_len"], st["ms_total"]))
        assert st["n"] == n and st["out_len"] == out_len and st["pipe_len"][0] == n and st["pipe_len"][3] == out_len and 0 < out_len < N // 2
        h_text.a[:] = 0
        assert gpu_ctx.pipeline_decompress_into(BWTZIP, h_out, h_text, out_len) == n
        assert sha256(h_text.a) == want
    finally:
        h_text.free(); h_out.free()
