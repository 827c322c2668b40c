"""GPU tests of the bwt compressor (pytest -m gpu): the forward transform against the reference's known-answer test and the oracle's
suffix array, the inverse against the input of the forward transform (the reference's own decoder is wrong on texts with 0xFF, DESIGN.md
section 5.2) and against the numpy LF table, buffers, malformed input, the facade and the command line, and 2*10^9 B end to end."""
import json
import os
import random
import subprocess
import time

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.models import bwt as M
from tests.util import sha256

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
KATS = json.load(open(os.path.join(HERE, "golden", "reference_kats.json")))

# Wall-clock cap of one structured text of 2^24 and more bytes through forward + inverse (second call on the context).  One run of the
# slowest of them, the planted repeats, took 0.051 s on an MI355X (the figures are in DESIGN.md section 5.2); the cap is 20 x that.  It
# catches a walk that is not bounded, it does not rate speed.
STRUCTURED_CAP_S = 1.0


def want_bwt(text):
    return M.bwt_from_sa(text, O.suffix_array(text))


def numpy_lf(b):
    return M.lf_table(b).astype(np.uint32)


def roundtrip(ctx, text, check_forward=True):
    got, st = ctx.bwt_compress(text)
    assert len(got) == len(text) and st["n"] == len(text) and st["out_len"] == len(text)
    if check_forward:
        assert got == want_bwt(text)
    back, _ = ctx.bwt_decompress(got)
    assert back == (text if len(text) > 1 else b"")
    return got, st


@pytest.mark.parametrize("k", KATS["bwt"], ids=lambda k: k["source"][:24])
def test_reference_kat(gpu_ctx, k):
    text = bytes.fromhex(k["text_hex"])
    got, _ = gpu_ctx.bwt_compress(text)
    assert got == bytes.fromhex(k["bwt_hex"])
    back, _ = gpu_ctx.bwt_decompress(got)
    assert back == text


def test_small_corpus_and_random_texts(gpu_ctx):
    for name, data in corpus.small_corpus() + corpus.random_small(200, 4711):
        roundtrip(gpu_ctx, T.escape(data))
    roundtrip(gpu_ctx, T.escape(bytes(range(256)) * 40))


@pytest.mark.parametrize("gen,seed,n", [("english", 42, 1 << 20), ("dna", 7, 1 << 20), ("english", 5, 1 << 24), ("dna", 9, 1 << 24)])
def test_generated_texts_against_the_oracle(gpu_ctx, gen, seed, n):
    data = (T.gen_english if gen == "english" else T.gen_dna)(n, seed)
    text = np.concatenate([data, np.zeros(1, dtype=np.uint8)]).tobytes()
    roundtrip(gpu_ctx, text)


def test_every_suffix_array_path(gpu_ctx):
    """the texts of test_every_option_value_is_bit_exact: wide path, doubling fall-back; the classic path through option wsort = 0"""
    rng = np.random.default_rng(3)
    blk = bytes(rng.integers(0, 4, 40_000, dtype=np.uint8).astype(np.uint8) + 65)
    texts = [O.escape(T.gen_english(3_000_000, 17).tobytes()),
             O.escape(T.gen_dna(1_200_000, 5).tobytes() + blk + b"#" + blk[100:30_000] + T.gen_dna(300_000, 6).tobytes() + blk[5_000:])]
    wants = [want_bwt(t) for t in texts]
    modes = set()
    for t, w in zip(texts, wants):
        got, st = roundtrip(gpu_ctx, t, check_forward=False)
        assert got == w
        modes.add((st["sa_key_words"] > 0, st["sa_mode"]))
    with T.Context(0, options={"wsort": 0}) as ctx:
        for t, w in zip(texts, wants):
            got, st = ctx.bwt_compress(t)
            assert got == w and st["sa_key_words"] == 0
    assert (True, 1) in modes and (True, 0) in modes          # the wide path with and without the doubling fall-back


@pytest.mark.parametrize("sample", [1, 3, 64, 4096])
@pytest.mark.parametrize("max_steps", [1, 5, 0])
def test_inverse_stage_parameters(gpu_ctx, sample, max_steps):
    texts = [T.escape(T.gen_english(200_000, 3).tobytes() + b"\x00\xff" * 300), b"a" * 70_000 + b"\0", T.escape(corpus.fib_word(22)),
             b"x\0", b"ab\xff\xfecd\xff\xffab\xfe\xfe\0"]
    for text in texts:
        b = want_bwt(text)
        out, st = gpu_ctx.bwt_inverse_stage(b, sample, max_steps)
        assert out == text, (sample, max_steps, len(text))
        assert np.array_equal(st["lf"], numpy_lf(b))
        assert st["launches"] >= 1 and 1 <= st["heads"] <= len(text)
        if max_steps == 1 or sample == 1:
            assert st["heads"] == len(text)                  # every row is a head


def structured_texts():
    rng = random.Random(99)
    n = 1 << 24
    base = corpus.planted(1 << 16, 4, rng, replen=2000)
    rr = corpus.run_rich(1 << 16, rng)
    return [("a^(2^24)", b"a" * n), ("(ab)^k", b"ab" * (n // 2)), ("fibonacci", corpus.fib_word(35)[:n + 12345]), ("thue_morse", corpus.thue_morse(24)),
            ("run_rich", (rr * (n // len(rr) + 1))[:n]), ("planted", (base * (n // len(base) + 1))[:n + 777])]


@pytest.mark.parametrize("name,data", structured_texts(), ids=lambda v: v if isinstance(v, str) else "")
def test_structured_texts_finish(gpu_ctx, name, data):
    text = data + b"\0"
    gpu_ctx.bwt_decompress(gpu_ctx.bwt_compress(text)[0])            # (the arena grows to the text's size outside the timed call)
    t0 = time.perf_counter()
    got, _ = gpu_ctx.bwt_compress(text)
    back, _ = gpu_ctx.bwt_decompress(got)
    dt = time.perf_counter() - t0
    print("bwt structured %-12s n %d: forward + inverse %.3f s" % (name, len(text), dt))
    assert back == text
    assert dt < STRUCTURED_CAP_S, (name, dt)
    for s, m in ((64, 5), (4096, 0)):
        t0 = time.perf_counter()
        out, st = gpu_ctx.bwt_inverse_stage(got, s, m, want_lf=False)
        dt = time.perf_counter() - t0
        print("bwt structured %-12s sample %d max_steps %d: %.3f s, %d heads, %d launches" % (name, s, m, dt, st["heads"], st["launches"]))
        assert out == text and dt < STRUCTURED_CAP_S, (name, s, m, dt)


def test_into_buffers(gpu_ctx):
    text = T.escape(T.gen_english(300_000, 8).tobytes() + b"\x00\xff")
    n = len(text)
    want = want_bwt(text)
    for fn, src, res in ((gpu_ctx.bwt_compress_into, text, want), (gpu_ctx.bwt_decompress_into, want, text)):
        buf = np.full(n + 64, 0xA5, dtype=np.uint8)
        args = (src, n, buf[:n]) if fn == gpu_ctx.bwt_compress_into else (src, buf[:n])
        got_n, _ = fn(*args)                                                       # exact fit
        assert got_n == n and buf[:n].tobytes() == res and bool((buf[n:] == 0xA5).all())
        buf[:] = 0xA5
        args = (src, n, buf[:n - 1]) if fn == gpu_ctx.bwt_compress_into else (src, buf[:n - 1])
        with pytest.raises(T.TdcGpuError) as e:                                   # one byte short
            fn(*args)
        assert e.value.status == -5 and e.value.required == n and bool((buf == 0xA5).all())
    pin_in, pin_out = T.PinnedBuffer(n), T.PinnedBuffer(n)
    try:
        pin_in.a[:] = np.frombuffer(text, dtype=np.uint8)
        got_n, st = gpu_ctx.bwt_compress_into(pin_in, n, pin_out)
        assert got_n == n and pin_out.a.tobytes() == want and st["ms_total"] > 0 and st["ms_sa"] > 0
        got_n, _ = gpu_ctx.bwt_decompress_into(pin_out, pin_in)
        assert got_n == n and pin_in.a.tobytes() == text
    finally:
        pin_in.free(); pin_out.free()
    for tiny in (b"", b"\0", b"q"):
        out, _ = gpu_ctx.bwt_decompress(tiny)
        assert out == b""
        buf = np.full(8, 0xA5, dtype=np.uint8)
        got_n, _ = gpu_ctx.bwt_decompress_into(tiny, buf)
        assert got_n == 0 and bool((buf == 0xA5).all())


def two_cycles(n, seed):
    """one 0 byte, but the LF permutation has more than one cycle"""
    rng = np.random.default_rng(seed)
    while True:
        b = rng.integers(1, 5, n, dtype=np.uint8)
        b[int(rng.integers(0, n))] = 0
        lf = M.lf_table(b.tobytes())
        i, seen = 0, 0
        while True:
            i = int(lf[i]); seen += 1
            if i == 0:
                break
        if seen < n:
            return b.tobytes()


def test_malformed_input_is_refused(gpu_ctx):
    text = T.escape(T.gen_english(100_000, 12).tobytes())
    good = want_bwt(text)
    z = good.index(b"\0")
    rng = np.random.default_rng(1)
    bad = {"no 0 byte": good[:z] + b"x" + good[z + 1:], "two 0 bytes": good[:7] + b"\0" + good[7:], "two cycles": two_cycles(50_000, 3),
           "two cycles, short": two_cycles(12, 4), "random bytes": rng.integers(0, 256, 65_536, dtype=np.uint8).tobytes(),
           "random bytes, one 0": bytes(rng.integers(1, 256, 65_536, dtype=np.uint8)) + b"\0"}
    for what, b in bad.items():
        for s, m in ((0, 0), (1, 1), (64, 5)):
            with pytest.raises(T.TdcGpuError) as e:
                gpu_ctx.bwt_inverse_stage(b, s, m)
            assert e.value.status == -2, (what, s, m)
        buf = np.full(len(b) + 16, 0xA5, dtype=np.uint8)
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.bwt_decompress_into(b, buf)
        assert e.value.status == -2 and bool((buf == 0xA5).all()), what
        with pytest.raises(T.TdcGpuError):
            gpu_ctx.bwt_decompress(b)
    got, _ = gpu_ctx.lcpcomp_compress(text, threshold=2, flatten=1)                # the context is usable afterwards
    assert got == O.lcpcomp_huff_compress(text, 2, 1)[0]
    assert gpu_ctx.bwt_decompress(good)[0] == text
    for bad_text, status in ((b"abc", -3), (b"", -3), (b"ab\0cd\0", -2)):           # the lcpcomp codes
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.bwt_compress(bad_text)
        assert e.value.status == status, bad_text


def test_facade_and_command_line(gpu_ctx, tmp_path):
    data = b"\x00\xff\xfe" * 1000 + T.gen_english(400_000, 6).tobytes() + bytes(range(256)) * 5
    z = T.BWTCompressor(gpu_ctx)
    stream = z.compress(data)
    assert len(stream) == len(T.escape(data)) and z.decompress(stream) == data
    assert z.decompress(z.compress(b"")) == b""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    src, comp, back = tmp_path / "in.bin", tmp_path / "in.tdc", tmp_path / "back.bin"
    src.write_bytes(data)
    for algo in ("bwt(dec=gpu)", "bwt"):
        r = subprocess.run([TDC, "-a", algo, "-f", "-o", str(comp), str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        blob = comp.read_bytes()
        assert blob == algo.encode() + b"%" + stream
        r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(comp)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data


def test_2e9_english_round_trip(gpu_ctx):
    """The inverse is checked on its own at the small sizes and the transform is injective on 0-terminated texts, so the round trip
    certifies the forward transform at a size the oracle's suffix array does not reach."""
    N = 2_000_000_000
    n = N + 1
    h_text, h_bwt = T.PinnedBuffer(n), T.PinnedBuffer(n)
    try:
        T.gen_english(N, 42, out=h_text.a)
        h_text.a[N] = 0
        want = sha256(h_text.a)
        got_n, st = gpu_ctx.bwt_compress_into(h_text, n, h_bwt)
        assert got_n == n and st["n"] == n and st["ms_sa"] > 0 and st["ms_encode"] > 0
        assert int(np.count_nonzero(h_bwt.a == 0)) == 1 and h_bwt.a[0] == h_text.a[N - 1]
        h_text.a[:] = 0xA5
        back_n, dst = gpu_ctx.bwt_decompress_into(h_bwt, h_text)
        assert back_n == n and dst["rounds"] >= 1
        assert sha256(h_text.a) == want
    finally:
        h_text.free(); h_bwt.free()
