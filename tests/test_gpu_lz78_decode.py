"""GPU tests of the device decoder of lz78(coder=gamma) streams (tdc_gpu_lz78_decompress{,_into}, lz78_decode.hip): round trips of the
oracle's and the device compressor's streams against their inputs (the decoded text is unique, so the input is the oracle), many
segments, the caller's buffer, the reference's sign-extended left-over phrase, malformed and oversized streams, the 10^9 B configs[3]
stream, and `tdc -d` with dec=gpu."""
import os
import random
import subprocess
import time

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.models import lz78_decode as M
from tests.models.lz78_decode import BitWriter
from tests.util import sha256, load_json

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")


def _ascii_tail(data):
    """the reference writes a left-over phrase that ends in a byte >= 0x80 as a sign-extended char: keep it ASCII"""
    return data if not data or data[-1] < 0x80 else data + b"."


def _round_trip(ctx, data):
    stream = O.lz78_gamma_compress(data)
    got, st = ctx.lz78_decompress(stream)
    assert got == data
    return st


@pytest.mark.parametrize("name,data", [(n, _ascii_tail(d)) for n, d in corpus.small_corpus()], ids=lambda x: x if isinstance(x, str) else "")
def test_round_trip_small_corpus(gpu_ctx, name, data):
    _round_trip(gpu_ctx, data)


def test_round_trip_random_small(gpu_ctx):
    for _, data in corpus.random_small(200, 780):
        _round_trip(gpu_ctx, _ascii_tail(data))


def test_round_trip_all_byte_values(gpu_ctx):
    rng = random.Random(3)
    for n in (1, 255, 4096, 100000):
        data = _ascii_tail(bytes(rng.randrange(256) for _ in range(n)) + bytes(range(256)))
        _round_trip(gpu_ctx, data)


def test_empty_and_one_byte(gpu_ctx):
    got, st = gpu_ctx.lz78_decompress(O.lz78_gamma_compress(b""))
    assert got == b"" and st["phrases"] == 0
    got, st = gpu_ctx.lz78_decompress(b"")
    assert got == b""
    got, st = gpu_ctx.lz78_decompress(O.lz78_gamma_compress(b"q"))
    assert got == b"q" and st["phrases"] == 1


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 10**5, 10**7])
def test_round_trip_runs(gpu_ctx, n):
    """a^n: phrase k is a^(k+1), depth ~ sqrt(2n) (about 4 500 at 10^7): deep reference chains"""
    st = _round_trip(gpu_ctx, b"a" * n)
    assert st["rounds"] >= 1


@pytest.mark.parametrize("n", [1, 50, 10**6])
def test_round_trip_ab(gpu_ctx, n):
    _round_trip(gpu_ctx, b"ab" * n)


@pytest.mark.parametrize("k", [5, 15, 27])
def test_round_trip_fibonacci(gpu_ctx, k):
    _round_trip(gpu_ctx, corpus.fib_word(k))


@pytest.mark.parametrize("gen,n", [("english", 1 << 20), ("dna", 1 << 20), ("english", 1 << 25), ("dna", 1 << 25)])
def test_round_trip_large(gpu_ctx, gen, n):
    data = (T.gen_english if gen == "english" else T.gen_dna)(n, 17).tobytes()
    data = _ascii_tail(data)
    st = _round_trip(gpu_ctx, data)
    assert st["phrases"] == len(O.lz78_factors(data)[0])


def test_device_compressor_round_trip(gpu_ctx):
    z = T.LZ78Compressor(gpu_ctx)
    for data in (b"", b"x", b"abracadabra" * 1000, _ascii_tail(T.gen_english(3 << 20, 5).tobytes()),
                 _ascii_tail(T.gen_dna(1 << 20, 6).tobytes())):
        assert z.decompress(z.compress(data)) == data


def test_many_segments():
    data = T.gen_english(3 << 20, 8).tobytes()
    stream = O.lz78_gamma_compress(data)
    with T.Context(0, options={"dec_seg": 4096}) as ctx:
        got, _ = ctx.lz78_decompress(stream)
    assert len(stream) * 8 // 4096 >= 500
    assert got == data


def test_into_pinned_and_one_byte_short(gpu_ctx):
    data = T.gen_english(5 << 20, 9).tobytes()
    stream = O.lz78_gamma_compress(data)
    src = T.PinnedBuffer(len(stream))
    src.a[:] = np.frombuffer(stream, dtype=np.uint8)
    out = T.PinnedBuffer(len(data))
    n, st = gpu_ctx.lz78_decompress_into(src, out)
    assert n == len(data) and out.a[:n].tobytes() == data and st["phrases"] > 0
    short = np.zeros(len(data) - 1, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.lz78_decompress_into(stream, short)
    assert e.value.status == ERR_OOM and e.value.required == len(data)
    src.free()
    out.free()


def test_reference_written_leftover(gpu_ctx):
    """LZ78Compressor.hpp:124-127 passes the left-over phrase's last byte as a (signed) char: >= 0x80 becomes a 64-bit gamma code"""
    w = BitWriter()
    for ident, ch in ((0, ord("x")), (0, ord("y")), (1, ord("y")), (3, ord("z"))):
        w.pair(ident, ch)
    w.pair(3, 0xFFFFFFFFFFFFFF80)                       # "xy" + 0x80
    got, st = gpu_ctx.lz78_decompress(w.finish())
    assert got == b"x" + b"y" + b"xy" + b"xyz" + b"xy\x80"
    assert st["phrases"] == 5


def _valid_after(ctx):
    data = b"the same context decodes a valid stream " * 50
    assert ctx.lz78_decompress(O.lz78_gamma_compress(data))[0] == data


def _malformed():
    good = O.lz78_gamma_compress(b"abcabcabcabd" * 40)
    w = BitWriter()
    w.bits = [int(b) for b in np.unpackbits(np.frombuffer(good, dtype=np.uint8))]
    total = (len(good) - 1) * 8 + (good[-1] & 7) if (good[-1] & 7) < 6 else (len(good) - 2) * 8 + (good[-1] & 7)
    w.bits = w.bits[:total - 1]
    out = {"truncated": w.finish()}
    w = BitWriter()
    w.pair(0, 97)
    w.pair(1, 98)
    w.pair(3, 99)                                       # pair 2 names phrase 3
    out["id_ahead"] = w.finish()
    w = BitWriter()
    w.pair(0, 97)
    w.pair(1, 98, id_width=33)
    out["id_33_bits"] = w.finish()
    return out


@pytest.mark.parametrize("kind", ["truncated", "id_ahead", "id_33_bits"])
def test_malformed_streams(gpu_ctx, kind):
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.lz78_decompress(_malformed()[kind])
    assert e.value.status == ERR_ARG
    _valid_after(gpu_ctx)


def _sequential_length(stream):
    """the pairs read one after another (the reference's loop): the text length, or None for a malformed stream"""
    bits, total = M.stream_bits(stream)
    x, k, lengths = 0, 0, []
    while x < total:
        p = M.pair_at(bits, total, x)
        if p is None or p[1] > k:
            return None
        lengths.append(1 + (lengths[p[1] - 1] if p[1] else 0))
        x, k = p[0], k + 1
    return sum(lengths)


def test_random_bytes(gpu_ctx):
    """random streams: refused with TDC_GPU_ERR_ARG exactly where the sequential reading finds a malformed pair"""
    rng = np.random.default_rng(4)
    for _ in range(10):
        s = rng.integers(0, 256, 1 << 14, dtype=np.uint8).tobytes()
        want = _sequential_length(s)
        if want is None:
            with pytest.raises(T.TdcGpuError) as e:
                gpu_ctx.lz78_decompress(s)
            assert e.value.status == ERR_ARG
        elif want > 2**32 - 2:
            with pytest.raises(T.TdcGpuError) as e:
                gpu_ctx.lz78_decompress(s)
            assert e.value.status == ERR_TOO_LARGE
        else:
            assert len(gpu_ctx.lz78_decompress(s)[0]) == want
    _valid_after(gpu_ctx)


def test_coder_must_be_gamma(gpu_ctx):
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.lz78_decompress(O.lz78_gamma_compress(b"abc"), coder=T.CODER_HUFF)
    assert e.value.status == ERR_UNSUPPORTED


def test_oversized_claim(gpu_ctx):
    """93 000 pairs that each extend the previous phrase claim ~4.3e9 bytes: refused before the text is allocated"""
    w = BitWriter()
    for k in range(93000):
        w.pair(k, 97)
    stream = w.finish()
    t0 = time.perf_counter()
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.lz78_decompress(stream)
    assert e.value.status == ERR_TOO_LARGE
    assert time.perf_counter() - t0 < 1.0
    _valid_after(gpu_ctx)


def test_configs3_lz78_1e9_decode(gpu_ctx):
    """BASELINE configs[3] at full size: the device stream against the committed oracle hash, then decoded on the device (more than
    2^32 bit positions: several segments, 64-bit positions)"""
    g = load_json("oracle_fullsize.json")["lz78_1e9"]
    data = T.gen_english(10**9, 42)
    stream, _ = gpu_ctx.lz78_compress(data)
    del data
    assert len(stream) == g["size"] and sha256(stream) == g["sha256"]
    assert len(stream) * 8 > 2**32
    text, st = gpu_ctx.lz78_decompress(stream)
    assert len(text) == 10**9
    assert sha256(text) == g["text_sha256"]


def test_cli_dec_gpu(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    data = _ascii_tail(T.gen_english(1 << 20, 12).tobytes())
    f = tmp_path / "in.txt"
    f.write_bytes(data)
    comp = tmp_path / "in.tdc"
    r = subprocess.run([TDC, "-a", "lz78(coder=gamma,dec=gpu)", "-o", str(comp), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blob = comp.read_bytes()
    head, payload = blob.split(b"%", 1)
    assert head == b"lz78(coder=gamma,dec=gpu)" and payload == O.lz78_gamma_compress(data)
    out = tmp_path / "out.gpu"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(comp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    host_in = tmp_path / "plain.tdc"
    host_in.write_bytes(b"lz78(coder=gamma)%" + payload)
    out_host = tmp_path / "out.host"
    r = subprocess.run([TDC, "-d", "-o", str(out_host), str(host_in)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == out_host.read_bytes() == data
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert "lz78(coder=gamma, dec=gpu)" in r.stdout


def test_more_than_2_32_scatter_work_items():
    """537 M phrases: the reference scatter has 8 work-items per factor, more than 2^32 in all (the dispatch grid is 32-bit: the launch
    is capped and loops).  Stream built directly: 128 one-byte phrases (0, c), then pairs (id in 64..127, c in 128..255) of exactly 32 bits,
    each phrase two bytes -- text[2j + 128], text[2j + 129] = 127 + id_j, c_j."""
    head = BitWriter()
    for c in range(128, 256):
        head.pair(0, c)                                   # 20 bits each: 2 560 bits, byte aligned
    assert len(head.bits) % 8 == 0
    zb = (1 << 29) + (1 << 20)
    assert 8 * (128 + zb) > 2**32
    j = np.arange(zb, dtype=np.uint32)
    ids = np.uint32(64) + ((j * np.uint32(2654435761)) >> np.uint32(7)) % np.uint32(64)      # (any ids in 64..127 and chars in 128..255)
    chars = np.uint32(128) + ((j * np.uint32(40503)) >> np.uint32(3)) % np.uint32(128)
    words = (np.uint32(1 << 24) | (ids << np.uint32(17)) | np.uint32(1 << 8) | chars).astype(">u4")
    del j
    stream = np.concatenate([np.packbits(np.array(head.bits, dtype=np.uint8)), words.view(np.uint8), np.zeros(1, dtype=np.uint8)])
    del words
    want = np.empty(128 + 2 * zb, dtype=np.uint8)
    want[:128] = np.arange(128, 256, dtype=np.uint8)
    want[128::2] = (127 + ids).astype(np.uint8)
    want[129::2] = chars.astype(np.uint8)
    del ids, chars
    out = np.empty(len(want), dtype=np.uint8)
    with T.Context(0) as ctx:
        n, st = ctx.lz78_decompress_into(stream, out)
    assert n == len(want) and st["phrases"] == 128 + zb
    assert np.array_equal(out, want)


def test_text_of_2_32_minus_2_bytes():
    """a^(2^32 - 2), the largest text the decoder takes (92 681 phrases a^k and a left-over a^37 073): the unchunked copy pass covers
    more than 2^32 - 256 positions (capped launch), into a pageable buffer; one byte more is TDC_GPU_ERR_TOO_LARGE"""
    def runs_stream(n):
        w = BitWriter()
        k = 0
        while (k + 1) * (k + 2) // 2 <= n:
            w.pair(k, 97)                                 # phrase k + 1 = a^(k + 1)
            k += 1
        r = n - k * (k + 1) // 2
        if r:
            w.pair(r - 1, 97)                             # left-over a^r
        return w.finish()

    n = 2**32 - 2
    out = np.zeros(n, dtype=np.uint8)
    with T.Context(0) as ctx:
        got, st = ctx.lz78_decompress_into(runs_stream(n), out)
        assert got == n and st["phrases"] == 92681 + 1
        assert int(np.count_nonzero(out != 97)) == 0
        with pytest.raises(T.TdcGpuError) as e:
            ctx.lz78_decompress(runs_stream(n + 1))
        assert e.value.status == ERR_TOO_LARGE
