"""GPU tests of the device decoder of lzss streams (tdc_gpu_lzss_sw_decompress{,_into}; lzss_sw_decode.hip): bit, gamma and delta streams
of the device compressor and of the model's coders (tests/models/lzss_sw.py) back to their texts with small and with default segments,
hand-built bit token lists around text positions 2^k, the smallest streams, the path option dec_parse picks, the refusals, damaged
streams against the host loop's verdict (tdc_lzss_sw_decode), the facade and the `tdc` round trip."""
import functools
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests import lzss_sw_damage as D
from tests.models import lzss_sw as M
from tests.models import lzss_sw_decode as MD

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CID = {"ascii": T.CODER_ASCII, "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
N = 70001


@pytest.fixture(scope="module")
def seg_ctx():
    """every stream on the device, in segments of 4096 bit positions"""
    with T.Context(0, options={"dec_parse": 2, "dec_seg": 4096}) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def dev_ctx():
    """every stream on the device, default segments"""
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        yield ctx


@functools.lru_cache(maxsize=None)
def text(kind, n=N):
    return (T.gen_english(n, 42) if kind == "english" else T.gen_dna(n, 42)).tobytes()


@functools.lru_cache(maxsize=None)
def truncates(kind, w, t):
    return M.truncates(text(kind), w, t)


def device(ctx, stream, coder, w):
    """(status, text, stats) of tdc_gpu_lzss_sw_decompress"""
    try:
        out, st = ctx.lzss_sw_decompress(stream, w, CID[coder])
        return 0, out, st
    except T.TdcGpuError as e:
        return e.status, None, None


def host(stream, coder, w):
    try:
        return 0, T.lzss_sw_decode(stream, CID[coder], w)
    except T.TdcGpuError as e:
        return e.status, None


@pytest.mark.parametrize("w,t", [(16, 3), (1, 1), (5, 2), (4096, 3)])
@pytest.mark.parametrize("coder", MD.CODERS)
def test_segments(seg_ctx, coder, w, t):
    for kind in ("english", "dna"):
        data = text(kind)
        if coder == "bit" and w == 5:                                                    # (3 bits for lengths of up to 2w - 1 = 9)
            assert not truncates(kind, w, t)
        stream, _ = seg_ctx.lzss_sw_compress(data, w, t, CID[coder])
        status, out, st = device(seg_ctx, stream, coder, w)
        assert status == 0 and st["device_parse"] == 1
        assert out == data, (kind, coder, w, t)
        assert st["factors"] == MD.factor_tokens(stream, coder, w) == len(T.lzss_sw_factors(data, w, t)[0])
        assert st["rounds"] >= 1
        buf = np.full(len(data), 0xA5, dtype=np.uint8)
        n, st2 = seg_ctx.lzss_sw_decompress_into(stream, buf, w, CID[coder])
        assert n == len(data) and buf.tobytes() == data and st2["factors"] == st["factors"] and st2["device_parse"] == 1
        short = np.full(len(data) - 1, 0xA5, dtype=np.uint8)
        with pytest.raises(T.TdcGpuError) as e:
            seg_ctx.lzss_sw_decompress_into(stream, short, w, CID[coder])
        assert e.value.status == ERR_OOM and e.value.required == len(data) and (short == 0xA5).all()


@pytest.mark.parametrize("case", MD.BOUNDARY_CASES)
def test_power_of_two_cuts_with_default_segments(dev_ctx, case):
    toks = MD.boundary_tokens(case, range(12, 19), n=300000)
    data = MD.text_of(toks)
    assert len(data) == 300000
    for w in (16, 4096):
        stream = M.encode(toks, "bit", w)
        status, out, st = device(dev_ctx, stream, "bit", w)
        assert status == 0 and st["device_parse"] == 1
        assert out == data, (case, w)
        assert st["factors"] == sum(1 for tok in toks if tok[1] is not None)


@pytest.mark.parametrize("coder", MD.CODERS)
def test_small_streams(seg_ctx, dev_ctx, coder):
    foreign = [(i, None, (7 * i) % 251) for i in range(1000)] + [(1000, 0, 20), (1020, 1, 5), (1025, None, 3), (1026, 2, 31), (1057, 1056, 4)]
    for ctx in (seg_ctx, dev_ctx):
        assert device(ctx, b"", coder, 16)[:2] == (0, b"")
        assert device(ctx, M.encode([], coder, 16), coder, 16)[:2] == (0, b"")           # the empty stream: the terminator alone
        status, out, st = device(ctx, M.encode([(0, None, 113)], coder, 16), coder, 16)
        assert (status, out) == (0, b"q") and st["device_parse"] == 1 and st["factors"] == 0
        run = b"a" * 5000
        stream = M.encode(M.parse(run, 16, 3), coder, 16)                                # a literal, then factors of distance 1
        status, out, st = device(ctx, stream, coder, 16)
        assert (status, out) == (0, run) and st["rounds"] >= 1 and st["factors"] == len(M.factors(run, 16, 3))
        stream = M.encode([(0, None, 98)] + [(1 + 31 * i, 31 * i, 31) for i in range(200)], coder, 16)   # one chain through every byte
        assert device(ctx, stream, coder, 16)[:2] == (0, b"b" * 6201)
        stream = M.encode(foreign, coder, 16)                                            # distances far above the window, up to p
        status, out, st = device(ctx, stream, coder, 16)
        assert (status, out) == (0, MD.text_of(foreign)) and st["factors"] == 4
        stream = M.encode([(0, None, 97), (1, 0, 0), (1, None, 98)], coder, 16)          # a factor of length 0 decodes to nothing
        assert device(ctx, stream, coder, 16)[:2] == (0, b"ab")


@pytest.mark.parametrize("coder", ("gamma", "delta"))
def test_a_small_stream_that_expands_far_beyond_the_arena(coder):
    """64 literals and four factors of 2^24 bytes each at distance 64: a stream of some hundred bytes whose text pass does not fit the
    arena the parse took, so the token records move into a larger one before the factor list is built"""
    unit = bytes(range(33, 97))
    toks = [(i, None, unit[i]) for i in range(64)] + [(64 + (i << 24), (i << 24), 1 << 24) for i in range(4)]
    n = 64 + (4 << 24)
    stream = M.encode(toks, coder, 16)
    with T.Context(0, options={"dec_parse": 2}) as ctx:                                  # a fresh context: its arena starts empty
        status, out, st = device(ctx, stream, coder, 16)
        assert status == 0 and st["device_parse"] == 1 and st["factors"] == 4
        assert len(out) == n and out == (unit * (n // 64 + 1))[:n]
        assert device(ctx, M.encode([(0, None, 113)], coder, 16), coder, 16)[:2] == (0, b"q")


def test_default_options_pick_the_path(gpu_ctx):
    data = text("english", 2 << 20)
    for coder in MD.CODERS:
        stream, _ = gpu_ctx.lzss_sw_compress(data, 16, 3, CID[coder])
        assert len(stream) >= 1 << 20
        out, st = gpu_ctx.lzss_sw_decompress(stream, 16, CID[coder])
        assert out == data and st["device_parse"] == 1 and st["factors"] > 0
        small, _ = gpu_ctx.lzss_sw_compress(text("english"), 16, 3, CID[coder])
        out, st = gpu_ctx.lzss_sw_decompress(small, 16, CID[coder])
        assert out == text("english") and st["device_parse"] == 0
    stream, _ = gpu_ctx.lzss_sw_compress(data, 16, 3, T.CODER_ASCII)
    assert len(stream) >= 1 << 20
    out, st = gpu_ctx.lzss_sw_decompress(stream, 16, T.CODER_ASCII)
    assert out == data and st["device_parse"] == 0


def test_ascii_keeps_the_host_loop(dev_ctx):
    data = text("english")
    stream, _ = dev_ctx.lzss_sw_compress(data, 16, 3, T.CODER_ASCII)
    out, st = dev_ctx.lzss_sw_decompress(stream, 16, T.CODER_ASCII)
    assert out == data and st["device_parse"] == 0 and st["factors"] == 0


def test_refusals(dev_ctx):
    good = M.encode(M.parse(b"abcabcabcabc", 16, 3), "bit", 16)
    for coder in (T.CODER_HUFF, T.CODER_ARITH, T.CODER_SLE, 99):
        with pytest.raises(T.TdcGpuError) as e:
            dev_ctx.lzss_sw_decompress(good, 16, coder)
        assert e.value.status == ERR_UNSUPPORTED
    with pytest.raises(T.TdcGpuError) as e:
        dev_ctx.lzss_sw_decompress(good, 0, T.CODER_BIT)
    assert e.value.status == ERR_ARG
    assert dev_ctx.lzss_sw_decompress(M.encode(M.parse(b"abcabcabcabc", 16, 3), "gamma", 16), 0, T.CODER_GAMMA)[0] == b"abcabcabcabc"
    for coder in ("gamma", "delta"):
        big = M.encode([(0, None, 97)] + [(1 + (i << 31), (i << 31), 1 << 31) for i in range(3)], coder, 16)    # 1 + 3 * 2^31 bytes
        with pytest.raises(T.TdcGpuError) as e:
            dev_ctx.lzss_sw_decompress(big, 16, CID[coder])
        assert e.value.status == ERR_TOO_LARGE
        buf = np.zeros(16, dtype=np.uint8)
        with pytest.raises(T.TdcGpuError) as e:
            dev_ctx.lzss_sw_decompress_into(big, buf, 16, CID[coder])
        assert e.value.status == ERR_TOO_LARGE
        assert dev_ctx.lzss_sw_decompress(good, 16, T.CODER_BIT)[0] == b"abcabcabcabc"    # the context is usable afterwards
    for toks in ([(0, None, 97), (1, 1, 2)], [(0, 0, 3)]):                               # distance 0, a factor in front of any text
        for coder in MD.CODERS:
            assert device(dev_ctx, M.encode(toks, coder, 16), coder, 16)[0] == ERR_ARG
    assert device(dev_ctx, M.encode([(0, None, 97), (1, -1, 2)], "gamma", 16), "gamma", 16)[0] == ERR_ARG     # distance 2 above a text of 1


@pytest.mark.parametrize("coder", MD.CODERS)
def test_damaged_streams_get_the_host_loops_verdict(seg_ctx, dev_ctx, coder):
    streams = D.damaged_streams(coder)
    w = D.WINDOW
    for ctx in (seg_ctx, dev_ctx):
        for name, s in streams:
            want = host(s, coder, w)
            status, out, _ = device(ctx, s, coder, w)
            if coder != "bit" and MD.over_cap(s, coder, w) and status == ERR_ARG:
                continue                                                                 # a field above a device cap: the licensed refusal
            assert (status == 0, out) == (want[0] == 0, want[1]), (name, status, want[0])
        assert streams[-1][0] == "good" and device(ctx, streams[-1][1], coder, w)[:2] == (0, D.TEXT)    # ... and a good stream afterwards


def test_facade_and_command_line(dev_ctx, tmp_path):
    data = text("english", 30000) + b"\x00\xff" + b"a" * 300
    for coder in MD.CODERS + ("ascii",):
        z = T.LZSSSlidingWindowCompressor(dev_ctx, coder, window=64, threshold=2, dec="gpu")
        s = z.compress(data)
        assert z.decompress(s) == data
        assert T.LZSSSlidingWindowCompressor(None, coder, window=64, threshold=2).decompress(s) == data
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    src = tmp_path / "in.txt"
    src.write_bytes(data)
    # (the file is small: every stream on the device, and the decoder's log says that it ran)
    env = dict(os.environ, TDC_GPU_DEBUG_KNOBS="1", TDC_GPU_DEC_PARSE="2", TDC_GPU_DEC_LOG="1")
    payloads = []
    for algo in ("lzss(coder=gamma,dec=gpu)", "lzss(coder=gamma)"):
        packed, back = tmp_path / "p.tdc", tmp_path / "p.out"
        r = subprocess.run([TDC, "-a", algo, "-f", "-o", str(packed), str(src)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        blob = packed.read_bytes()
        assert blob.startswith(algo.encode() + b"%")                                     # the header is written as given
        payloads.append(blob[len(algo) + 1:])
        r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(packed)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data
        assert ("lzss decode:" in r.stderr) == ("dec=gpu" in algo)                       # tdc -d of a dec=gpu file uses the device
    assert payloads[0] == payloads[1]
