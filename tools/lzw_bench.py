"""Timing of lzw(coder=bit | gamma): compression (host parse and device pack separately, beside lz78(coder=gamma) on the same text),
decompression on the device (option dec_parse = 2) against the host loop (tdc_lzw_decode, the facade's loop) on the same stream in the
same run, one call's stage times (option dec_log, on stderr), and a sweep over small texts for the dec_parse = 1 threshold.
Usage: python3 tools/lzw_bench.py [english|dna] [N] [reps] [--sweep]     (output: profiles/lzw_<gen>_<N>.txt by redirection)"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

args = [a for a in sys.argv[1:] if not a.startswith("--")]
gen = args[0] if len(args) > 0 else "english"
N = int(float(args[1])) if len(args) > 1 else 1 << 28
reps = int(args[2]) if len(args) > 2 else 4
CODERS = (("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA))


def make(n):
    return T.gen_english(n, 42) if gen == "english" else T.gen_dna(n, 7)


def best(fn, k):
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return (min(ts[1:]) if k > 1 else ts[0]), ts, r


def host_decode_time(a, cid, n):
    """tdc_lzw_decode into a buffer of the known size (one pass)"""
    out = np.empty(max(n, 1), dtype=np.uint8)
    sz = ctypes.c_size_t()
    L = T._native.load()
    t0 = time.perf_counter()
    rc = L.tdc_lzw_decode(a.ctypes.data_as(ctypes.c_void_p), len(a), cid, out.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(sz))
    t = time.perf_counter() - t0
    assert rc == 0 and sz.value == n
    return t, out


def device_decode_time(ctx, a, cid, k):
    def call():
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        c, r = ctypes.c_uint64(), ctypes.c_uint32()
        rc = ctx._L.tdc_gpu_lzw_decompress(ctx._h, a.ctypes.data_as(ctypes.c_void_p), len(a), cid, ctypes.byref(p), ctypes.byref(n),
                                           ctypes.byref(c), ctypes.byref(r))
        assert rc == 0, rc
        return p, n.value, c.value, r.value
    ts, res = [], None
    for _ in range(k):
        t0 = time.perf_counter()
        res = call()
        ts.append(time.perf_counter() - t0)
        if _ < k - 1:
            ctx._L.tdc_gpu_free(res[0])
    return (min(ts[1:]) if k > 1 else ts[0]), ts, res


if "--sweep" in sys.argv:
    print("dec_parse = 1 threshold sweep (%s): stream bytes, device ms (best of 5 after a warm-up), host loop ms" % gen)
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        for n in (1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 22):
            data = make(n)
            for name, cid in CODERS:
                stream, _ = ctx.lzw_compress(data, cid)
                a = np.frombuffer(stream, dtype=np.uint8)
                td, _, res = device_decode_time(ctx, a, cid, 6)
                ctx._L.tdc_gpu_free(res[0])
                th = min(host_decode_time(a, cid, n)[0] for _ in range(3))
                print("  text %8d  %-5s stream %8d B   device %8.3f ms   host %8.3f ms   %s" % (n, name, len(stream), td * 1e3, th * 1e3,
                                                                                              "device" if td < th else "host"), flush=True)
    sys.exit(0)

data = make(N)
want = data.tobytes()
t0 = time.perf_counter()
codes = T.lzw_factors(data)
t_parse = time.perf_counter() - t0
t0 = time.perf_counter()
ids, _ = T.lz78_factors(data)
t_parse78 = time.perf_counter() - t0
print("%s %d B: lzw host parse %.2f s = %.1f MB/s (%d codes); lz78 host parse %.2f s = %.1f MB/s (%d phrases)"
      % (gen, N, t_parse, N / 1e6 / t_parse, len(codes), t_parse78, N / 1e6 / t_parse78, len(ids)), flush=True)
del ids
streams = {}
with T.Context(0) as ctx:
    for name, cid in CODERS:
        t0 = time.perf_counter()
        stream, st = ctx.lzw_compress(data, cid)
        t = time.perf_counter() - t0
        streams[name] = stream
        print("lzw_compress(coder=%s): %.2f s in all; stream %d B; on the device: upload %.2f ms, pack %.2f ms, download %.2f ms"
              % (name, t, len(stream), st["ms_h2d"], st["ms_encode"], st["ms_d2h"]), flush=True)
    if want[-1:] < b"\x80":
        t0 = time.perf_counter()
        s78, st = ctx.lz78_compress(data)
        print("lz78_compress(coder=gamma): %.2f s in all; stream %d B; pack %.2f ms" % (time.perf_counter() - t0, len(s78), st["ms_encode"]), flush=True)
        del s78
del data

for name, cid in CODERS:
    a = np.frombuffer(streams[name], dtype=np.uint8)
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        t, ts, res = device_decode_time(ctx, a, cid, reps)
        ok = res[1] == N and ctypes.string_at(res[0], res[1]) == want
        ctx._L.tdc_gpu_free(res[0])
        print("tdc_gpu_lzw_decompress(coder=%s, pageable): %d codes, %d rounds, best %.1f ms = %.2f GB/s of text, correct %s (all: %s)"
              % (name, res[2], res[3], t * 1e3, N / 1e9 / t, ok, " ".join("%.1f" % (x * 1e3) for x in ts)), flush=True)
        h_in = T.PinnedBuffer(len(a)); h_in.a[:] = a
        h_out = T.PinnedBuffer(N)
        tp, tsp, r = best(lambda: ctx.lzw_decompress_into(h_in, h_out, cid), reps)
        ok = r[0] == N and h_out.a[:N].tobytes() == want
        print("tdc_gpu_lzw_decompress_into(coder=%s, pinned buffers): best %.1f ms = %.2f GB/s of text, correct %s (all: %s)"
              % (name, tp * 1e3, N / 1e9 / tp, ok, " ".join("%.1f" % (x * 1e3) for x in tsp)), flush=True)
        print("stage times of one more call (option dec_log, stderr):", flush=True)
        ctx.set_option("dec_log", 1)
        ctx.lzw_decompress_into(h_in, h_out, cid)
        ctx.set_option("dec_log", 0)
        h_in.free(); h_out.free()
    th, out = host_decode_time(a, cid, N)
    print("tdc_lzw_decode(coder=%s), the host loop: %.1f ms = %.3f GB/s of text, correct %s; device decode %.1fx faster (pinned: %.1fx)"
          % (name, th * 1e3, N / 1e9 / th, out.tobytes() == want, th / t, th / tp), flush=True)
    del out
