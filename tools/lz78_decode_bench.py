"""Decompression timing of lz78(coder=gamma) streams: tdc_gpu_lz78_decompress (device parse, pageable output), the same into pinned
buffers (tdc_gpu_lz78_decompress_into), and the host loop of the C++ facade (`tdc -d` without dec=gpu) on the same stream.
Usage: python3 tools/lz78_decode_bench.py [english|dna] [N] [reps]"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gen = sys.argv[1] if len(sys.argv) > 1 else "english"
N = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1 << 28
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
data = T.gen_english(N, 42) if gen == "english" else T.gen_dna(N, 7)
with T.Context(0) as ctx:
    t0 = time.perf_counter()
    stream, cst = ctx.lz78_compress(data)
    tc = time.perf_counter() - t0
print("%s %d B: stream %d B (%d bit positions), %d phrases; lz78_compress %.1f s" % (gen, N, len(stream), len(stream) * 8, cst["factors"], tc), flush=True)
want = data.tobytes()
del data

with T.Context(0) as ctx:
    a = np.frombuffer(stream, dtype=np.uint8)
    ts = []
    for i in range(reps):                          # the C ABI call alone (the binding's copy into a Python bytes object is not the library's time)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        ph, r = ctypes.c_uint64(), ctypes.c_uint32()
        t0 = time.perf_counter()
        rc = ctx._L.tdc_gpu_lz78_decompress(ctx._h, a.ctypes.data_as(ctypes.c_void_p), len(a), T.CODER_GAMMA, ctypes.byref(p), ctypes.byref(n),
                                            ctypes.byref(ph), ctypes.byref(r))
        ts.append(time.perf_counter() - t0)
        assert rc == 0, rc
        if i == reps - 1:
            ok = n.value == N and ctypes.string_at(p, n.value) == want
        ctx._L.tdc_gpu_free(p)
    t = min(ts[1:]) if reps > 1 else ts[0]
    print("tdc_gpu_lz78_decompress (pageable): %d phrases, %d rounds, best %.1f ms = %.2f GB/s of text, correct %s (all: %s)"
          % (ph.value, r.value, t * 1e3, N / 1e9 / t, ok, " ".join("%.1f" % (x * 1e3) for x in ts)), flush=True)
    t_dev = t

    h_in = T.PinnedBuffer(len(stream)); h_in.a[:] = a
    h_out = T.PinnedBuffer(N)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        n, st = ctx.lz78_decompress_into(h_in, h_out)
        ts.append(time.perf_counter() - t0)
    ok = n == N and h_out.a[:n].tobytes() == want
    t = min(ts[1:]) if reps > 1 else ts[0]
    print("tdc_gpu_lz78_decompress_into (pinned buffers): best %.1f ms = %.2f GB/s of text, correct %s (all: %s)"
          % (t * 1e3, N / 1e9 / t, ok, " ".join("%.1f" % (x * 1e3) for x in ts)), flush=True)
    h_in.free(); h_out.free()

# the host loop of the C++ facade on the same stream (one run: file in, file out, as `tdc -d` does it)
tdc = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
with tempfile.TemporaryDirectory() as d:
    f, o = os.path.join(d, "s.tdc"), os.path.join(d, "s.out")
    with open(f, "wb") as fh:
        fh.write(b"lz78(coder=gamma)%" + stream)
    t0 = time.perf_counter()
    r = subprocess.run([tdc, "-d", "-f", "-o", o, f], capture_output=True, text=True)
    th = time.perf_counter() - t0
    with open(o, "rb") as fh:
        ok = r.returncode == 0 and fh.read() == want
print("tdc -d, host loop (file to file): %.1f ms = %.3f GB/s of text, correct %s; device decode %.1fx faster"
      % (th * 1e3, N / 1e9 / th, ok, th / t_dev), flush=True)
