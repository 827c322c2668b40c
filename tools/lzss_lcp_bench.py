"""Timing of lzss_lcp(coder=huff | bit | gamma | delta | ascii): the stage times of one compression per coder (suffix array, factorizer,
encoder, in all), and decompression of the same stream on the device (option dec_parse = 2, pinned buffers) against the host loop
(tdc_lzss_decode) in the same run.
Usage: python3 tools/lzss_lcp_bench.py [english|dna] [N] [reps]     (output: profiles/lzss_lcp_<gen>_<N>.txt by redirection)"""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

gen = sys.argv[1] if len(sys.argv) > 1 else "english"
N = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1 << 28
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
CODERS = (("huff", T.CODER_HUFF), ("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA), ("delta", T.CODER_DELTA), ("ascii", T.CODER_ASCII))

data = (T.gen_english(N - 1, 42) if gen == "english" else T.gen_dna(N - 1, 7)).tobytes()      # no 0x00 / 0xFF: escaping adds the sentinel only
text = np.frombuffer(data + b"\0", dtype=np.uint8)
del data
print("lzss_lcp, %s, text of %d B, threshold 3" % (gen, len(text)), flush=True)


def host_decode_time(a, cid, n):
    """tdc_lzss_decode into a buffer of the known size (one pass)"""
    out = np.empty(n, dtype=np.uint8)
    sz = ctypes.c_size_t()
    L = T._native.load()
    t0 = time.perf_counter()
    rc = L.tdc_lzss_decode(a.ctypes.data_as(ctypes.c_void_p), len(a), cid, out.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(sz))
    t = time.perf_counter() - t0
    assert rc == 0 and sz.value == n, (rc, sz.value)
    return t, out


with T.Context(0, options={"dec_parse": 2}) as ctx:
    h_text = T.PinnedBuffer(len(text)); h_text.a[:] = text
    for name, cid in CODERS:
        h_out = T.PinnedBuffer(T.lzss_lcp_bound(len(text), cid))
        best = None
        for _ in range(reps):
            ln, st = ctx.lzss_lcp_compress_into(h_text, len(text), h_out, 3, cid)
            if best is None or st["ms_total"] < best["ms_total"]:
                best = st
        print("compress(coder=%s): stream %d B (bound %d), %d factors; ms_sa %.2f  ms_factorize %.2f  ms_encode %.2f  ms_total %.2f  = %.2f GB/s"
              % (name, ln, h_out.nbytes, best["factors"], best["ms_sa"], best["ms_factorize"], best["ms_encode"], best["ms_total"],
                 len(text) / 1e6 / best["ms_total"]), flush=True)
        h_in = T.PinnedBuffer(ln); h_in.a[:] = h_out.a[:ln]
        h_back = T.PinnedBuffer(len(text))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            n, dst = ctx.lzss_lcp_decompress_into(h_in, h_back, cid)
            ts.append(time.perf_counter() - t0)
        ok = n == len(text) and bool((h_back.a[:n] == text).all())
        td = min(ts[1:]) if reps > 1 else ts[0]
        th, out = host_decode_time(h_in.a[:ln].copy(), cid, len(text))
        print("decompress(coder=%s): device_parse %d, %d rounds, best %.1f ms = %.2f GB/s of text, correct %s (all: %s); host loop %.1f ms, correct %s: %.1fx"
              % (name, dst["device_parse"], dst["rounds"], td * 1e3, len(text) / 1e9 / td, ok, " ".join("%.1f" % (x * 1e3) for x in ts),
                 th * 1e3, bool((out == text).all()), th / td), flush=True)
        del out
        h_out.free(); h_in.free(); h_back.free()
    h_text.free()
