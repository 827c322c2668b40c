"""Timing of lzss (the sliding-window factorizer, lzss_sw.hip): the device call per coder with its stage times (ms_factorize = match
kernel, orbit and token list; ms_encode = cost pass, scan and pack), pinned buffers on both sides, beside tdc_lzss_sw_factors -- the
same parse on one host core -- on the same text in the same run.  Every stream is decoded back by tdc_lzss_sw_decode.
Usage: python3 tools/lzss_sw_bench.py [english|dna|run] [N] [WINDOW] [reps]     (output: profiles/lzss_sw_<text>_<N>.txt by redirection)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

gen = sys.argv[1] if len(sys.argv) > 1 else "english"
N = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1 << 28
W = int(sys.argv[3]) if len(sys.argv) > 3 else 16
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 4
THRESHOLD = 3
CODERS = (("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA), ("delta", T.CODER_DELTA), ("ascii", T.CODER_ASCII))

text = T.PinnedBuffer(N)
if gen == "english":
    T.gen_english(N, 42, out=text.a)
elif gen == "dna":
    T.gen_dna(N, 7, out=text.a)
else:
    text.a[:] = ord("a")                                    # a^n: every lane stops at its first candidate
want = text.a.tobytes()
print("lzss, %s, text of %d B, window %d, threshold %d" % (gen, N, W, THRESHOLD))

t0 = time.perf_counter()
hp, hs, hl = T.lzss_sw_factors(text.a, W, THRESHOLD)
t_host = time.perf_counter() - t0
print("host parse (tdc_lzss_sw_factors, one core): %d factors, longest %d, %.1f ms = %.3f GB/s"
      % (len(hp), int(hl.max()) if len(hl) else 0, t_host * 1e3, N / t_host / 1e9))

with T.Context(0) as ctx:
    t0 = time.perf_counter()
    dp, ds, dl = ctx.lzss_sw_factorize(text.a, W, THRESHOLD)
    t_fact = time.perf_counter() - t0
    same = np.array_equal(dp, hp) and np.array_equal(ds, hs) and np.array_equal(dl, hl)
    print("device factorize entry (first call, pageable result): %.1f ms, equal to the host parse: %s" % (t_fact * 1e3, same))
    for name, cid in CODERS:
        bound = T.lzss_sw_bound(N, W, cid)
        out = T.PinnedBuffer(bound)
        best, all_ms = None, []
        for _ in range(reps):
            try:
                n, st = ctx.lzss_sw_compress_into(text, N, out, W, THRESHOLD, cid)
            except T.TdcGpuError as e:
                print("compress(coder=%s): refused (%s)" % (name, e))
                best = None
                break
            all_ms.append(st["ms_total"])
            if best is None or st["ms_total"] < best["ms_total"]:
                best = st
        if best is not None:
            t0 = time.perf_counter()
            back = T.lzss_sw_decode(out.a[:n], cid, W)
            t_dec = time.perf_counter() - t0
            print("compress(coder=%s): stream %d B (bound %d), %d factors; ms_h2d %.2f  ms_factorize %.2f  ms_encode %.2f  ms_d2h %.2f  ms_total %.2f"
                  "  = %.2f GB/s, factorize alone %.2f GB/s = %.1fx the host parse (all: %s); host decode %.1f ms, correct %s"
                  % (name, n, bound, best["factors"], best["ms_h2d"], best["ms_factorize"], best["ms_encode"], best["ms_d2h"], best["ms_total"],
                     N / best["ms_total"] / 1e6, N / best["ms_factorize"] / 1e6, t_host * 1e3 / best["ms_factorize"],
                     " ".join("%.1f" % x for x in all_ms), t_dec * 1e3, back == want), flush=True)
        out.free()
text.free()
