"""Timing of lzss (the sliding-window factorizer, lzss_sw.hip): the device call per coder with its stage times (ms_factorize = match
kernel, orbit and token list; ms_encode = cost pass, scan and pack), pinned buffers on both sides, beside tdc_lzss_sw_factors -- the
same parse on one host core -- on the same text in the same run.  Every stream is decoded back by tdc_lzss_sw_decode, the host loop;
the bit, gamma and delta streams also by the device decoder (lzss_sw_decode.hip: option dec_parse = 2, pinned stream and output; wall
clock around the call, which returns with its streams idle), with the ratio of the two.  One more decode per coder on a context with
dec_log = 1 prints the decoder's stage times, its segments and the bit positions next() was evaluated for (stderr).
Usage: python3 tools/lzss_sw_bench.py [english|dna|run] [N] [WINDOW] [reps]     (output by redirection, stderr included:
profiles/lzss_sw_<text>_<N>.txt; the decode lines alone: profiles/lzss_sw_decode_<text>_<N>.txt)"""
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

with T.Context(0, options={"dec_parse": 2}) as ctx, T.Context(0, options={"dec_parse": 2, "dec_log": 1}) as log_ctx:
    back_buf = T.PinnedBuffer(N)
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
            if cid != T.CODER_ASCII:
                stream = out.a[:n]                            # (a view of the pinned buffer)
                dec_ms = []
                for _ in range(reps + 1):                     # the first call grows the arena and loads the kernels
                    t0 = time.perf_counter()
                    m, dst = ctx.lzss_sw_decompress_into(stream, back_buf, W, cid)
                    dec_ms.append((time.perf_counter() - t0) * 1e3)
                ok = m == N and np.array_equal(back_buf.a[:m], text.a) and dst["device_parse"] == 1
                fast = min(dec_ms[1:])
                print("decompress(coder=%s): device %.2f ms = %.2f GB/s of text (first call %.1f ms, then: %s); host loop on the same stream %.1f ms"
                      " = %.1fx the device; %d factors, %d rounds, correct %s"
                      % (name, fast, N / fast / 1e6, dec_ms[0], " ".join("%.2f" % x for x in dec_ms[1:]), t_dec * 1e3, t_dec * 1e3 / fast,
                         dst["factors"], dst["rounds"], ok), flush=True)
                sys.stdout.flush()
                print("decompress(coder=%s): stages (dec_log = 1: every stage waits for the device)" % name, file=sys.stderr, flush=True)
                log_ctx.lzss_sw_decompress_into(stream, back_buf, W, cid)
                sys.stderr.flush()
        out.free()
    back_buf.free()
text.free()
