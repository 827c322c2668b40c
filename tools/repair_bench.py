"""Timing of repair (the Re-Pair grammar built on the device, repair.hip): the device call at several max_rules with its stage times
(ms_factorize = the grammar: first count and all rounds; ms_encode = cost pass, scan and pack) and its rounds -- mean, first, last, and
the tie rounds against the others --, pinned buffers on both sides, beside tdc_repair_grammar -- the same loop on one host core -- on the
same text at the largest max_rules it is expected to finish within --host-seconds.  Every stream is decoded back by tdc_repair_decode.
A round is timed on the host clock from its read-back to the next one's (no synchronisation is added for it).
Usage: python3 tools/repair_bench.py [english|dna] [N] [--rules 256,4096,65536] [--reps R] [--host-seconds S]
       python3 tools/repair_bench.py --trace DIR      (per-kernel totals of a rocprofv3 --kernel-trace --stats run of the line above)
       python3 tools/repair_bench.py --decode [english|dna] [N] [--rules ...] [--dec-reps R] [--cross]
           (the device decoder against the host loop on the streams of bit, gamma and delta; --cross: streams of 64 KiB .. 4 MiB)
(output: profiles/repair_<text>_<N>.txt, profiles/repair_decode_<text>_<N>.txt by redirection)"""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("gen", nargs="?", default="english")
ap.add_argument("n", nargs="?", default="16777216")
ap.add_argument("--rules", default="256,4096,65536")
ap.add_argument("--reps", type=int, default=1)
ap.add_argument("--host-seconds", type=float, default=60.0)
ap.add_argument("--trace", default=None)
ap.add_argument("--decode", action="store_true")
ap.add_argument("--cross", action="store_true")
ap.add_argument("--dec-reps", type=int, default=3)
args = ap.parse_args()

if args.trace:
    files = glob.glob(os.path.join(args.trace, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no kernel_stats.csv under %s" % args.trace)
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print("kernel trace (%s): %d kernels, %.1f ms of kernel time" % (os.path.basename(files[0]), len(rows), total / 1e6))
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:16]:
        name = r["Name"].replace("(anonymous namespace)::", "").replace("tdc::", "").replace("void ", "").split("(")[0][:60]
        print("%10.2f ms %5.1f %%  %8d launches  mean %8.1f us  %s" % (float(r["TotalDurationNs"]) / 1e6, 100 * float(r["TotalDurationNs"]) / total,
                                                                      int(r["Calls"]), float(r["AverageNs"]) / 1e3, name))
    sys.exit(0)

import tudocomp_amd as T

if args.decode:
    # Decode column: every stream the compressor makes is decoded by the device decoder (repair_decode.hip; dec_parse = 2, pinned buffers,
    # one warm call, then --dec-reps timed ones) and, in the same run, by the host loop tdc_repair_decode on the same stream (one call that
    # parses, sums the length and expands).  --cross: streams of about 64 KiB .. 4 MiB instead, to see where the two paths cross.
    import ctypes
    import numpy as np
    L = T._native.load()
    CODERS = (("bit", T.CODER_BIT), ("gamma", T.CODER_GAMMA), ("delta", T.CODER_DELTA))
    N = int(float(args.n))
    rules = [int(x) for x in args.rules.split(",")]
    jobs = [(N, mr) for mr in rules] if not args.cross else [(n, 256) for n in (100 << 10, 400 << 10, 1600 << 10, 6400 << 10)]
    print("repair decode, %s; device: dec_parse=2, pinned buffers, one warm call then %d timed ones (all shown, the fastest first); host: "
          "tdc_repair_decode, one call on the same stream" % (args.gen, args.dec_reps))
    print("text B | max_rules | coder | stream B | device ms (h2d / parse+grammar / items+resolver+d2h) | host ms | segments | length rounds | "
          "placement rounds | factors | resolver rounds")
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        for n_text, mr in jobs:
            text = T.PinnedBuffer(n_text)
            (T.gen_english if args.gen == "english" else T.gen_dna)(n_text, 42 if args.gen == "english" else 7, out=text.a)
            want = text.a.tobytes()
            back = T.PinnedBuffer(n_text)
            for name, cid in CODERS:
                out = T.PinnedBuffer(T.repair_bound(n_text, cid))
                slen, _ = ctx.repair_compress_into(text, n_text, out, mr, cid)
                stream = T.PinnedBuffer(slen)
                stream.a[:] = out.a[:slen]
                out.free()
                runs = []
                for _ in range(1 + args.dec_reps):
                    back.a[:] = 0
                    n, st = ctx.repair_decompress_stats_into(stream, back, cid)
                    assert n == n_text and st["device_parse"] == 1 and back.a.tobytes() == want
                    runs.append(st)
                runs = sorted(runs[1:], key=lambda s: s["ms_total"])
                best = runs[0]
                hbuf, hn = np.zeros(n_text, dtype=np.uint8), ctypes.c_size_t()
                t0 = time.perf_counter()
                rc = L.tdc_repair_decode(stream.a.ctypes.data_as(ctypes.c_void_p), slen, cid, hbuf.ctypes.data_as(ctypes.c_void_p), n_text, ctypes.byref(hn))
                t_host = time.perf_counter() - t0
                assert rc == 0 and hn.value == n_text and hbuf.tobytes() == want
                print("%d | %d | %s | %d | %s (%.2f / %.2f / %.2f) | %.2f | %d | %d | %d | %d | %d"
                      % (n_text, mr, name, slen, " ".join("%.2f" % s["ms_total"] for s in runs), best["ms_h2d"], best["ms_factorize"], best["ms_d2h"],
                         t_host * 1e3, best["small_levels"], best["len_rounds"], best["levels"], best["factors"], best["flatten_rounds"]), flush=True)
                stream.free()
            back.free()
            text.free()
    sys.exit(0)

N = int(float(args.n))
RULES = [int(x) for x in args.rules.split(",")]
text = T.PinnedBuffer(N)
if args.gen == "english":
    T.gen_english(N, 42, out=text.a)
else:
    T.gen_dna(N, 7, out=text.a)
want = text.a.tobytes()
print("repair(coder=bit), %s, text of %d B; %d run(s) per max_rules, the fastest shown with all totals behind it" % (args.gen, N, args.reps))

with T.Context(0) as ctx:
    bound = T.repair_bound(N, T.CODER_BIT)
    out = T.PinnedBuffer(bound)
    ctx.repair_compress_into(text, min(N, 1 << 20), out, 16, T.CODER_BIT)          # warm-up: code objects, the arena's first pages
    for mr in RULES:
        best, all_ms = None, []
        for _ in range(args.reps):
            n, st = ctx.repair_compress_into(text, N, out, mr, T.CODER_BIT)
            all_ms.append(st["ms_total"])
            if best is None or st["ms_total"] < best["ms_total"]:
                best = st
        t0 = time.perf_counter()
        back = T.repair_decode(out.a[:n], T.CODER_BIT)
        t_dec = time.perf_counter() - t0
        r, ties = best["rules"], best["tie_rounds"]
        plain = r - ties
        print("max_rules %d: %d rules, %d pairs replaced, stream %d B (bound %d), arena %.2f GB, %d rebuilds; ms_h2d %.2f  ms_factorize %.2f  "
              "ms_encode %.2f  ms_d2h %.2f  ms_total %.2f (all: %s)"
              % (mr, r, best["replaced"], n, bound, best["arena_bytes"] / 1e9, best["rebuilds"], best["ms_h2d"], best["ms_factorize"], best["ms_encode"],
                 best["ms_d2h"], best["ms_total"], " ".join("%.1f" % x for x in all_ms)))
        print("    rounds: mean %.3f ms (ms_factorize / rules, the first count included), first %.3f ms, last %.3f ms; %d tie rounds of mean %.3f ms, "
              "%d others of mean %.3f ms; host decode %.1f ms, correct %s"
              % (best["ms_factorize"] / max(r, 1), best["ms_round_first"], best["ms_round_last"], ties, best["ms_round_tie"] / max(ties, 1), plain,
                 (best["ms_factorize"] - best["ms_round_tie"]) / max(plain, 1), t_dec * 1e3, back == want), flush=True)
    out.free()

if args.host_seconds > 0:
    t0 = time.perf_counter()
    T.repair_grammar(text.a, 4)
    per_rule = (time.perf_counter() - t0) / 4
    fits = [r for r in sorted(set(RULES + [4, 16, 64, 1024])) if r * per_rule <= args.host_seconds]
    mr = max(fits) if fits else 4
    t0 = time.perf_counter()
    hr, hs = T.repair_grammar(text.a, mr)
    t_host = time.perf_counter() - t0
    print("host loop (tdc_repair_grammar, one core; %.2f s per rule over the first 4): max_rules %d -> %d rules, %d symbols left, %.1f s = %.1f ms per round"
          % (per_rule, mr, len(hr), len(hs), t_host, t_host * 1e3 / max(len(hr), 1)))
text.free()
