"""Timing of the repair batch call (repair_batch.hip: one workgroup runs the whole round loop of one text) against what a caller had
before it.  English text, pinned buffers on both sides, wall clock around every call (each returns with its streams idle), one warm-up,
then the median of RUNS runs with the fastest and the slowest beside it; a case whose warm-up takes more than SLOW seconds is timed
with ONE run, and its line says so.

  (a) the batch call                            tdc_gpu_repair_compress_batch, with its stage times and counters
  (b) a loop of the single call                 tdc_gpu_repair_compress on the same context over a SAMPLE of the texts (every
                                                count / sample-th one), scaled to all of them: the single call is a host-driven loop
                                                with a read-back per rule, a loop over all texts would take most of an hour
  (c) the host loop, 16 threads                 tdc_repair_grammar over a sample of the texts in a pool of 16 threads (the calls release
                                                the interpreter lock), scaled: the honest alternative.  It yields the grammars, not the
                                                streams.
Every stream of the last run of (a) is decoded by tdc_repair_decode and compared with its text; the streams of (b) are compared with
those of (a) byte for byte, the rule counts of (c) with those of (a).

Usage: python3 tools/repair_batch_bench.py CASE CODER MAX_RULES [RUNS]   CASE: 4096x64k | 65536x4k | 1x16m; CODER: bit | gamma
                                                                         1x16m: one workgroup walks the whole text once per rule --
                                                                         against the single call, (c) is left out
       python3 tools/repair_batch_bench.py sweep [RUNS]                  option repair_batch_rounds over 4096x64k, bit, unlimited
       python3 tools/repair_batch_bench.py all [RUNS]                    the sweep and every case, each in a process of its own under
                                                                         `timeout -k 10`, stopping at the first one that fails
(output by redirection: profiles/repair_batch_english.txt)"""
import concurrent.futures
import ctypes
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

CASES = {"4096x64k": (4096, 64 << 10), "65536x4k": (65536, 4 << 10), "1x16m": (1, 16 << 20)}
CODERS = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA}
SAMPLE_B = {"4096x64k": 8, "65536x4k": 64, "1x16m": 1}              # texts of the loop (b)
SAMPLE_C = {"4096x64k": 32, "65536x4k": 1024}                       # texts of the pool (c)
SWEEP = (16, 64, 256, 1024, 4096)
LIMIT = 420                                                         # seconds a case may take
SLOW = 8.0
THREADS = 16


def timed(runs, f):
    """one warm-up, then `runs` timed calls (one if the warm-up was slow): (median, fastest, slowest) in ms, the runs, the last result"""
    t0 = time.perf_counter()
    r = f()
    if time.perf_counter() - t0 > SLOW:
        runs = 1
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ms), min(ms), max(ms)), runs, r


def line(what, total, t):
    print("  %-58s median %10.2f ms  (fastest %.2f, slowest %.2f)  = %8.4f GB/s of text" % (what, t[0], t[1], t[2], total / t[0] / 1e6), flush=True)


def host_loop(text, picks, each, max_rules):
    """tdc_repair_grammar of the picked texts, THREADS threads; returns the rule counts"""
    L = T._native.load()
    base = text.a.ctypes.data
    rules = {}

    def work(part):
        r, s, nr, ns = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
        for k in part:
            rc = L.tdc_repair_grammar(base + k * each, each, max_rules, ctypes.byref(r), ctypes.byref(nr), ctypes.byref(s), ctypes.byref(ns))
            assert rc == 0
            L.tdc_gpu_free(r)
            L.tdc_gpu_free(s)
            rules[k] = nr.value

    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(work, [picks[t::THREADS] for t in range(min(THREADS, len(picks)))]))
    return rules


def setup(case, cid):
    count, each = CASES[case]
    total = count * each
    text = T.PinnedBuffer(total)
    T.gen_english(total, 42, out=text.a)
    off = np.arange(count + 1, dtype=np.uint64) * np.uint64(each)
    out = T.PinnedBuffer(T.repair_batch_bound([each] * count, cid))
    return count, each, total, text, off, out


def main(case, coder, max_rules, runs):
    cid = CODERS[coder]
    count, each, total, text, off, out = setup(case, cid)
    print("repair batch, english, %d texts of %d B = %d B, coder=%s, max_rules=%d" % (count, each, total, coder, max_rules), flush=True)
    with T.Context(0) as ctx:
        ta, did, (out_off, out_len, status, st) = timed(runs, lambda: ctx.repair_compress_batch_into(text, off, out, max_rules, cid))
        assert not status.any()
        line("(a) batch call, %s behind one warm-up" % ("median of %d runs" % did if did > 1 else "ONE run"), total, ta)
        print("      last run: ms_h2d %.2f  ms_factorize (grammars) %.2f  ms_encode %.2f  ms_d2h %.2f  ms_total %.2f; %d launches, %d B used, "
              "%d rules, %d tie rounds, %d rebuilds, arena %d B" % (st["ms_h2d"], st["ms_factorize"], st["ms_encode"], st["ms_d2h"], st["ms_total"],
                                                                   st["len_rounds"], st["out_len"], st["rules"], st["tie_rounds"], st["rebuilds"],
                                                                   st["arena_bytes"]), flush=True)
        stream = lambda k: out.a[int(out_off[k]):int(out_off[k]) + int(out_len[k])]
        t0 = time.perf_counter()
        back = all(T.repair_decode(stream(k), cid) == text.a[k * each:(k + 1) * each].tobytes() for k in range(count))
        print("      every stream decoded (tdc_repair_decode) and compared with its text: %s  (%.1f s)" % (back, time.perf_counter() - t0), flush=True)
        picks = list(range(0, count, max(1, count // SAMPLE_B[case])))[:SAMPLE_B[case]]
        got = {}

        def loop():
            for k in picks:
                got[k] = ctx.repair_compress(text.a[k * each:(k + 1) * each], max_rules, cid)[0]

        t0 = time.perf_counter()
        loop()
        tb = (time.perf_counter() - t0) * 1e3 * count / len(picks)
        same = all(stream(k).tobytes() == got[k] for k in picks)
        print("  (b) loop of the single call: %d of %d texts, ONE run, scaled         %10.2f ms  = %8.4f GB/s of text; streams equal to (a)'s: %s; (b) / (a) = %.1f"
              % (len(picks), count, tb, total / tb / 1e6, same, tb / ta[0]), flush=True)
        if case in SAMPLE_C:
            picks = list(range(0, count, count // SAMPLE_C[case]))[:SAMPLE_C[case]]
            t0 = time.perf_counter()
            rules = host_loop(text, picks, each, max_rules)
            tc = (time.perf_counter() - t0) * 1e3 * count / len(picks)
            print("  (c) tdc_repair_grammar, %d threads: %d of %d texts, ONE run, scaled  %10.2f ms  = %8.4f GB/s of text; (c) / (a) = %.1f, (c) / the grammars of (a) = %.1f"
                  % (THREADS, len(picks), count, tc, total / tc / 1e6, tc / ta[0], tc / st["ms_factorize"]), flush=True)
            r, _, _ = ctx.repair_grammar_batch([text.a[k * each:(k + 1) * each] for k in picks[:64]], max_rules)
            print("      rule counts of (c) and of the device equal on %d texts: %s" % (len(r), all(len(r[j]) == rules[k] for j, k in enumerate(picks[:64]))), flush=True)
    for b in (text, out):
        b.free()


def sweep(runs):
    case, cid = "4096x64k", T.CODER_BIT
    count, each, total, text, off, out = setup(case, cid)
    print("repair batch, option repair_batch_rounds, english, %d texts of %d B, coder=bit, max_rules=0; %d run(s) behind one warm-up" % (count, each, runs), flush=True)
    with T.Context(0) as ctx:
        for rounds in SWEEP:
            ctx.set_option("repair_batch_rounds", rounds)
            t, did, (_, _, _, st) = timed(runs, lambda: ctx.repair_compress_batch_into(text, off, out, 0, cid))
            print("  repair_batch_rounds %5d: %3d launches  median %10.2f ms  (fastest %.2f, slowest %.2f; %d run(s))  grammars %10.2f ms"
                  % (rounds, st["len_rounds"], t[0], t[1], t[2], did, st["ms_factorize"]), flush=True)
    for b in (text, out):
        b.free()


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a or (a[0] not in ("all", "sweep") and (a[0] not in CASES or len(a) < 3 or a[1] not in CODERS)):
        sys.exit(__doc__)
    if a[0] == "all":
        jobs = [["sweep"]] + [[case, coder, mr] for case in ("4096x64k", "65536x4k") for mr in ("0", "256") for coder in CODERS]
        jobs += [["1x16m", "bit", "256"]]
        for job in jobs:
            rc = subprocess.call(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__)] + job + a[1:2])
            if rc:
                sys.exit("repair_batch_bench: %s ended with status %d; nothing more is started" % (" ".join(job), rc))
    elif a[0] == "sweep":
        sweep(int(a[1]) if len(a) > 1 else 3)
    else:
        main(a[0], a[1], int(a[2]), int(a[3]) if len(a) > 3 else 5)
