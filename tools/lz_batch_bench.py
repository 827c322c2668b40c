"""Timing of the lzw / lz78 batch calls (lz_batch.hip: the texts are parsed on the device, one wave per text) against what a caller had
before them.  English text, pinned buffers on both sides, wall clock around every call (each returns with its streams idle), one
warm-up, then the median of RUNS runs with the fastest and the slowest beside it.

  (a) the batch call                           tdc_gpu_lzw_compress_batch / tdc_gpu_lz78_compress_batch, with its stage times
  (b) a loop of the single call over the texts tdc_gpu_lzw_compress / tdc_gpu_lz78_compress on the same context (host parse, device coder)
  (c) the host parse alone, 16 threads         tdc_lzw_factors / tdc_lz78_factors over the texts in a pool of 16 threads (the calls
                                               release the interpreter lock; one ctypes call per text is part of the time): the honest
                                               alternative to the device parse.  It yields the items, not the streams.
The streams of (a) and (b) are compared byte for byte.

Usage: python3 tools/lz_batch_bench.py CASE ALGO [RUNS] [LOOP_RUNS]   CASE: 4096x64k | 65536x4k | 1x16m; ALGO: lzw-bit | lzw-gamma | lz78-gamma
                                                                      LOOP_RUNS: runs of the loop (b); 1x16m: one wave walks the whole text,
                                                                      the batch call runs RUNS times WITHOUT a warm-up
       python3 tools/lz_batch_bench.py all [RUNS] [LOOP_RUNS]         every case and algorithm, each in a process of its own under
                                                                      `timeout -k 10`, stopping at the first one that fails
(output by redirection: profiles/lz_batch_english.txt)"""
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
ALGOS = {"lzw-bit": ("lzw", T.CODER_BIT), "lzw-gamma": ("lzw", T.CODER_GAMMA), "lz78-gamma": ("lz78", T.CODER_GAMMA)}
LIMIT = {"4096x64k": 300, "65536x4k": 400, "1x16m": 300}            # seconds a case may take
THREADS = 16


def timed(runs, f, warm=True):
    """one warm-up, then `runs` timed calls: (median, fastest, slowest) in ms, and the last result"""
    r = f() if warm else None
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ms), min(ms), max(ms)), r


def line(what, total, t):
    print("  %-52s median %10.2f ms  (fastest %.2f, slowest %.2f)  = %7.3f GB/s of text" % (what, t[0], t[1], t[2], total / t[0] / 1e6), flush=True)


def host_parse(algo, text, count, each):
    """the host parse of every text, THREADS threads; returns the number of items"""
    L = T._native.load()
    base = text.a.ctypes.data
    free = L.tdc_gpu_free

    def work(part):
        items = 0
        a, b, z = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        for k in part:
            if algo == "lzw":
                rc = L.tdc_lzw_factors(base + k * each, each, ctypes.byref(a), ctypes.byref(z))
            else:
                rc = L.tdc_lz78_factors(base + k * each, each, ctypes.byref(a), ctypes.byref(b), ctypes.byref(z))
                free(b)
            free(a)
            assert rc == 0
            items += z.value
        return items

    parts = [range(t, count, THREADS) for t in range(min(THREADS, count))]
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        return sum(pool.map(work, parts))


def main(case, name, runs, loop_runs):
    count, each = CASES[case]
    algo, cid = ALGOS[name]
    total = count * each
    text = T.PinnedBuffer(total)
    T.gen_english(total, 42, out=text.a)
    off = np.arange(count + 1, dtype=np.uint64) * np.uint64(each)
    cap = (T.lzw_batch_bound if algo == "lzw" else T.lz78_batch_bound)([each] * count, cid)
    out_a = T.PinnedBuffer(cap)
    print("%s batch, english, %d texts of %d B = %d B, coder=%s, median of %d runs (loop: %d) behind one warm-up"
          % (algo, count, each, total, name.split("-")[1], runs, loop_runs), flush=True)
    with T.Context(0) as ctx:
        into = ctx.lzw_compress_batch_into if algo == "lzw" else ctx.lz78_compress_batch_into
        ta, (out_off, out_len, status, st) = timed(runs, lambda: into(text, off, out_a, cid), warm=count > 1)
        assert not status.any()
        line("(a) batch call" + ("" if count > 1 else ", %d run(s), no warm-up" % runs), total, ta)
        print("      stages of the last run: ms_h2d %.2f  ms_factorize (parse) %.2f  ms_encode %.2f  ms_d2h %.2f  ms_total %.2f; %d B used, %d items, arena %d B"
              % (st["ms_h2d"], st["ms_factorize"], st["ms_encode"], st["ms_d2h"], st["ms_total"], st["out_len"], st["factors"], st["arena_bytes"]))
        single = (lambda x: ctx.lzw_compress(x, cid)[0]) if algo == "lzw" else (lambda x: ctx.lz78_compress(x, cid)[0])
        got = [None] * count

        def loop():
            for k in range(count):
                got[k] = single(text.a[k * each:(k + 1) * each])

        tb, _ = timed(loop_runs, loop)
        line("(b) loop of the single call over the texts", total, tb)
        same = all(out_a.a[int(out_off[k]):int(out_off[k]) + int(out_len[k])].tobytes() == got[k] for k in range(count))
        print("      streams of (a) and (b) equal: %s; (b) / (a) = %.2f" % (same, tb[0] / ta[0]), flush=True)
        tc, items = timed(runs, lambda: host_parse(algo, text, count, each))
        line("(c) host parse alone, %d threads" % min(THREADS, count), total, tc)
        print("      items of (c) and (a) equal: %s; (a) / (c) = %.2f, the parse of (a) alone / (c) = %.2f"
              % (items == st["factors"], ta[0] / tc[0], st["ms_factorize"] / tc[0]), flush=True)
    for b in (text, out_a):
        b.free()


if __name__ == "__main__":
    if len(sys.argv) < 2 or (sys.argv[1] != "all" and (sys.argv[1] not in CASES or len(sys.argv) < 3 or sys.argv[2] not in ALGOS)):
        sys.exit(__doc__)
    if sys.argv[1] == "all":
        for case in CASES:
            for name in ALGOS:
                rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[case]), sys.executable, os.path.abspath(__file__), case, name] + sys.argv[2:4])
                if rc:
                    sys.exit("lz_batch_bench: %s %s ended with status %d; nothing more is started" % (case, name, rc))
    else:
        runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
        main(sys.argv[1], sys.argv[2], runs, int(sys.argv[4]) if len(sys.argv) > 4 else runs)
