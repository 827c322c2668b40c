"""Timing of the lzw / lz78 batch decoders (lz_batch_decode.hip: the items of all streams as one forest, one pass) against what a caller
had before them.  English text, the streams made by the batch compressor (one long text: by the single call), pinned buffers on both
sides, wall clock around every call (each returns with its streams idle), one warm-up, then the median of RUNS runs with the fastest
and the slowest beside it.

  (a) the batch call                              tdc_gpu_lzw_decompress_batch / tdc_gpu_lz78_decompress_batch, with its stage times
  (b) a loop of the single device entry point     tdc_gpu_lzw_decompress / tdc_gpu_lz78_decompress at default options on the same context
                                                  (lzw: streams below 64 KiB take the host loop there; lz78: every stream is a device call)
  (c) lzw: the host loop, 16 threads              tdc_lzw_decode over the streams in a pool of 16 threads (the calls release the
                                                  interpreter lock; one ctypes call per stream is part of the time)
The texts of (a), (b) and (c) are compared byte for byte with the input.

Usage: python3 tools/lz_batch_decode_bench.py CASE ALGO [RUNS] [LOOP_RUNS]   CASE: 4096x64k | 65536x4k | 1x16m; ALGO: lzw-bit | lzw-gamma | lz78-gamma
                                                                             LOOP_RUNS: runs of the loop (b), behind no warm-up of its own
       python3 tools/lz_batch_decode_bench.py all [RUNS] [LOOP_RUNS]         every case and algorithm, each in a process of its own under
                                                                             `timeout -k 10`, stopping at the first one that fails
(output by redirection: profiles/lz_batch_decode_english.txt)"""
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
LIMIT = {"4096x64k": 300, "65536x4k": 500, "1x16m": 300}            # seconds a case may take
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


def host_decode(blob, s_off, s_len, cid, out, each):
    """tdc_lzw_decode of every stream into its slot of `out`, THREADS threads; True if every call succeeded with `each` bytes"""
    L = T._native.load()
    src, dst = blob.a.ctypes.data, out.a.ctypes.data
    count = len(s_off)

    def work(part):
        n = ctypes.c_size_t()
        ok = True
        for k in part:
            rc = L.tdc_lzw_decode(src + int(s_off[k]), int(s_len[k]), cid, dst + k * each, each, ctypes.byref(n))
            ok = ok and rc == 0 and n.value == each
        return ok

    parts = [range(t, count, THREADS) for t in range(min(THREADS, count))]
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        return all(pool.map(work, parts))


def main(case, name, runs, loop_runs):
    count, each = CASES[case]
    algo, cid = ALGOS[name]
    total = count * each
    text = T.PinnedBuffer(total)
    T.gen_english(total, 42, out=text.a)
    out = T.PinnedBuffer(total)
    print("%s batch decoder, english, %d streams of %d B of text = %d B, coder=%s, median of %d runs behind one warm-up (loop: %d, no warm-up)"
          % (algo, count, each, total, name.split("-")[1], runs, loop_runs), flush=True)
    with T.Context(0) as ctx:
        # the streams: what the batch compressor leaves (every stream at a multiple of 8), or the single call's for one long text
        if count > 1:
            off = np.arange(count + 1, dtype=np.uint64) * np.uint64(each)
            cap = (T.lzw_batch_bound if algo == "lzw" else T.lz78_batch_bound)([each] * count, cid)
            blob = T.PinnedBuffer(cap)
            comp = ctx.lzw_compress_batch_into if algo == "lzw" else ctx.lz78_compress_batch_into
            o, s_len, status, _ = comp(text, off, blob, cid)
            assert not status.any()
            s_off = o[:-1].copy()
        else:
            one = (ctx.lzw_compress(text.a, cid) if algo == "lzw" else ctx.lz78_compress(text.a, cid))[0]
            blob = T.PinnedBuffer(len(one))
            blob.a[:] = np.frombuffer(one, dtype=np.uint8)
            s_off, s_len = np.zeros(1, dtype=np.uint64), np.array([len(one)], dtype=np.uint64)
        into = ctx.lzw_decompress_batch_into if algo == "lzw" else ctx.lz78_decompress_batch_into
        ta, (out_off, status, st) = timed(runs, lambda: into(blob, s_off, s_len, out, cid))
        assert not status.any() and int(out_off[count]) == total
        same_a = bool((out.a == text.a).all())
        line("(a) batch call", total, ta)
        print("      stages of the last run: ms_h2d %.2f  ms_factorize (parse, lengths, sizes) %.2f  ms_encode (literals, resolver, download) %.2f  ms_total %.2f;"
              " %d B of streams, %d items, rounds %d + %d, arena %d B"
              % (st["ms_h2d"], st["ms_factorize"], st["ms_encode"], st["ms_total"], st["n"], st["factors"], st["len_rounds"], st["flatten_rounds"],
                 st["arena_bytes"]))
        out.a[:] = 0
        single = (lambda x, dst: ctx.lzw_decompress_into(x, dst, cid)) if algo == "lzw" else (lambda x, dst: ctx.lz78_decompress_into(x, dst))
        views = [(blob.a[int(s_off[k]):int(s_off[k]) + int(s_len[k])], out.a[k * each:(k + 1) * each]) for k in range(count)]
        dev = 0

        def loop():
            nonlocal dev
            dev = 0
            for x, dst in views:
                dev += single(x, dst)[1].get("device_parse", 1)

        tb, _ = timed(loop_runs, loop, warm=False)
        same_b = bool((out.a == text.a).all())
        line("(b) loop of the single device entry point", total, tb)
        print("      texts of (a) and (b) equal the input: %s, %s; %d of %d streams of (b) parsed on the device; (b) / (a) = %.2f"
              % (same_a, same_b, dev, count, tb[0] / ta[0]), flush=True)
        if algo == "lzw":
            out.a[:] = 0
            tc, ok = timed(runs, lambda: host_decode(blob, s_off, s_len, cid, out, each))
            line("(c) tdc_lzw_decode, %d threads" % min(THREADS, count), total, tc)
            print("      texts of (c) equal the input: %s; (a) / (c) = %.2f" % (ok and bool((out.a == text.a).all()), ta[0] / tc[0]), flush=True)
    for b in (text, out, blob):
        b.free()
    print(flush=True)


if __name__ == "__main__":
    if len(sys.argv) < 2 or (sys.argv[1] != "all" and (sys.argv[1] not in CASES or len(sys.argv) < 3 or sys.argv[2] not in ALGOS)):
        sys.exit(__doc__)
    if sys.argv[1] == "all":
        for case in CASES:
            for name in ALGOS:
                rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[case]), sys.executable, os.path.abspath(__file__), case, name] + sys.argv[2:4])
                if rc:
                    sys.exit("lz_batch_decode_bench: %s %s ended with status %d; nothing more is started" % (case, name, rc))
    else:
        runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
        main(sys.argv[1], sys.argv[2], runs, int(sys.argv[4]) if len(sys.argv) > 4 else 1)
