"""Timing of the batch decoder of repair streams (repair_batch_decode.hip: the grammars of all streams as one forest, one pass) against
what a caller had before it.  English text, the streams made by the batch compressor (one long text: by the single call), pinned buffers
on both sides, wall clock around every call (each returns with its streams idle), one warm-up, then the median of RUNS runs with the
fastest and the slowest beside it.

  (a) the batch call                              tdc_gpu_repair_decompress_batch, with its stage times and its three round counts
  (b) a loop of the single device entry point     tdc_gpu_repair_decompress_into on the same context, at default options (streams below
                                                  1 MiB take the host loop there) and at dec_parse = 2 (every stream a device call).
                                                  More than SAMPLE streams: the first SAMPLE of them, ONE run, scaled by the stream
                                                  bytes -- the line says so
  (c) the host loop, 16 threads                   tdc_repair_decode over the streams in a pool of 16 threads (the calls release the
                                                  interpreter lock; one ctypes call per stream is part of the time)
The texts of (a), (b) and (c) are compared byte for byte with the input.

Usage: python3 tools/repair_batch_decode_bench.py CASE CODER MAX_RULES [RUNS]   CASE: 4096x64k | 65536x4k | 1x16m; CODER: bit | gamma | delta
       python3 tools/repair_batch_decode_bench.py all [RUNS]                    the cases, bit and gamma, max_rules 0 and 256 (1x16m: 256
                                                                                alone), each in a process of its own under `timeout -k 10`,
                                                                                stopping at the first one that fails
(output by redirection: profiles/repair_batch_decode_english.txt)"""
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
CODERS = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
LIMIT = 400                                                          # seconds a case may take
THREADS = 16
SAMPLE = 512


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
    print("  %-58s median %10.2f ms  (fastest %.2f, slowest %.2f)  = %7.3f GB/s of text" % (what, t[0], t[1], t[2], total / t[0] / 1e6), flush=True)


def host_decode(blob, s_off, s_len, cid, out, each):
    """tdc_repair_decode of every stream into its slot of `out`, THREADS threads; True if every call succeeded with `each` bytes"""
    L = T._native.load()
    src, dst = blob.a.ctypes.data, out.a.ctypes.data
    count = len(s_off)

    def work(part):
        n = ctypes.c_size_t()
        ok = True
        for k in part:
            rc = L.tdc_repair_decode(src + int(s_off[k]), int(s_len[k]), cid, dst + k * each, each, ctypes.byref(n))
            ok = ok and rc == 0 and n.value == each
        return ok

    parts = [range(t, count, THREADS) for t in range(min(THREADS, count))]
    with concurrent.futures.ThreadPoolExecutor(THREADS) as pool:
        return all(pool.map(work, parts))


def main(case, coder, max_rules, runs):
    count, each = CASES[case]
    cid = CODERS[coder]
    total = count * each
    text = T.PinnedBuffer(total)
    T.gen_english(total, 42, out=text.a)
    out = T.PinnedBuffer(total)
    print("repair batch decoder, english, %d streams of %d B of text = %d B, coder=%s, max_rules=%d, median of %d runs behind one warm-up"
          % (count, each, total, coder, max_rules, runs), flush=True)
    with T.Context(0) as ctx:
        # the streams: what the batch compressor leaves (every stream at a multiple of 8), or the single call's for one long text
        if count > 1:
            off = np.arange(count + 1, dtype=np.uint64) * np.uint64(each)
            blob = T.PinnedBuffer(T.repair_batch_bound([each] * count, cid))
            o, s_len, status, _ = ctx.repair_compress_batch_into(text, off, blob, max_rules, cid)
            assert not status.any()
            s_off = o[:-1].copy()
        else:
            one = ctx.repair_compress(text.a, max_rules, cid)[0]
            blob = T.PinnedBuffer(len(one))
            blob.a[:] = np.frombuffer(one, dtype=np.uint8)
            s_off, s_len = np.zeros(1, dtype=np.uint64), np.array([len(one)], dtype=np.uint64)
        ta, (out_off, status, st) = timed(runs, lambda: ctx.repair_decompress_batch_into(blob, s_off, s_len, out, cid))
        assert not status.any() and int(out_off[count]) == total
        same_a = bool((out.a == text.a).all())
        line("(a) batch call", total, ta)
        print("      stages of the last run: ms_h2d %.2f  ms_factorize (walks, lengths, sizes) %.2f  ms_encode (first occurrences, items, resolver,"
              " download) %.2f  ms_total %.2f; %d B of streams, %d rules, %d factors, rounds %d (lengths) + %d (first occurrences) + %d (resolver),"
              " arena %d B" % (st["ms_h2d"], st["ms_factorize"], st["ms_encode"], st["ms_total"], st["n"], st["rules"], st["factors"],
                               st["len_rounds"], st["levels"], st["flatten_rounds"], st["arena_bytes"]))
        take = min(count, SAMPLE)
        scale = float(s_len.sum()) / float(s_len[:take].sum())
        views = [(blob.a[int(s_off[k]):int(s_off[k]) + int(s_len[k])], out.a[k * each:(k + 1) * each]) for k in range(take)]
        for parse, what in ((1, "default options"), (2, "dec_parse = 2")):
            ctx.set_option("dec_parse", parse)
            out.a[:] = 0

            def loop():
                for x, dst in views:
                    ctx.repair_decompress_into(x, dst, cid)

            tb, _ = timed(1 if take < count else runs, loop, warm=take == count)
            same_b = bool((out.a[:take * each] == text.a[:take * each]).all())
            tb = tuple(v * scale for v in tb)
            line("(b) loop of tdc_gpu_repair_decompress_into, %s" % what, total, tb)
            print("      %s; texts equal the input: (a) %s, (b) %s; (b) / (a) = %.2f"
                  % ("all streams" if take == count else "the first %d streams, one run, scaled by %.1f" % (take, scale), same_a, same_b, tb[0] / ta[0]),
                  flush=True)
        ctx.set_option("dec_parse", 1)
        out.a[:] = 0
        tc, ok = timed(runs, lambda: host_decode(blob, s_off, s_len, cid, out, each))
        line("(c) tdc_repair_decode, %d threads" % min(THREADS, count), total, tc)
        print("      texts of (c) equal the input: %s; (c) / (a) = %.2f" % (ok and bool((out.a == text.a).all()), tc[0] / ta[0]), flush=True)
    for b in (text, out, blob):
        b.free()
    print(flush=True)


if __name__ == "__main__":
    if len(sys.argv) < 2 or (sys.argv[1] != "all" and (sys.argv[1] not in CASES or len(sys.argv) < 4 or sys.argv[2] not in CODERS)):
        sys.exit(__doc__)
    if sys.argv[1] == "all":
        for case in CASES:
            for max_rules in ((256,) if case == "1x16m" else (0, 256)):
                for coder in ("bit", "gamma"):
                    rc = subprocess.call(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), case, coder, str(max_rules)] + sys.argv[2:3])
                    if rc:
                        sys.exit("repair_batch_decode_bench: %s %s %d ended with status %d; nothing more is started" % (case, coder, max_rules, rc))
    else:
        main(sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 5)
