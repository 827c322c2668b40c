"""Timing of the lzss batch calls (lzss_sw_batch.hip) against what a caller had before them: a loop of the single calls over the same
texts on the same context.  English text of 256 MiB in all, window 16, threshold 3, pinned buffers on both sides, wall clock around
every call (each returns with its streams idle), one warm-up, then the median of RUNS runs with the fastest and the slowest beside it.

  compress    (a) tdc_gpu_lzss_sw_compress_batch   (b) a loop of tdc_gpu_lzss_sw_compress_into over the texts
              (c) tdc_gpu_lzss_sw_compress_into on the concatenation (one stream: not the same output, the same amount of work)
  decompress  (a) tdc_gpu_lzss_sw_decompress_batch (b) a loop of tdc_gpu_lzss_sw_decompress_into, default options
              (c) tdc_gpu_lzss_sw_decompress_into on the stream of (c)
The streams of (a) and (b) are compared byte for byte, the texts of every decoder with the input.

Usage: python3 tools/lzss_batch_bench.py CASE CODER [RUNS] [LOOP_RUNS]     CASE: 4096x64k | 65536x4k | 1x256m; CODER: bit | gamma
                                                                           LOOP_RUNS: runs of the loops (b); under 1x256m, of the batch
                                                                           decoder, which one wave runs alone there (no warm-up; 0: not run)
       python3 tools/lzss_batch_bench.py all [RUNS] [LOOP_RUNS]            every case and coder, each in a process of its own under
                                                                           `timeout -k 10`, stopping at the first one that fails
(output by redirection: profiles/lzss_batch_english.txt)"""
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

CASES = {"4096x64k": (4096, 64 << 10), "65536x4k": (65536, 4 << 10), "1x256m": (1, 256 << 20)}
CODERS = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA}
LIMIT = {"4096x64k": 600, "65536x4k": 1100, "1x256m": 900}          # seconds a case may take
W, THRESHOLD = 16, 3


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


def main(case, coder, runs, loop_runs):
    count, each = CASES[case]
    cid = CODERS[coder]
    total = count * each
    text = T.PinnedBuffer(total)
    T.gen_english(total, 42, out=text.a)
    off = np.arange(count + 1, dtype=np.uint64) * np.uint64(each)
    slot = (T.lzss_sw_bound(each, W, cid) + 7) // 8 * 8
    cap = T.lzss_sw_batch_bound([each] * count, W, cid)
    assert cap == slot * count
    out_a, out_b, back = T.PinnedBuffer(cap), T.PinnedBuffer(cap), T.PinnedBuffer(total)
    print("lzss batch, english, %d texts of %d B = %d B, window %d, threshold %d, coder=%s, median of %d runs (loops: %d) behind one warm-up"
          % (count, each, total, W, THRESHOLD, coder, runs, loop_runs), flush=True)
    with T.Context(0) as ctx:
        # ---- compress
        ta, (out_off, out_len, status, st) = timed(runs, lambda: ctx.lzss_sw_compress_batch_into(text, off, out_a, W, THRESHOLD, cid))
        assert not status.any()
        line("compress   (a) batch call", total, ta)
        print("      stages of the last run: ms_h2d %.2f  ms_factorize %.2f  ms_encode %.2f  ms_d2h %.2f  ms_total %.2f; %d B used, %d factors, arena %d B"
              % (st["ms_h2d"], st["ms_factorize"], st["ms_encode"], st["ms_d2h"], st["ms_total"], st["out_len"], st["factors"], st["arena_bytes"]))
        lens = np.zeros(count, dtype=np.int64)

        def loop_compress():
            for k in range(count):
                lens[k] = ctx.lzss_sw_compress_into(text.a[k * each:(k + 1) * each], each, out_b.a[k * slot:(k + 1) * slot], W, THRESHOLD, cid)[0]

        if count > 1:
            tb, _ = timed(loop_runs, loop_compress)
            line("compress   (b) loop of the single call over the texts", total, tb)
            same = all(out_a.a[int(out_off[k]):int(out_off[k]) + int(out_len[k])].tobytes() == out_b.a[k * slot:k * slot + int(lens[k])].tobytes()
                       for k in range(count))
            print("      streams of (a) and (b) equal: %s; (b) / (a) = %.2f" % (same, tb[0] / ta[0]), flush=True)
        if count == 1 or case == "4096x64k":
            tc, (n_c, _) = timed(runs, lambda: ctx.lzss_sw_compress_into(text, total, out_b, W, THRESHOLD, cid))
            line("compress   (c) single call on the concatenation", total, tc)
            print("      (a) / (c) = %.2f" % (ta[0] / tc[0]), flush=True)
        # ---- decompress
        # (one text: one wave walks the whole stream, which takes minutes -- LOOP_RUNS calls without a warm-up, 0 skips it)
        if count > 1 or loop_runs:
            ta, (text_off, status, st) = timed(runs if count > 1 else loop_runs,
                                               lambda: ctx.lzss_sw_decompress_batch_into(out_a, out_off[:-1], out_len, back, cid, W), warm=count > 1)
            ok = not status.any() and int(text_off[-1]) == total and np.array_equal(back.a, text.a)
            line("decompress (a) batch call" + ("" if count > 1 else ", %d run(s), no warm-up" % loop_runs), total, ta)
            print("      stages of the last run: ms_h2d %.2f  sizes pass %.2f  write pass %.2f  ms_d2h %.2f  ms_total %.2f; correct %s"
                  % (st["ms_h2d"], st["ms_factorize"], st["ms_encode"], st["ms_d2h"], st["ms_total"], ok), flush=True)
        else:
            ta = None
            print("  decompress (a) batch call: not run", flush=True)
        back.a[:] = 0

        def loop_decompress():
            for k in range(count):
                o = int(out_off[k])
                ctx.lzss_sw_decompress_into(out_a.a[o:o + int(out_len[k])], back.a[k * each:(k + 1) * each], W, cid)

        if count > 1:
            tb, _ = timed(loop_runs, loop_decompress)
            line("decompress (b) loop of the single call, default options", total, tb)
            print("      correct %s; (b) / (a) = %.2f" % (np.array_equal(back.a, text.a), tb[0] / ta[0]), flush=True)
        if count == 1 or case == "4096x64k":
            back.a[:] = 0
            tc, _ = timed(runs, lambda: ctx.lzss_sw_decompress_into(out_b.a[:n_c], back, W, cid))
            line("decompress (c) single call on the stream of (c)", total, tc)
            print("      correct %s%s" % (np.array_equal(back.a, text.a), "; (a) / (c) = %.2f" % (ta[0] / tc[0]) if ta else ""), flush=True)
    for b in (text, out_a, out_b, back):
        b.free()


if __name__ == "__main__":
    if len(sys.argv) < 2 or (sys.argv[1] != "all" and (sys.argv[1] not in CASES or len(sys.argv) < 3 or sys.argv[2] not in CODERS)):
        sys.exit(__doc__)
    if sys.argv[1] == "all":
        for case in CASES:
            for coder in CODERS:
                rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[case]), sys.executable, os.path.abspath(__file__), case, coder] + sys.argv[2:4])
                if rc:
                    sys.exit("lzss_batch_bench: %s %s ended with status %d; nothing more is started" % (case, coder, rc))
    else:
        runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
        main(sys.argv[1], sys.argv[2], runs, int(sys.argv[4]) if len(sys.argv) > 4 else runs)
