"""Timing of the bwt batch calls (bwt_batch.hip: one prefix doubling over the unresolved positions of all texts; the LF cycles of all
buffers as one forest) against what a caller had before them.  English text cut into texts that end in a 0, pinned buffers on both
sides, wall clock around every call (each returns with its streams idle), one warm-up, then the median of RUNS runs with the fastest
and the slowest beside it.

  (a) the batch call, forward    tdc_gpu_bwt_compress_batch, with its stage times and counters
  (b) the loop, forward          tdc_gpu_bwt_compress_into on the same context over a SAMPLE of the texts (every count / sample-th
                                 one, 512 at the most), ONE run, the calls alone timed, scaled to all of them
  (c) the batch call, inverse    tdc_gpu_bwt_decompress_batch on the transforms of (a)
  (d) the loop, inverse          tdc_gpu_bwt_decompress_into over the same sample, ONE run, scaled
The transforms of (b) are compared with those of (a) byte for byte, the texts of (c) with the input, those of (d) with the input.

Usage: python3 tools/bwt_batch_bench.py CASE [RUNS]     CASE: 4096x64k | 65536x4k | 1xcap (one text of BWT_BATCH_TEXT_CAP bytes, through
                                                        both paths: where the single call is the tool)
       python3 tools/bwt_batch_bench.py all [RUNS]      every case, each in a process of its own under `timeout -k 10`, stopping at the
                                                        first one that fails
(output by redirection: profiles/bwt_batch_english.txt)"""
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

CASES = {"4096x64k": (4096, 64 << 10), "65536x4k": (65536, 4 << 10), "1xcap": (1, 1 << 20)}
SAMPLE = 512
LIMIT = 420                                                         # seconds a case may take


def timed(runs, f):
    """one warm-up, then `runs` timed calls: (median, fastest, slowest) in ms and the last result"""
    r = f()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return (statistics.median(ms), min(ms), max(ms)), r


def line(what, total, t):
    print("  %-52s median %10.2f ms  (fastest %.2f, slowest %.2f)  = %8.4f GB/s of text" % (what, t[0], t[1], t[2], total / t[0] / 1e6), flush=True)


def main(case, runs):
    count, each = CASES[case]
    total = count * each
    text, bwt, back = T.PinnedBuffer(total), T.PinnedBuffer(total), T.PinnedBuffer(total)
    one_in, one_out = T.PinnedBuffer(each), T.PinnedBuffer(each)
    T.gen_english(total, 42, out=text.a)
    text.a[text.a == 0] = 32
    text.a[each - 1::each] = 0                                      # every text ends in its only 0
    off = np.arange(count + 1, dtype=np.uint64) * np.uint64(each)
    picks = list(range(0, count, max(1, count // SAMPLE)))[:SAMPLE]
    print("bwt batch, english, %d texts of %d B = %d B; %d runs behind one warm-up" % (count, each, total, runs), flush=True)
    with T.Context(0) as ctx:
        ta, (status, st) = timed(runs, lambda: ctx.bwt_compress_batch_into(text, off, bwt))
        assert not status.any()
        line("(a) batch call, forward", total, ta)
        print("      last run: ms_h2d %.2f  ms_sa %.2f  ms_encode (gather) %.2f  ms_d2h %.2f  ms_total %.2f; %d doubling rounds, %d records sorted, "
              "arena %d B" % (st["ms_h2d"], st["ms_sa"], st["ms_encode"], st["ms_d2h"], st["ms_total"], st["len_rounds"], st["sa_sorted_elems"],
                              st["arena_bytes"]), flush=True)
        same, spent = True, 0.0
        for k in picks:                                             # (the copy into the pinned buffer and the compare are not timed)
            one_in.a[:] = text.a[k * each:(k + 1) * each]
            t0 = time.perf_counter()
            ctx.bwt_compress_into(one_in, each, one_out)
            spent += time.perf_counter() - t0
            same = same and np.array_equal(one_out.a, bwt.a[k * each:(k + 1) * each])
        tb = spent * 1e3 * count / len(picks)
        print("  (b) loop of the single call, forward: %d of %d texts, ONE run, scaled  %10.2f ms  = %8.4f GB/s of text; transforms equal to (a)'s: %s; "
              "(b) / (a) = %.1f" % (len(picks), count, tb, total / tb / 1e6, same, tb / ta[0]), flush=True)
        tc, (status, st) = timed(runs, lambda: ctx.bwt_decompress_batch_into(bwt, off, back))
        assert not status.any()
        line("(c) batch call, inverse", total, tc)
        print("      last run: ms_h2d %.2f  ms_sa (LF) %.2f  ms_encode (walks, ranking) %.2f  ms_d2h %.2f  ms_total %.2f; %d walk launches, %d jump "
              "rounds, %d heads, longest list %d, arena %d B; texts equal to the input: %s"
              % (st["ms_h2d"], st["ms_sa"], st["ms_encode"], st["ms_d2h"], st["ms_total"], st["levels"], st["len_rounds"], st["entries"],
                 st["flen_max"], st["arena_bytes"], np.array_equal(back.a, text.a)), flush=True)
        same, spent = True, 0.0
        for k in picks:
            one_in.a[:] = bwt.a[k * each:(k + 1) * each]
            t0 = time.perf_counter()
            ctx.bwt_decompress_into(one_in, one_out)
            spent += time.perf_counter() - t0
            same = same and np.array_equal(one_out.a, text.a[k * each:(k + 1) * each])
        td = spent * 1e3 * count / len(picks)
        print("  (d) loop of the single call, inverse: %d of %d texts, ONE run, scaled  %10.2f ms  = %8.4f GB/s of text; texts equal to the input: %s; "
              "(d) / (c) = %.1f" % (len(picks), count, td, total / td / 1e6, same, td / tc[0]), flush=True)
    for b in (text, bwt, back, one_in, one_out):
        b.free()


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a or (a[0] != "all" and a[0] not in CASES):
        sys.exit(__doc__)
    if a[0] == "all":
        for case in CASES:
            rc = subprocess.call(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), case] + a[1:2])
            if rc:
                sys.exit("bwt_batch_bench: %s ended with status %d; nothing more is started" % (case, rc))
    else:
        main(a[0], int(a[1]) if len(a) > 1 else 5)
