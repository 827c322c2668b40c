"""Timing of the batch pipeline call (bytestages_batch.hip behind bwt_batch.hip: rle, mtf and encode(huff) over the texts of a batch,
the intermediates in device memory) against what a caller had before it.  English text cut into texts that end in a 0, pinned buffers
on both sides, wall clock around every call (each returns with its streams idle), one warm-up, then the median of RUNS runs with the
fastest and the slowest beside it.  For each of the chains bwt:rle:mtf:encode(huff) and rle:mtf:encode(huff):

  (a) the batch call             tdc_gpu_pipeline_compress_batch into a buffer sized by its sizes pass, with its stats
  (b) the loop                   tdc_gpu_pipeline_compress_into on the same context over a SAMPLE of the texts (every count / sample-th
                                 one, 512 at the most), ONE run, the calls alone timed, scaled to all of them -- the way without (a)
  (c) the floor (bwt chain)      tdc_gpu_bwt_compress_batch alone, same texts
  (d) stage times                ONE batch call with option pipe_log (a synchronisation behind every stage; the log lines go to stderr),
                                 the host's table build of encode(huff) on the library's threads and, ONE call each, on one thread
The streams of (b) are compared with those of (a) byte for byte.

Usage: python3 tools/bwtzip_batch_bench.py CASE [RUNS]     CASE: 4096x64k | 65536x4k
       python3 tools/bwtzip_batch_bench.py all [RUNS]      every case, each in a process of its own under `timeout -k 10`, stopping at
                                                           the first one that fails
(output by redirection: profiles/bwtzip_batch_english.txt)"""
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import tudocomp_amd as T

CASES = {"4096x64k": (4096, 64 << 10), "65536x4k": (65536, 4 << 10)}
CHAINS = (("bwt:rle:mtf:encode(huff)", [T.STAGE_BWT, (T.STAGE_RLE, 0), T.STAGE_MTF, T.STAGE_HUFF]),
          ("rle:mtf:encode(huff)", [(T.STAGE_RLE, 0), T.STAGE_MTF, T.STAGE_HUFF]))
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
    text, bwt = T.PinnedBuffer(total), T.PinnedBuffer(total)
    one_in, one_out = T.PinnedBuffer(each), T.PinnedBuffer(T.pipeline_bound(CHAINS[0][1], each))
    T.gen_english(total, 42, out=text.a)
    text.a[text.a == 0] = 32
    text.a[each - 1::each] = 0                                      # every text ends in its only 0
    off = np.arange(count + 1, dtype=np.uint64) * np.uint64(each)
    picks = list(range(0, count, max(1, count // SAMPLE)))[:SAMPLE]
    print("bwtzip batch, english, %d texts of %d B = %d B; %d runs behind one warm-up" % (count, each, total, runs), flush=True)
    with T.Context(0) as ctx:
        for name, stages in CHAINS:
            print(" chain %s" % name, flush=True)
            try:
                ctx.pipeline_compress_batch_into(stages, text, off, None)
                required = 8
            except T.TdcGpuError as e:
                required = e.required
            out = T.PinnedBuffer(required)
            ta, (out_off, out_len, status, st) = timed(runs, lambda: ctx.pipeline_compress_batch_into(stages, text, off, out))
            assert not status.any()
            line("(a) batch call", total, ta)
            print("      last run: ms_h2d %.2f  ms_d2h %.2f  ms_total %.2f; bytes behind the stages %s; %d B of streams (%.4f of the text), "
                  "arena %d B" % (st["ms_h2d"], st["ms_d2h"], st["ms_total"], st["pipe_len"], int(out_len.sum()), out_len.sum() / total,
                                  st["arena_bytes"]), flush=True)
            same, spent = True, 0.0
            for k in picks:                                         # (the copy into the pinned buffer and the compare are not timed)
                one_in.a[:] = text.a[k * each:(k + 1) * each]
                t0 = time.perf_counter()
                n, _ = ctx.pipeline_compress_into(stages, one_in, each, one_out)
                spent += time.perf_counter() - t0
                o = int(out_off[k])
                same = same and n == int(out_len[k]) and np.array_equal(one_out.a[:n], out.a[o:o + n])
            tb = spent * 1e3 * count / len(picks)
            print("  (b) loop of the single call: %d of %d texts, ONE run, scaled  %10.2f ms  = %8.4f GB/s of text; streams equal to (a)'s: %s; "
                  "(b) / (a) = %.1f" % (len(picks), count, tb, total / tb / 1e6, same, tb / ta[0]), flush=True)
            if stages[0] == T.STAGE_BWT:
                tc, (status, _) = timed(runs, lambda: ctx.bwt_compress_batch_into(text, off, bwt))
                assert not status.any()
                line("(c) bwt_compress_batch_into alone (the floor)", total, tc)
                print("      (a) - (c) = %.2f ms for rle, mtf, encode(huff) and the smaller download" % (ta[0] - tc[0]), flush=True)
            ctx.set_option("pipe_log", 1)
            for threads in (0, 1):
                ctx.set_option("pipe_batch_threads", threads)
                sys.stderr.write("pipe_log: %s, %s, pipe_batch_threads %d\n" % (case, name, threads))
                t0 = time.perf_counter()
                _, _, _, st = ctx.pipeline_compress_batch_into(stages, text, off, out)
                ms = (time.perf_counter() - t0) * 1e3
                print("  (d) ONE call with pipe_log, table build on %s: %.2f ms; per stage %s ms" %
                      ("the library's threads" if threads == 0 else "one thread", ms, ["%.2f" % x for x in st["pipe_ms"]]), flush=True)
            ctx.set_option("pipe_log", 0)
            ctx.set_option("pipe_batch_threads", 0)
            out.free()
    for b in (text, bwt, one_in, one_out):
        b.free()


if __name__ == "__main__":
    a = sys.argv[1:]
    if not a or (a[0] != "all" and a[0] not in CASES):
        sys.exit(__doc__)
    if a[0] == "all":
        for case in CASES:
            rc = subprocess.call(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), case] + a[1:2])
            if rc:
                sys.exit("bwtzip_batch_bench: %s ended with status %d; nothing more is started" % (case, rc))
    else:
        main(a[0], int(a[1]) if len(a) > 1 else 5)
