#!/usr/bin/env python3
"""Times the bwtzip chain (bwt:rle:mtf:encode(huff)) on one text: tools/bwtzip_bench.py --text english|dna --size BYTES [--calls 5]

One process, one context, page-locked buffers.  After a warm-up call: the chain through pipeline_compress_into (medians, the length
behind every stage), the same call alternating three times with bwt_compress_into on the same text and buffers (the difference is what
the three byte stages cost or save), one chain call with option pipe_log (stage times on stderr, each behind a synchronisation), the
three stages alone on the transform, and the way back (--decompress-only skips everything in front of it): after a warm-up of both
paths, pipeline_decompress_stats into page-locked memory with the default options (device decoders) against option dec_parse = 0 (the
host loops for encode(huff), mtf and rle; the inverse of bwt on the device either way), then one call of each with pipe_log (stage
lines on stderr, each behind a synchronisation).  Prints one line per figure; redirect both streams into
profiles/bwtzip_<text>_<size>.txt or profiles/bwtzip_decode_<text>_<size>.txt."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tudocomp_amd as T  # noqa: E402

BWTZIP = [T.STAGE_BWT, T.STAGE_RLE, T.STAGE_MTF, T.STAGE_HUFF]


def timed(fn, calls):
    fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


def line(what, ts, extra=""):
    print("%-44s min %9.2f  median %9.2f  max %9.2f ms  (%d calls) %s" % (what, min(ts), float(np.median(ts)), max(ts), len(ts), extra), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", choices=("english", "dna"), default="english")
    ap.add_argument("--size", type=int, default=1 << 28)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-decompress", action="store_true")
    ap.add_argument("--decompress-only", action="store_true")
    a = ap.parse_args()
    N, n = a.size, a.size + 1
    seed = 42 if a.text == "english" else 7
    gen = T.gen_english if a.text == "english" else T.gen_dna
    h_text, h_out, h_back = T.PinnedBuffer(n), T.PinnedBuffer(2 * n), T.PinnedBuffer(n)       # (rle alone may double its input)
    try:
        gen(N, seed, out=h_text.a)
        h_text.a[N] = 0
        print("bwtzip_bench: %s seed %d, %d bytes + sentinel" % (a.text, seed, N), flush=True)
        with T.Context(0) as ctx:
            if not a.decompress_only:
                (zlen, st), ts = timed(lambda: ctx.pipeline_compress_into(BWTZIP, h_text, n, h_out), a.calls)
                line("chain pipeline_compress_into", ts, "lengths behind bwt / rle / mtf / huff: %s" % st["pipe_len"])
                (_, bs), tb = timed(lambda: ctx.bwt_compress_into(h_text, n, h_back), a.calls)
                line("bwt_compress_into", tb, "device: h2d %.2f sa %.2f gather %.2f d2h %.2f total %.2f ms"
                     % (bs["ms_h2d"], bs["ms_sa"], bs["ms_encode"], bs["ms_d2h"], bs["ms_total"]))
                for rep in range(3):
                    for name, fn in (("bwt_compress_into", lambda: ctx.bwt_compress_into(h_text, n, h_back)),
                                     ("chain pipeline_compress_into", lambda: ctx.pipeline_compress_into(BWTZIP, h_text, n, h_out))):
                        t0 = time.perf_counter()
                        fn()
                        print("alternate %d  %-32s wall %9.2f ms" % (rep, name, (time.perf_counter() - t0) * 1e3), flush=True)
                # the three stages alone, on the transform bwt_compress_into left in h_back (upload and download included)
                b = h_back
                for name, stage in (("rle", (T.STAGE_RLE, 0)), ("mtf", T.STAGE_MTF), ("encode(huff)", T.STAGE_HUFF)):
                    (ln, _), ts1 = timed(lambda: ctx.pipeline_compress_into([stage], b, n, h_out), max(2, a.calls // 2))
                    line("%s alone on the transform, incl. transfers" % name, ts1, "%d -> %d bytes" % (n, ln))
            zlen, _ = ctx.pipeline_compress_into(BWTZIP, h_text, n, h_out)
            sys.stdout.flush()
            if not a.decompress_only:
                ctx.set_option("pipe_log", 1)
                ctx.pipeline_compress_into(BWTZIP, h_text, n, h_out)
                ctx.set_option("pipe_log", 0)
            if not a.no_decompress:
                for mode, what in ((1, "device decoders (default)"), (0, "host loops (dec_parse = 0)")):
                    ctx.set_option("dec_parse", mode)
                    calls = a.calls if mode else 1
                    (m, st), ts = timed(lambda: ctx.pipeline_decompress_stats(BWTZIP, h_out, h_back, zlen), calls)
                    assert m == n and bool((h_back.a == h_text.a).all()), "round trip failed"
                    line("chain pipeline_decompress_stats, %s" % what, ts, "pipe_dev 0x%x, lengths %s, arena %.2f GB" % (st["pipe_dev"], st["pipe_len"], st["arena_bytes"] / 1e9))
                    sys.stdout.flush()
                    ctx.set_option("pipe_log", 1)
                    ctx.pipeline_decompress_stats(BWTZIP, h_out, h_back, zlen)
                    ctx.set_option("pipe_log", 0)
                ctx.set_option("dec_parse", 1)
    finally:
        h_text.free(); h_out.free(); h_back.free()


if __name__ == "__main__":
    main()
