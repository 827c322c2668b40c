#!/usr/bin/env python3
"""Times encode(sle) as a stage on one text: tools/sle_stage_bench.py --text english|dna --size BYTES [--kmer 3] [--calls 5]

One process, one context, page-locked buffers.  After a warm-up call of each shape:
  1. encode(sle) alone through pipeline_compress_into (medians; upload and download included), and one call with option pipe_log
     (the stage's own time on stderr and in pipe_ms, behind a synchronisation);
  2. the chains bwt:rle:mtf:encode(sle) and bwt:rle:mtf:encode(huff) on the same text and buffers, alternating three times, and one
     pipe_log call of each (pipe_ms per stage, lengths behind every stage);
  3. the way back on the stream of 1: pipeline_decompress_stats with dec_parse = 2 (the device decoder) against tdc_sle_decode (the host
     loop, no context) on the same stream in the same run, alternating, and one pipe_log call of the device path.
Every round trip is checked.  Prints one line per figure; redirect both streams into profiles/sle_stage_<text>_<size>.txt."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tudocomp_amd as T  # noqa: E402


def timed(fn, calls):
    fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return r, ts


def line(what, ts, extra=""):
    print("%-52s min %9.2f  median %9.2f  max %9.2f ms  (%d calls) %s" % (what, min(ts), float(np.median(ts)), max(ts), len(ts), extra), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", choices=("english", "dna"), default="english")
    ap.add_argument("--size", type=int, default=1 << 28)
    ap.add_argument("--kmer", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    N, n = a.size, a.size + 1
    seed = 42 if a.text == "english" else 7
    gen = T.gen_english if a.text == "english" else T.gen_dna
    sle = (T.STAGE_SLE, a.kmer)
    chain_sle = [T.STAGE_BWT, T.STAGE_RLE, T.STAGE_MTF, sle]
    chain_huff = [T.STAGE_BWT, T.STAGE_RLE, T.STAGE_MTF, T.STAGE_HUFF]
    h_text, h_out, h_back = T.PinnedBuffer(n), T.PinnedBuffer(T.pipeline_bound([sle], n)), T.PinnedBuffer(n)
    L = T._native.load()
    try:
        gen(N, seed, out=h_text.a)
        h_text.a[N] = 0
        print("sle_stage_bench: %s seed %d, %d bytes + sentinel, kmer %d" % (a.text, seed, N, a.kmer), flush=True)
        with T.Context(0, options={"dec_parse": 2}) as ctx:
            # 1. the stage alone
            (zlen, st), ts = timed(lambda: ctx.pipeline_compress_into([sle], h_text, n, h_out), a.calls)
            line("encode(sle) alone, incl. transfers", ts, "%d -> %d bytes, arena %.2f GB" % (n, zlen, st["arena_bytes"] / 1e9))
            ctx.set_option("pipe_log", 1)
            _, st = ctx.pipeline_compress_into([sle], h_text, n, h_out)
            ctx.set_option("pipe_log", 0)
            print("encode(sle) alone, stage time (pipe_ms) %9.2f ms" % st["pipe_ms"][0], flush=True)
            # 3. the way back, on that stream (before the chains reuse h_out)
            def device():
                return ctx.pipeline_decompress_stats([sle], h_out, h_back, zlen)

            def host():
                m = ctypes.c_size_t()
                rc = L.tdc_sle_decode(h_out.a.ctypes.data_as(ctypes.c_void_p), zlen, a.kmer, h_back.a.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(m))
                assert rc == 0, rc
                return m.value

            device(); host()
            for rep in range(3):
                for name, fn in (("device decode (dec_parse = 2), incl. transfers", device), ("tdc_sle_decode (host loop)", host)):
                    h_back.a[:4096] = 0
                    t0 = time.perf_counter()
                    r = fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    m = r[0] if isinstance(r, tuple) else r
                    assert m == n and bool((h_back.a == h_text.a).all()), "round trip failed"
                    print("alternate %d  %-48s wall %9.2f ms%s" % (rep, name, dt, "  pipe_dev 0x%x" % r[1]["pipe_dev"] if isinstance(r, tuple) else ""), flush=True)
            ctx.set_option("pipe_log", 1)
            _, st = device()
            ctx.set_option("pipe_log", 0)
            print("device decode, stage time (pipe_ms) %9.2f ms" % st["pipe_ms"][0], flush=True)
            # 2. the chains
            for stages in (chain_sle, chain_huff):
                ctx.pipeline_compress_into(stages, h_text, n, h_out)
            for rep in range(3):
                for name, stages in (("bwt:rle:mtf:encode(sle)", chain_sle), ("bwt:rle:mtf:encode(huff)", chain_huff)):
                    t0 = time.perf_counter()
                    zl, _ = ctx.pipeline_compress_into(stages, h_text, n, h_out)
                    print("alternate %d  %-48s wall %9.2f ms -> %d bytes" % (rep, name, (time.perf_counter() - t0) * 1e3, zl), flush=True)
            ctx.set_option("pipe_log", 1)
            for name, stages in (("bwt:rle:mtf:encode(sle)", chain_sle), ("bwt:rle:mtf:encode(huff)", chain_huff)):
                zl, st = ctx.pipeline_compress_into(stages, h_text, n, h_out)
                print("%s stage times (pipe_ms) %s, lengths %s" % (name, ["%.2f" % t for t in st["pipe_ms"]], st["pipe_len"]), flush=True)
                m, st = ctx.pipeline_decompress_stats(stages, h_out, h_back, zl)
                assert m == n and bool((h_back.a == h_text.a).all()), "round trip failed"
                print("%s decode stage times (pipe_ms) %s, pipe_dev 0x%x" % (name, ["%.2f" % t for t in st["pipe_ms"]], st["pipe_dev"]), flush=True)
            ctx.set_option("pipe_log", 0)
    finally:
        h_text.free(); h_out.free(); h_back.free()


if __name__ == "__main__":
    main()
