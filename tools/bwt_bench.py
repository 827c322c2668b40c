#!/usr/bin/env python3
"""Times the bwt compressor on one text: tools/bwt_bench.py --text english|dna --size BYTES [--calls 5] [--host-prefix BYTES]

One process, one context.  After a warm-up call each: bwt_compress_into and bwt_decompress_into with page-locked buffers, the same with
pageable buffers, one inverse with option bwt_log (stage times on stderr), the stage entry point over a few sample distances (--sweep),
and the facade's host inverse loop (`tdc -d` on a prefix of --host-prefix bytes, 64 MiB by default; 0 skips it).  With --lcpcomp the
forward transform alternates three times with lcpcomp_compress_into(coder=huff, threshold=2) on the same buffers.  Prints one line per
figure; redirect into profiles/bwt_<text>_<size>.txt."""
import argparse
import os
import subprocess
import sys
import tempfile
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
    print("%-44s min %9.2f  median %9.2f  max %9.2f ms  (%d calls) %s" % (what, min(ts), float(np.median(ts)), max(ts), len(ts), extra), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", choices=("english", "dna"), default="english")
    ap.add_argument("--size", type=int, default=1 << 28)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-prefix", type=int, default=1 << 26)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--lcpcomp", action="store_true")
    ap.add_argument("--no-pageable", action="store_true")
    a = ap.parse_args()
    N, n = a.size, a.size + 1
    seed = 42 if a.text == "english" else 7
    gen = T.gen_english if a.text == "english" else T.gen_dna
    h_text, h_bwt, h_back = T.PinnedBuffer(n), T.PinnedBuffer(n), T.PinnedBuffer(n)
    try:
        gen(N, seed, out=h_text.a)
        h_text.a[N] = 0
        print("bwt_bench: %s seed %d, %d bytes + sentinel" % (a.text, seed, N), flush=True)
        with T.Context(0) as ctx:
            (_, st), ts = timed(lambda: ctx.bwt_compress_into(h_text, n, h_bwt), a.calls)
            line("bwt_compress_into, page-locked", ts, "device: h2d %.2f sa %.2f gather %.2f d2h %.2f total %.2f ms"
                 % (st["ms_h2d"], st["ms_sa"], st["ms_encode"], st["ms_d2h"], st["ms_total"]))
            (_, ds), ts = timed(lambda: ctx.bwt_decompress_into(h_bwt, h_back), a.calls)
            line("bwt_decompress_into, page-locked", ts, "rounds %d" % ds["rounds"])
            assert bool((h_back.a == h_text.a).all()), "round trip failed"
            if not a.no_pageable:
                p_text, p_out = h_text.a.copy(), np.empty(n, dtype=np.uint8)
                _, ts = timed(lambda: ctx.bwt_compress_into(p_text, n, p_out), a.calls)
                line("bwt_compress_into, pageable", ts)
                p_bwt = h_bwt.a.copy()
                _, ts = timed(lambda: ctx.bwt_decompress_into(p_bwt, p_out), a.calls)
                line("bwt_decompress_into, pageable", ts)
                del p_text, p_out, p_bwt
            if a.lcpcomp:
                for rep in range(3):
                    for name, fn in (("bwt_compress_into", lambda: ctx.bwt_compress_into(h_text, n, h_bwt)),
                                     ("lcpcomp_compress_into(huff, 2)", lambda: ctx.lcpcomp_compress_into(h_text, n, h_back, 2, 1))):
                        t0 = time.perf_counter()
                        _, s = fn()
                        print("alternate %d  %-32s wall %9.2f ms  device total %9.2f ms" % (rep, name, (time.perf_counter() - t0) * 1e3, s["ms_total"]), flush=True)
                ctx.bwt_compress_into(h_text, n, h_bwt)
            sys.stderr.flush()
            ctx.set_option("bwt_log", 1)
            ctx.bwt_decompress_into(h_bwt, h_back)
            ctx.set_option("bwt_log", 0)
            for item in [x for x in a.sweep.split(",") if x]:
                s, m = (int(v) for v in item.split(":"))
                b = h_bwt.a
                (_, st), ts = timed(lambda: ctx.bwt_inverse_stage(b, s, m, want_lf=False), max(2, a.calls // 2))
                line("inverse_stage sample %d max_steps %d" % (s, m), ts, "heads %d launches %d (pageable buffers)" % (st["heads"], st["launches"]))
        if a.host_prefix:
            m = min(a.host_prefix, N)
            with T.Context(0) as ctx:
                prefix = np.concatenate([h_text.a[:m], np.zeros(1, dtype=np.uint8)])
                b, _ = ctx.bwt_compress(prefix)
            tdc = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
            with tempfile.TemporaryDirectory() as d:
                f = os.path.join(d, "p.tdc")
                with open(f, "wb") as fh:
                    fh.write(b"bwt%" + b)
                ts = []
                for _ in range(2):
                    r = subprocess.run([tdc, "-d", "-f", "-s", "-o", os.path.join(d, "p.out"), f], capture_output=True, text=True)
                    assert r.returncode == 0, r.stderr
                    t0 = time.perf_counter()
                    subprocess.run([tdc, "-d", "-f", "-o", os.path.join(d, "p.out"), f], check=True)
                    ts.append((time.perf_counter() - t0) * 1e3)
                line("host inverse loop (tdc -d), %d B prefix" % m, ts, "whole process incl. file i/o and unescaping")
    finally:
        h_text.free(); h_bwt.free(); h_back.free()


if __name__ == "__main__":
    main()
