#!/bin/bash
# Development aid: stage lengths in the KERNEL TRACE of one step (bench.py --steps 1 --warmup 1), for a list of option settings -- stable to
# ~0.1 ms where an A/B of whole steps wanders by a millisecond:  tools/stage_spans.sh "VAR=x" "VAR=y VAR2=z" ...
#   up+sa = first kernel of the step (the histogram of the first chunk) -> fused scatter; sa = last kernel behind the upload -> fused scatter; leaf = last partition scatter -> first pass over the head flags; rounds = that -> fused
#   scatter; phi = fused scatter -> candidates (fused_cand: -> behind the image kernel, which classifies them); fact = candidates -> flatten (the classification
#   counts in fact with cand_class_kernel and in phi with fused_cand: across that switch compare phi+fact, printed as one span, not its halves); flat = flatten -> pack
#   (with flatten_chunks the first pack starts inside the flatten stage: flat then ends at the first range's pack);
#   tail = start of flatten_init -> end of the step's last device activity, kernel or copy (the last download chunk is in the copy trace), with the
#   ends of the last flatten round, the last pack and the last download behind it, all counted from the start of flatten_init
#   --size N as the first argument: a text of N bytes instead of the metric's 2e9
R=$PWD
SIZE=""
if [ "$1" = "--size" ]; then SIZE="--size $2"; shift 2; fi
for cfg in "$@"; do
  OUT=$R/gpurun_out/stagespan; rm -rf $OUT; mkdir -p $OUT
  ( cd /tmp && export TMPDIR=/tmp && env TDC_GPU_DEBUG_KNOBS=1 $cfg timeout 300 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $OUT -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extra $SIZE > /dev/null 2> $OUT/err.txt )
  python3 - "$cfg" $OUT <<'PY'
import csv, glob, sys
cfg, out = sys.argv[1:3]
f = glob.glob(out + "/**/*kernel_trace.csv", recursive=True)
if not f: print(cfg, "no trace"); sys.exit(0)
rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f[0]))))
copies = []
for g in glob.glob(out + "/**/*memory_copy_trace.csv", recursive=True):
    copies += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy " + r.get("Direction", "")) for r in csv.DictReader(open(g))]
def tail(fl):          # from the start of flatten_init to the end of the step's last device activity (the step ends at a gap of 20 ms)
    t0 = rows[fl][0]
    act = sorted(rows[fl:] + [c for c in copies if c[0] >= t0])
    end, ends = act[0][1], {}
    for a in act:
        if a[0] - end > 20e6: break
        end = max(end, a[1])
        for key, pats in (("flat", ("flatten_round",)), ("pack", ("pack_cls",)), ("d2h", ("DEVICE_TO_HOST", "rocclr_copyBuffer"))):      # (a download is a copy kernel or a row of the copy trace)
            if any(pat in a[2] for pat in pats): ends[key] = max(ends.get(key, 0), a[1])
    return " | tail %.3f (last flatten round %s, last pack %s, last download %s)" % ((end - t0) / 1e6, *("%.3f" % ((ends[k] - t0) / 1e6) if k in ends else "-" for k in ("flat", "pack", "d2h")))
def last(pat, hi=None): return [i for i, r in enumerate(rows[:hi]) if pat in r[2]][-1]
def first(pat, lo): return next(i for i in range(lo, len(rows)) if pat in rows[i][2])
def cand(lo):          # where the candidates start: cand_class_kernel, or (fused_cand: the image kernel classifies) the first kernel behind the fold of its counters
    try: return first("cand_class", lo)
    except StopIteration: return first("fs_cand_fold", lo) + 1
try:
    i0 = last("ws_scatter_kernel<2, false, true")
    up = last("byte_hist", i0)
    up0 = up
    while up0 > 0 and rows[up0][0] - rows[up0 - 1][0] < 20e6 : up0 -= 1      # first kernel of the step (a gap of 20 ms and more: the step before)
    j = first("sa_flag_count", i0); k = first("fs_count", j); c = cand(k); fl = first("flatten_init", c); pk = first("pack_cls", fl)
    ms = lambda a, b: (b - a) / 1e6
    print("%-44s up+sa %.2f | sa %.2f (leaf %.2f rounds %.2f) phi %.2f fact %.2f (phi+fact %.2f) flat %.2f | sum %.2f%s" % (cfg, ms(rows[up0][0], rows[k][0]), ms(rows[up][1], rows[k][0]), ms(rows[i0][1], rows[j][0]), ms(rows[j][0], rows[k][0]),
          ms(rows[k][0], rows[c][0]), ms(rows[c][0], rows[fl][0]), ms(rows[k][0], rows[fl][0]), ms(rows[fl][0], rows[pk][0]), ms(rows[up][1], rows[pk][0]), tail(fl)))
except Exception as e: print(cfg, "trace not understood:", e)
PY
  rm -rf $OUT
done
