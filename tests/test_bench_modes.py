"""bench.py: a plain run does only what its headline needs (set up, warm up, the timed steps, --dump-outputs, the JSON line); --full adds
the CPU baseline, the extras, the comparisons with the oracle's streams, the profiled step and, for N > 1, the second exchange and the
container check.  The option handling is checked on the CPU; small GPU runs check the lines of both kinds of run and the containers a
plain two-rank rehearsal leaves behind."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

HEADLINE = {"metric": "input MB/s end-to-end lcpcomp+huffman", "unit": "MB/s", "higher_is_better": True, "dtype": "u32"}
FULL_ONLY = {"roofline", "kernels", "cpu_baseline", "decompress", "configs1_256MiB", "configs2_dna_1e9", "configs3_lz78",
             "stream_matches_golden", "rccl_gather", "container_ok"}


def _bench():
    spec = importlib.util.spec_from_file_location("bench", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _args(B, monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return B.parse_args()


def test_full_is_off_by_default(monkeypatch):
    B = _bench()
    assert _args(B, monkeypatch, "--gpus", "1", "--steps", "2", "--warmup", "1").full is False
    assert _args(B, monkeypatch, "--gpus", "1", "--steps", "2", "--warmup", "1", "--full").full is True


@pytest.mark.parametrize("full", [False, True])
def test_self_launch_runs_the_cpu_baseline_and_passes_full_on_only_with_full(monkeypatch, capsys, full):
    """`bench.py --gpus 2` without torchrun's environment: the parent times the CPU baseline and hands it to the ranks only with --full,
    and the ranks get --full exactly when the parent did"""
    B = _bench()
    args = _args(B, monkeypatch, "--gpus", "2", "--steps", "2", "--warmup", "1", *(["--full"] if full else []))
    baselines, cmds = [], []
    monkeypatch.setattr(B, "cpu_baseline", lambda a, seed: baselines.append(seed) or ({"value": 1.0}, (1, 1, "0" * 64), None))

    def run(cmd, **kw):
        cmds.append(cmd)
        return types.SimpleNamespace(returncode=0, stdout='{"metric": "m", "value": 1.0}\n')

    monkeypatch.setattr(B.subprocess, "run", run)
    with pytest.raises(SystemExit) as e:
        B.launch_ranks(args)
    assert e.value.code == 0
    assert len(cmds) == 1 and "torch.distributed.run" in cmds[0]
    assert ("--full" in cmds[0]) == full and ("--cpu-result" in cmds[0]) == full
    assert baselines == ([42] if full else [])
    assert capsys.readouterr().out.strip() == '{"metric": "m", "value": 1.0}'


def _run(*argv, env=None):
    p = subprocess.run([sys.executable, BENCH, *argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_full_adds_the_rest():
    common = ["--gpus", "1", "--size", str(1 << 20), "--steps", "2", "--warmup", "1"]
    plain = _run(*common)
    assert {k: plain[k] for k in HEADLINE} == HEADLINE
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert plain["hbm_resident"]["value"] > 0 and plain["stats"]["out_len"] > 0 and plain["stages_ms"]["total"] > 0
    assert not FULL_ONLY & set(plain), sorted(FULL_ONLY & set(plain))
    full = _run(*common, "--full", "--no-cpu-baseline")
    assert {k: full[k] for k in HEADLINE} == HEADLINE
    assert full["stats"]["out_len"] == plain["stats"]["out_len"]
    assert full["kernels"] and full["roofline"]["kernel"] in full["kernels"]
    assert full["decompress"]["round_trip"] is True


@pytest.mark.gpu
@pytest.mark.parametrize("exchange", ["shared host memory", "rccl gather to rank 0"])
def test_plain_two_rank_rehearsal_dumps_the_oracle_streams_of_both_shards(tmp_path, exchange):
    """a plain `bench.py --gpus 2` (two ranks on this box's one GPU over gloo) with either exchange as `value`: no --full keys, and the
    dumped block container holds the oracle's stream of every rank's shard (seed 42 + rank)"""
    import tudocomp_amd as T
    from tudocomp_amd.blocks import header_len, unpack_container
    from oracle import oracle as O
    n = 1 << 20
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["TDC_BENCH_BACKEND"] = "gloo"
    if exchange != "shared host memory":
        env["TDC_BENCH_RCCL_GATHER"] = "1"
    d = str(tmp_path / "out")
    j = _run("--gpus", "2", "--size", str(n), "--steps", "2", "--warmup", "1", "--dump-outputs", d, env=env)
    assert {k: j[k] for k in HEADLINE} == HEADLINE and j["value"] > 0
    assert j["n_gpus"] == 2 and j["ranks_seen"] == 2 and j["exchange"] == exchange
    assert not FULL_ONLY & set(j), sorted(FULL_ONLY & set(j))
    blob = bytes(np.load(os.path.join(d, "stream.npy")).astype(np.uint8))
    assert len(blob) == header_len(2) + j["gathered_bytes"]
    parts = unpack_container(blob)
    assert len(parts) == 2
    for r, (raw_len, payload) in enumerate(parts):
        want, _ = O.lcpcomp_huff_compress(np.concatenate([T.gen_english(n, 42 + r), np.zeros(1, dtype=np.uint8)]), 2, 1)
        assert raw_len == n and bytes(payload) == want, r
