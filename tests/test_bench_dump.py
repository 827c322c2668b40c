"""bench.py --dump-outputs: the stream of the last timed step as .npy files (float32 / float64, bounded size, seeded sample of a
long stream).  The writer is checked on the CPU; one small GPU run checks that the dumped stream is the oracle's stream of the
benchmark's text."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_short_stream_is_written_whole(tmp_path):
    B = _bench()
    s = np.random.default_rng(3).integers(0, 256, 100000, dtype=np.uint8)
    B.dump_stream(str(tmp_path), s)
    got = _load(str(tmp_path))
    assert set(got) == {"stream", "stream_length", "stream_byte_histogram", "stream_head", "stream_tail"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["stream"].astype(np.uint8), s)
    assert got["stream_length"][0] == s.size
    assert np.array_equal(got["stream_byte_histogram"], np.bincount(s, minlength=256))
    assert np.array_equal(got["stream_head"], s[:B.DUMP_EDGE]) and np.array_equal(got["stream_tail"], s[-B.DUMP_EDGE:])


def test_long_stream_is_sampled_within_64_mb_and_reproducibly(tmp_path):
    B = _bench()
    s = np.random.default_rng(4).integers(0, 256, B.DUMP_FULL_MAX * 3 + 17, dtype=np.uint8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    B.dump_stream(a, s)
    B.dump_stream(b, s.copy())
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 << 20
    ga, gb = _load(a), _load(b)
    assert set(ga) == set(gb) and all(np.array_equal(ga[k], gb[k]) for k in ga)
    idx = ga["stream_index"].astype(np.int64)
    assert idx.size == B.DUMP_SAMPLE and np.all(np.diff(idx) >= 0) and idx[0] >= 0 and idx[-1] < s.size
    assert np.array_equal(ga["stream"].astype(np.uint8), s[idx])
    assert ga["stream_length"][0] == s.size


@pytest.mark.gpu
def test_bench_dumps_the_oracle_stream_of_its_text(tmp_path):
    """bench.py's timed path on a 1 MiB English text: the dumped stream equals the oracle's stream of the same text (generator seed 42,
    sentinel, threshold 2, flatten 1), and --steps is the number of timed steps the line reports"""
    import tudocomp_amd as T
    from oracle import oracle as O
    n = 1 << 20
    d = str(tmp_path / "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", str(n), "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-extra", "--dump-outputs", d],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["ms_per_step"] > 0
    want, _ = O.lcpcomp_huff_compress(np.concatenate([T.gen_english(n, 42), np.zeros(1, dtype=np.uint8)]), 2, 1)
    got = _load(d)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert bytes(got["stream"].astype(np.uint8)) == want
    assert got["stream_length"][0] == len(want)
