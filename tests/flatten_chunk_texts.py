"""Texts of tests/test_gpu_flatten_chunks.py: n = 2^21 + 3 * 4096 + 1 bytes including the sentinel -- the smallest length at which
the pack and the download of a host-buffer call overlap (1 024 encoder tiles of 2 048 positions), and no multiple of a tile."""
import numpy as np

import tudocomp_amd as T

N = (1 << 21) + 3 * 4096 + 1


def _rand(rng, k):
    return rng.integers(1, 255, k, dtype=np.uint8)            # bytes 1 .. 254: nothing to escape


def english():
    return T.gen_english(N - 1, 42)


def random_then_english():
    """a first half of random bytes (no block of it is laid out twice), then English"""
    rng = np.random.default_rng(11)
    h = (N - 1) // 2
    return np.concatenate([_rand(rng, h), T.gen_english(N - 1 - h, 43)])


def long_run():
    """one byte repeated for 1.5 MiB inside English: one factor longer than several ranges, tile bounds inside it"""
    e = T.gen_english(N - 1, 44)
    e[200_000:200_000 + 3 * (1 << 19)] = 66
    return e


def shifted_copies():
    """B . noise . B' . noise . B'' ...: a random block of 64 KiB; every later copy is cut from the copy before it, shifted by a few
    bytes -- the factors of copy j point into copy j - 1, whose factors point into copy j - 2: chains three and more deep, across the
    range borders, sources included"""
    rng = np.random.default_rng(12)
    parts, prev, total = [], _rand(rng, 1 << 16), 0
    while total < N - 1:
        parts.append(prev)
        noise = _rand(rng, int(rng.integers(40, 400)))
        parts.append(noise)
        total += len(prev) + len(noise)
        sh = int(rng.integers(1, 9))
        prev = np.concatenate([prev[sh:], _rand(rng, sh)])
    return np.concatenate(parts)[:N - 1]


def periodic_block():
    """a random block of 8 KiB repeated to the end.  The longest repeat is the whole text against itself one period on, so one factor
    covers everything but the last period, and the few thousand short factors of that period share a handful of tiles at the very
    end: with 16 ranges most tile bounds coincide and most pack ranges are empty.  (The random half of random_then_english cannot be
    free of factors at threshold 2 -- 254^2 byte pairs do not fill a MiB -- so this text stands in for what that one is meant to show.)"""
    rng = np.random.default_rng(13)
    b = _rand(rng, 8192)
    return np.tile(b, (N - 1) // len(b) + 1)[:N - 1]


TEXTS = {"english": english, "random_then_english": random_then_english, "long_run": long_run, "shifted_copies": shifted_copies,
         "periodic_block": periodic_block}
