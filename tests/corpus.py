"""Small input corpus shared by the CPU and GPU parity tests.

Strings in the spirit of the reference's roundtrip_batch / string generators (test/test/util.hpp:98-207):
empty and tiny inputs, periodic and run-rich words, Fibonacci and Thue-Morse words, random texts over small and
large alphabets, inputs containing 0x00 / 0xFF (escaping changes n) and planted long repeats.
"""
import random

import numpy as np


def fib_word(k):
    a, b = b"b", b"a"
    for _ in range(k):
        a, b = b, b + a
    return b


def thue_morse(k):
    s = b"a"
    for _ in range(k):
        s = s + bytes(ord("a") + ord("b") - c for c in s)
    return s


def run_rich(n, rng):
    out = b""
    while len(out) < n:
        out += bytes([rng.randrange(97, 100)]) * rng.randrange(1, 40)
    return out[:n]


def planted(n, sigma, rng, replen=64):
    base = bytes(rng.randrange(65, 65 + sigma) for _ in range(replen))
    out = b""
    while len(out) < n:
        if rng.random() < 0.3:
            k = rng.randrange(1, replen + 1)
            o = rng.randrange(0, replen - k + 1)
            out += base[o:o + k]
        else:
            out += bytes(rng.randrange(65, 65 + sigma) for _ in range(rng.randrange(1, 20)))
    return out[:n]


def small_corpus():
    rng = random.Random(20260101)
    c = [
        ("empty", b""),
        ("a", b"a"),
        ("ab", b"ab"),
        ("aa", b"aa"),
        ("survey_example", b"abcdebcdeabcd abcdebcdeabcd banana bandana"),
        ("abcabc", b"abcabcabcabcabcabcabcabc"),
        ("a^100", b"a" * 100),
        ("a^1000", b"a" * 1000),
        ("ab^300", b"ab" * 300),
        ("banana", b"bananabanana"),
        ("sentence", b"This is a test. This is only a test. Testing, testing, one two three."),
        ("utf8", "größe straße ünïcödé größe straße".encode("utf-8")),
        ("zeros", b"\x00\x00\x00\x00abc\x00\x00"),
        ("ff", b"\xff\xfe\xff\xff\x00\x01\xff\xfe\x00" * 7),
        ("all_bytes", bytes(range(256)) * 3),
        ("fib12", fib_word(12)),
        ("fib17", fib_word(17)),
        ("thue10", thue_morse(10)),
        ("thue13", thue_morse(13)),
        ("runrich", run_rich(3000, rng)),
        ("planted2", planted(5000, 2, rng)),
        ("planted4", planted(20000, 4, rng, replen=300)),
        ("planted26", planted(30000, 26, rng, replen=1000)),
    ]
    for sigma in (2, 3, 5, 17, 40, 200):
        for n in (50, 700, 6000):
            c.append(("rand_s%d_n%d" % (sigma, n), bytes(rng.randrange(1, 1 + sigma) for _ in range(n))))
    return c


def random_small(count, seed):
    rng = random.Random(seed)
    out = []
    for i in range(count):
        kind = rng.randrange(5)
        n = rng.randrange(1, 600)
        sigma = rng.randrange(1, 6)
        if kind == 0:
            s = bytes(rng.randrange(97, 97 + sigma) for _ in range(n))
        elif kind == 1:
            s = planted(n, sigma, rng, replen=rng.randrange(2, 50))
        elif kind == 2:
            s = run_rich(n, rng)
        elif kind == 3:
            w = bytes(rng.randrange(97, 97 + sigma) for _ in range(rng.randrange(1, 8)))
            s = (w * (n // len(w) + 1))[:n]
        else:
            s = bytes(rng.choice([0, 255, 97, 98]) for _ in range(n))
        out.append(("r%d" % i, s))
    return out


# ---- generators of the alphabet / code-depth tests (tests/test_gpu_alphabets.py); numpy, deterministic for a seed -------------------

def chain_counts(k, slack=0.05, extra=2):
    """k counts 1, 1, ... in which every count exceeds, by a fraction `slack` and at least 1, the sum of all counts but its
    predecessor plus `extra` (the weight of the few literals outside the chain: the sentinel, ...): Huffman merges them as a chain,
    the rarest symbols get codes of about k - 1 bits.  (Fibonacci numbers leave a margin of exactly 1 and lose depth to any literal
    the plan did not count.)"""
    c = [1, 1][:k]
    while len(c) < k:
        rest = sum(c) - c[-1] + extra
        c.append(max(c[-1], rest + 1 + int(rest * slack)))
    return c


def deep_code_text(target_longest, seed=1, slack=0.05, copy_len=48, seg=(120, 230)):
    """Raw bytes (no 0x00 / 0xFF) whose lcpcomp literals have a chain-shaped histogram -- Huffman codes of `target_longest` bits at
    thresholds 24..copy_len (the tests read the depth from the stream) -- and that still has factors: segments of `seg` shuffled
    literals over the byte values 0x80.. with chain_counts(target_longest) occurrences (the sentinel and a 'z' are the extra two), each followed by a run of `copy_len` bytes 'z'.  No literal
    byte occurs in a run, so a factor (threshold up to copy_len) covers a run and never a rare literal, and the runs add a literal
    or two themselves; two segments plus a run stay below 512 bytes, the longest literal run the device parse takes (fdist_max)."""
    rng = np.random.default_rng(seed)
    counts = chain_counts(target_longest, slack)
    lits = np.repeat(np.arange(0x80, 0x80 + len(counts), dtype=np.uint8), counts)
    rng.shuffle(lits)
    run = np.full(copy_len, ord("z"), dtype=np.uint8)
    cuts = np.cumsum(rng.integers(seg[0], seg[1] + 1, size=len(lits) // seg[0] + 2))
    cuts = cuts[cuts < len(lits)]
    parts = []
    for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(lits)]])):
        parts.append(lits[a:b])
        parts.append(run)
    return np.concatenate(parts)


def alphabet_text(n, sigma, dist="uniform", seed=1, escapes=False, zipf_s=1.1):
    """n raw bytes over sigma - 1 byte values, so that the escaped, 0-terminated text has exactly `sigma` symbols counting the
    sentinel.  dist: "uniform" or "zipf" (rank r drawn with weight 1 / r^zipf_s).  escapes=True puts 0x00 and 0xFF among the values
    and leaves 0xFE out (the escaping writes 0x00 as FF FE and 0xFF as FF FF: the alphabet keeps its size, the text grows and
    gains 0xFF literals); sigma = 256 needs it (255 values besides the sentinel)."""
    rng = np.random.default_rng(seed)
    k = sigma - 1
    if escapes or k > 253:
        assert k >= 2
        vals = np.concatenate([[0x00, 0xFF], rng.permutation(np.arange(1, 0xFE))[:k - 2]]).astype(np.uint8)
    else:
        vals = rng.permutation(np.arange(1, 0xFE))[:k].astype(np.uint8)
    rng.shuffle(vals)
    if dist == "uniform":
        idx = rng.integers(0, k, size=n)
    else:
        w = 1.0 / np.arange(1, k + 1) ** zipf_s
        idx = rng.choice(k, size=n, p=w / w.sum())
    out = vals[idx]
    out[:k] = vals                                   # every value occurs
    return out
