"""Texts and buffers for the bwt batch tests (tests/test_bwt_batch_model.py, tests/test_gpu_bwt_batch.py): escaped, 0-terminated views
of a given length (terminator included) and nature, built once."""
import functools

import numpy as np

import tudocomp_amd as T

NATURES = ("a_run", "ab", "fibonacci", "thue_morse", "random2", "random255", "english", "escapes")
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537)


def _body(nature, m, seed):
    """m bytes without a 0"""
    rng = np.random.default_rng(seed)
    if nature == "a_run":
        return b"a" * m
    if nature == "ab":
        return (b"ab" * (m // 2 + 1))[:m]
    if nature == "fibonacci":
        a, b = b"a", b"ab"
        while len(b) < m:
            a, b = b, b + a
        return b[:m]
    if nature == "thue_morse":
        return bytes(97 + (bin(i).count("1") & 1) for i in range(m))
    if nature == "random2":
        return rng.integers(97, 99, m, dtype=np.uint8).tobytes()
    if nature == "random255":
        return rng.integers(1, 256, m, dtype=np.uint8).tobytes()
    if nature == "english":
        return T.escape(T.gen_english(m + 16, seed).tobytes())[:m].replace(b"\x00", b"e")
    if nature == "escapes":                                   # FF FE (an escaped 0x00) and FF FF (an escaped 0xFF) among a few letters
        raw = rng.choice(np.array([0, 255, 97, 98], dtype=np.uint8), m, p=[0.35, 0.35, 0.15, 0.15]).tobytes()
        return (T.escape(raw)[:-1] + b"\xff\xff" * 2)[:m]
    raise KeyError(nature)


@functools.lru_cache(maxsize=None)
def text(nature, n, seed=1):
    """a view of n bytes, the terminating 0 among them (n >= 1)"""
    t = _body(nature, n - 1, seed) + b"\x00"
    assert len(t) == n and t.count(0) == 1
    return t


def model_texts():
    """small texts of every nature for the CPU model, a few hundred bytes at the most"""
    out = [b"\x00", b"a\x00", text("a_run", 4098)[-300:], text("a_run", 130)]
    for nature in NATURES:
        for n in (2, 3, 4, 5, 6, 9, 33, 64, 65, 200):
            out.append(text(nature, n, 3))
    rng = np.random.default_rng(7)
    out += [rng.integers(1, 4, 150, dtype=np.uint8).tobytes() + b"\x00" for _ in range(3)]
    return out
