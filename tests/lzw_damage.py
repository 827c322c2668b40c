"""The damaged streams of the lzw differential tests (tests/test_gpu_lzw.py, tests/test_lzw_model.py): 150 single-bit flips and
truncations of one 200 KB stream per coder."""
import random

import tudocomp_amd as T
from tests.models import lzw as M

_cache = {}


def base_stream(coder):
    """200 KB of stream: codes from the host parse (checked against the model elsewhere), coded by the model"""
    if coder not in _cache:
        n = 430000 if coder == "bit" else 235000
        data = T.gen_english(n, 77).tobytes()
        s = M.encode(T.lzw_factors(data).tolist(), coder)
        assert 190000 <= len(s) <= 215000, len(s)
        _cache[coder] = (data, s)
    return _cache[coder]


def damaged_streams(coder, count=150, seed=5):
    _, s = base_stream(coder)
    rng = random.Random(seed)
    out = []
    for i in range(count):
        b = bytearray(s)
        if i % 3 == 2:                                    # a truncation: the last byte kept becomes the terminator
            del b[rng.randrange(1, len(b)):]
        else:                                             # a single bit; two thirds of them in the second half, where less depends on it
            at = rng.randrange(len(b) // 2, len(b) - 1) if i % 3 else rng.randrange(len(b) - 1)
            b[at] ^= 1 << rng.randrange(8)
        out.append(bytes(b))
    return out
