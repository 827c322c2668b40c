"""Inputs that put the item count of the shared field coder (csrc/field_coder.hpp: tiles of 2048 items, 8 per thread) on a tile border,
for repair, lz78 and lzw.  The GPU tests compress them; tests/test_repair_model.py, tests/test_lzw_model.py and
tests/test_lz78_decode_model.py hold the counts -- and the two sides of the terminator rule, 5 and 6 bits in the last byte -- against
the models without a GPU."""
import functools

import numpy as np

from tests.models.lzss_coders import payload_bits

BORDERS = (2047, 2048, 2049, 4097)


def residue(stream):
    """bits used in the last payload byte: up to 5 the terminator shares that byte, from 6 on it takes one of its own"""
    return payload_bits(stream) & 7


def no_repeated_pair(n):
    """a, b, a, b', ... for every a < b: no pair of adjacent bytes occurs twice, so the grammar has no rule and n + 1 fields"""
    out = []
    for a in range(256):
        for b in range(a + 1, 256):
            out += (a, b)
    return bytes(out[:n])


def repair_borders():
    """(text, max_rules, fields): 1 + 2 rules + start symbols.  The last one holds every pair twice: 1100 rules, so that the first tile
    border lies among the rule sides."""
    return tuple((no_repeated_pair(f - 1), 0, f) for f in BORDERS) + ((no_repeated_pair(2200) * 2, 1100, None),)


@functools.lru_cache(maxsize=None)
def two_letters_64k():
    """(16 KiB of two letters parse into 1800 lz78 phrases and 1982 lzw codes only)"""
    return (np.random.default_rng(78).integers(0, 2, 64 << 10, dtype=np.uint8) + ord("a")).tobytes()


def phrase_prefixes(text, lengths, counts):
    """the prefixes of `text` that end where phrase k ends, k in counts: such a prefix parses into exactly k items"""
    ends = np.cumsum(lengths)
    return [(k, text[:int(ends[k - 1])]) for k in counts]


LZ78_COUNTS = BORDERS                           # (a pair is two codes of odd length: no lz78 stream ends with 5 bits; 2049 and 4097 end with 6)
LZW_COUNTS = (5, 6, 2046) + BORDERS             # 5 and 6 codes: residues 5 and 6 under bit; 2047 and 2046 codes: 5 and 6 under gamma
