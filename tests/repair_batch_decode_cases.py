"""Streams for the batch decoder of repair (tudocomp_amd/csrc/repair_batch_decode.hip) and what they must yield, from code that is not
under test: tests/models/repair.py (the coders and the reference's decode loop), the host loop's grammars (tests/repair_batches.py) and
tests/models/repair_batch_decode.py.  tests/test_repair_batch_decode_cli.py checks the expectations on the CPU,
tests/test_gpu_repair_batch_decode.py runs the streams."""
import functools
import random

import numpy as np

import tudocomp_amd as T
from tests import repair_batches as RB
from tests import repair_damage as RD
from tests.models import repair as M
from tests.models import repair_batch_decode as B
from tests.models.lzss_coders import terminate

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = B.ERR_ARG, B.ERR_TOO_LARGE, B.ERR_OOM, B.ERR_UNSUPPORTED
CODERS = B.CODERS
CODER_ID = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
KNOWN = (b"abcabcabcabc", b"", b"the cat sat on the mat, the cat sat")
RULE_COUNTS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097)   # bit: both sides of every index width's border, and of 4096
DEPTH = 40
# the damaged streams of tests/repair_damage.py per coder, and how many of them a device cap separates from the host's verdict
DAMAGED = {"bit": 1695, "gamma": 2493, "delta": 2598}
EXCEPTED_MOST = 0.05


def pack(streams, align=8, order=None):
    """the streams in one blob, each at a multiple of `align`, 0xEE in between: (blob, s_off, s_len).  order: the sequence in which the
    streams lie in the blob (a permutation of their indices); s_off / s_len stay in the streams' order"""
    s_off, pos = [0] * len(streams), 0
    for k in (order if order is not None else range(len(streams))):
        s_off[k] = pos
        pos += -(-len(streams[k]) // align) * align if align > 1 else len(streams[k])
    blob = np.full(max(pos, 1), 0xEE, dtype=np.uint8)
    for o, s in zip(s_off, streams):
        blob[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return blob, np.array(s_off, dtype=np.uint64), np.array([len(s) for s in streams], dtype=np.uint64)


def stream_of(text, coder):
    """the model's coder on the host loop's grammar of `text`"""
    return RB.stream(bytes(text), coder)


def known(coder):
    return [stream_of(x, coder) for x in KNOWN]


def expand(rules, start):
    ln = M.expansion_lengths(rules)
    assert sum(1 if x < 256 else ln[x - 256] for x in start) < 1 << 24
    out, memo = bytearray(), {}

    def of(x):
        if x < 256:
            return bytes([x])
        if x not in memo:
            l, r = rules[x - 256]
            memo[x] = of(l) + of(r)
        return memo[x]
    for k in range(len(rules)):                                       # bottom-up, so that of() never recurses deeper than one rule
        if ln[k] <= 4096:
            of(256 + k)
    for x in start:
        out += of(x)
    return bytes(out)


# ---- foreign grammars: no compressor writes them, every decoder reads them -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def foreign(nrules, seed=0, nstart=40):
    """(rules, start, text): sides drawn among the bytes and the rules in front (expansions kept below 64 bytes), some rules used twice
    and more, most never"""
    rng = random.Random(1000 * nrules + seed)
    rules, ln = [], []
    for i in range(nrules):
        sides = []
        for _ in range(2):
            cand = rng.randrange(max(0, i - 50), i) if i and rng.random() < 0.6 else None
            sides.append(256 + cand if cand is not None and ln[cand] <= 32 else rng.randrange(97, 123))
        rules.append(tuple(sides))
        ln.append(sum(1 if x < 256 else ln[x - 256] for x in sides))
    picks = [rng.randrange(nrules) for _ in range(6)] if nrules else []
    start = [256 + rng.choice(picks) if picks and rng.random() < 0.5 else rng.randrange(65, 91) for _ in range(nstart)]
    if nrules:
        start.append(256 + nrules - 1)                                # the last rule: the widest index of the start sequence
    return tuple(rules), tuple(start), expand(rules, start)


def foreign_stream(nrules, coder, seed=0):
    rules, start, text = foreign(nrules, seed)
    return M.encode(list(rules), list(start), coder), text


# ---- long streams: the wave's LDS window (260 words) is refilled every kilobyte ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_streams(coder):
    """[(stream, text)] above 5 KiB each: one of literals alone, one of indices almost alone (4097 rules, 3000 start symbols that name
    rules), one ordinary grammar (9000 bytes of English).  The test lays them at all four byte offsets from a word border, so that the
    window's refills fall at other bits of the count field, the literals and the indices every time."""
    lit = bytes(random.Random(5).randrange(256) for _ in range(6000))          # no pair twice to speak of: literals
    rules, start, _ = foreign(4097, 1)
    idx_start = [256 + random.Random(6).randrange(4097) for _ in range(3000)]
    out = [(M.encode([], list(lit), coder), lit), (M.encode(list(rules), idx_start, coder), expand(rules, idx_start)),
           (stream_of(RB.english(9000, 77), coder), RB.english(9000, 77))]
    assert all(len(s) > 5 * 1024 for s, _ in out)
    return out


# ---- empty and minimal streams -----------------------------------------------------------------------------------------------------------
def minimal(coder):
    """[(stream, status)]"""
    return [(b"", ERR_ARG), (M.encode([], [], coder), 0), (b"\x06", ERR_ARG), (b"\x07", ERR_ARG)]


# ---- an index is checked against its own stream ----------------------------------------------------------------------------------------------
def own_stream_batch(coder):
    """(streams, statuses, texts): between good streams, a first rule that names rule 0, a start symbol that names rule R_k, and a side of
    rule 1 that names rule 1 -- valid only against the rules of the stream in front of it"""
    good = stream_of(b"abcabcabcabcabcabc", coder)
    first = M.encode([(256, 97)], [256], coder)
    at_r = M.encode([(97, 98)], [256, 257], coder)
    neighbour = M.encode([(97, 98), (257, 99)], [257], coder)
    text = b"abcabcabcabcabcabc"
    return [good, first, good, at_r, good, neighbour, good], [0, ERR_ARG, 0, ERR_ARG, 0, ERR_ARG, 0], [text, b"", text, b"", text, b"", text]


# ---- depth -----------------------------------------------------------------------------------------------------------------------------------
def chain(d, used=True):
    """A_0 = ab, A_i = A_{i-1} x: height d.  used=False: nothing names the chain, the start sequence is two bytes"""
    rules = [(97, 98)] + [(256 + i - 1, 120) for i in range(1, d)]
    start = [256 + d - 1] if used else [121, 122]
    return rules, start, (b"ab" + b"x" * (d - 1) if used else b"yz")


def depth_batch(coder, d=DEPTH):
    """(streams, texts, statuses at cap d, statuses at cap d - 1)"""
    a, b = stream_of(KNOWN[0], coder), stream_of(KNOWN[2], coder)
    r1, s1, t1 = chain(d)
    r2, s2, t2 = chain(d, used=False)
    r3, s3, t3 = chain(d - 1)
    streams = [a, M.encode(r1, s1, coder), b, M.encode(r2, s2, coder), M.encode(r3, s3, coder), a]
    return streams, [KNOWN[0], t1, KNOWN[2], t2, t3, KNOWN[0]], [0] * 6, [0, ERR_UNSUPPORTED, 0, ERR_UNSUPPORTED, 0, 0]


# ---- claims: the doubling grammar, rule 0 = (a, a), rule k = (k - 1, k - 1): rule k stands for 2^(k + 1) bytes ----------------------------------
def doubling(top, start, coder):
    """rules 0 .. top, the start sequence given as rule numbers"""
    rules = [(97, 97)] + [(256 + k - 1, 256 + k - 1) for k in range(1, top + 1)]
    return M.encode(rules, [256 + k for k in start], coder)


def bad_and_large(coder):
    """the doubling grammar with start = [rule 30, rule 30] (2^32 bytes) and a first rule that names rule 0"""
    rules = [(256, 97)] + [(256 + k - 1, 256 + k - 1) for k in range(1, 31)]
    return M.encode(rules, [256 + 30, 256 + 30], coder)


MOVE_TOP = 21                                                         # rule 21: 4 MiB of text from some 40 bytes of stream


def two_bit_tokens(n):
    """a gamma stream of one rule and n start symbols "11" (the rule 0, as no encoder writes it): four tokens per stream byte"""
    bits = M.encode_bits([(97, 98)], [], "gamma") + "11" * n
    return terminate(bits)


# ---- the damaged streams -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def damaged(coder):
    """(streams, statuses, texts, excepted): a good stream, every stream of repair_damage.damaged_streams, a good stream; the verdicts
    are tests/models/repair_batch_decode.expected's on each stream alone"""
    good = stream_of(KNOWN[2], coder)
    streams = [good] + [s for _, s in RD.damaged_streams(coder)] + [good]
    verdicts = [B.expected(s, coder) for s in streams]
    return streams, [v[0] for v in verdicts], [v[1] for v in verdicts], sum(v[2] for v in verdicts)
