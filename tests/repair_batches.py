"""Batches for the repair batch calls (tudocomp_amd/csrc/repair_batch.hip) and what they must yield, from code that is not under test:
the host loop tdc_repair_grammar (module-level T.repair_grammar) for the grammars, tests/models/repair.py for the streams, and
tests/golden/repair_kats.json where it has the case.  Every batch is named for what it reaches; tests/test_repair_batch_cli.py checks on
the CPU that it does, tests/test_repair_batch_model.py runs the model of the kernel on them, tests/test_gpu_repair_batch.py the kernel."""
import functools

import numpy as np

import tudocomp_amd as T
from tests.models import repair as M
from tests.util import load_json

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
TEXT_CAP = 1 << 24                              # the longest text of a batch (include/tdc_gpu.h)
CID = {"bit": T.CODER_BIT, "ascii": T.CODER_ASCII, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
WORKGROUP, CHUNK = 256, 2048                    # threads of a workgroup; positions per chunk of its scans (8 per thread)
RUNS = tuple(range(1, 71)) + (255, 256, 257, 1023, 1024, 1025)


def english(n, seed=42):
    return T.gen_english(n, seed).tobytes()


def dna(n, seed=7):
    return T.gen_dna(n, seed).tobytes()


def rnd(n, sigma, seed):
    return np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def tie_text():
    """every two-letter word over 16 letters, twice, shuffled: hundreds of pairs that count the same (as tests/test_gpu_repair.py)"""
    letters = b"abcdefghijklmnop"
    words = [bytes((x, y)) for x in letters for y in letters] * 2
    order = np.random.default_rng(16).permutation(len(words))
    return b"".join(words[i] for i in order)


@functools.lru_cache(maxsize=None)
def kat_cases():
    return tuple((c["text"].encode(), tuple(tuple(x) for x in c["rules"]), tuple(c["start"])) for c in load_json("repair_kats.json")["cases"])


def _known():
    out = [x for x, _, _ in kat_cases()] + [tie_text(), tie_text() + tie_text()[::-1]]
    out += [b"a" * k for k in RUNS + (65535, 65536, 65537)]
    for k in (1, 2, 3, 4, 5, 6, 7, 100, 1000, 4097):                  # adjacent pairs
        out += [b"ab" * k, b"ab" * k + b"a", b"b" + b"ab" * k]
    for k in (2, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049):            # runs inside a text
        out.append(b"xy" * 3 + b"a" * k + b"yx" * 3 + b"a" * (k + 1) + b"b")
    return out


def _split_runs():
    """a^k cut in two neighbouring texts, between other texts: a run must not reach over a border"""
    out = []
    for k in RUNS:
        out += [b"a" * (k // 2), b"a" * (k - k // 2)]
        if k % 7 == 0:
            out.append(b"ba")
    return out


def _same_at_three_places():
    x = english(1500, 5)
    return [x, b"a" * 40, english(300, 6), x, x[-20:] * 3, b"", x, x[:20] * 2]


def _smallest():
    long = (english(700, 8), dna(900, 9), b"ab" * 200)
    out = []
    for j, n in enumerate((0, 1, 2, 3, 0, 1, 2, 3, 2, 3)):
        out += [long[j % 3], (b"aaa", b"aba", b"abc", b"bbb")[j % 4][:n]]
    return out + [long[0]]


def _forks():
    """lengths at the workgroup size and at the borders of its scan chunks, for texts that take the plain mark and for runs that take
    the chunked one -- with the run's first position even and odd, and runs that reach over one, two and three chunk borders"""
    out = []
    for n in (WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1):
        out += [english(n, n), b"a" * n, b"b" + b"a" * (n - 1), b"bc" + b"a" * (n - 3) + b"b"]
    for lead in (0, 1, 2, 7, 2047, 2048):
        out.append(b"b" * lead + b"a" * 6200 + b"cb" * 5)
    out.append((b"a" * 2047 + b"b") * 3 + b"a" * 2049)
    return out


def _long_among_short():
    rng = np.random.default_rng(70001)
    short = [english(int(n), 100 + j) for j, n in enumerate(rng.integers(0, 400, 200))]
    return short[:77] + [english(70001, 77)] + short[77:]


def _random300():
    rng = np.random.default_rng(300)
    lens = rng.integers(0, 3001, 300)
    out = []
    for j, n in enumerate(lens):
        n = int(n)
        out.append((english(n, 1000 + j), dna(n, 2000 + j), rnd(n, 16, 3000 + j))[j % 3])
    return out


def _capped():
    """for max_rules 1, 64 and 512: texts that reach the cap, and texts that need fewer rules than it -- none at all among them"""
    return list(_random300()[::10]) + [b"", b"a", b"abcd", b"abab", b"ab" * 40, english(16384, 512)]


_BATCHES = {
    "count0": lambda: [],
    "count1": lambda: [english(1000, 1)],
    "only_empties": lambda: [b""] * 5,
    "known": _known,
    "no_pair_across": lambda: [b"ab"] * 50,                      # no text has a repeated pair, the concatenation has 49
    "a_next_to_a": lambda: [b"xyza", b"abab", b"banana", b"a", b"a", b"aa", b"a" * 5, b"aab"],
    "split_runs": _split_runs,
    "same_at_three_places": _same_at_three_places,
    "smallest": _smallest,
    "forks": _forks,
    "long_among_short": _long_among_short,
    "random300": _random300,
    "capped": _capped,
}
NAMES = tuple(_BATCHES)


@functools.lru_cache(maxsize=None)
def batch(name):
    return tuple(_BATCHES[name]())


# ---- what a text must yield ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host(x, max_rules=0):
    """the specification, computed once per text: (rules, start) of tdc_repair_grammar"""
    r, s = T.repair_grammar(x, max_rules)
    r.setflags(write=False)
    s.setflags(write=False)
    return r, s


def as_model(rules, start):
    return [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in rules], [int(x) for x in start]


@functools.lru_cache(maxsize=None)
def stream(x, coder, max_rules=0):
    """the model's coder on the host loop's grammar"""
    return M.encode(*as_model(*host(x, max_rules)), coder)


def text_bound(n, coder):
    """tdc_gpu_repair_bound restated (2 n + 1 fields at their widest, 16 bytes for the count's excess and the terminator), rounded up
    to 8; 0 above 2^30"""
    if n > 1 << 30:
        return 0
    per = {"bit": 32, "ascii": 96, "gamma": 64, "delta": 43}[coder]
    return (((2 * n + 1) * per + 7) // 8 + 16 + 7) // 8 * 8
