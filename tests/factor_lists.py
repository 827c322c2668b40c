"""Hand-shaped factor lists for the stage entry points (tdc_gpu_flatten, tdc_gpu_encode_*) and the decoder, plus a plain reference
of what a list means.

The factorizers only ever emit lists of a few shapes (lengths >= threshold, a suffix-array neighbour as the source, chain depths
and literal runs set by the text).  The shapes here are the ones the kernels' assumptions meet rarely: staircases of factors that
each wait for the one before, chains of a million steps through one self-overlapping factor, forward chains, equal lengths,
extreme sources, literal runs of exactly 512 / 513, position chains of depth ~2^24.

Every case follows the entry points' contract: an escaped text (literal bytes 1..254, so no 0 and no escape byte) that ends with
a 0 sentinel which is a literal, factors sorted by position, disjoint, inside the text, and acyclic.  `resolve` is the reference:
numpy pointer jumping over per-position references, independent of the oracle and of the device.  A case's text is what its
list resolves to, so a list and its text always agree.

No GPU and nothing from tudocomp_amd is needed here.
"""
import numpy as np

MAX_FACTOR = 1 << 22          # longest single factor handed to the stand-alone entry points (one thread scatters a factor)


class CycleError(ValueError):
    """some text position never reaches a literal"""


def _arrays(pos, src, length):
    return (np.asarray(pos, dtype=np.int64).reshape(-1), np.asarray(src, dtype=np.int64).reshape(-1),
            np.asarray(length, dtype=np.int64).reshape(-1))


def check_list(n, pos, src, length):
    """raises ValueError unless (pos, src, len) is a list the entry points accept for a text of n positions"""
    pos, src, length = _arrays(pos, src, length)
    if not (len(pos) == len(src) == len(length)):
        raise ValueError("pos / src / len differ in length")
    if len(pos) == 0:
        return
    if (length <= 0).any():
        raise ValueError("factor of length 0")
    if (pos[1:] < pos[:-1] + length[:-1]).any():
        raise ValueError("factors not sorted or overlapping")
    if (pos < 0).any() or (pos + length > n).any() or (src < 0).any() or (src + length > n).any():
        raise ValueError("factor or source outside the text")


def resolve(n, literals, pos, src, length):
    """The text a factor list means: literals[p] at every position no factor covers, text[src + j] at pos + j.  Pointer jumping
    (ref <- ref[ref]) halves every chain per round, so a chain of depth d is done after ceil(log2 d) + 1 rounds; a position still
    not at a literal after that is on a cycle (CycleError)."""
    lit = np.frombuffer(bytes(literals), dtype=np.uint8) if isinstance(literals, (bytes, bytearray)) else np.asarray(literals, dtype=np.uint8)
    if len(lit) != n:
        raise ValueError("literals must hold n bytes")
    check_list(n, pos, src, length)
    pos, src, length = _arrays(pos, src, length)
    ref = np.arange(n, dtype=np.int32)
    is_lit = np.ones(n, dtype=bool)
    if len(pos):
        tot = int(length.sum())
        first = np.repeat(np.cumsum(length) - length, length)
        off = np.arange(tot, dtype=np.int64) - first
        q = np.repeat(pos, length) + off
        ref[q] = (np.repeat(src, length) + off).astype(np.int32)
        is_lit[q] = False
    for _ in range(int(n).bit_length() + 2):
        if is_lit[ref].all():
            return lit[ref].tobytes()
        ref = ref[ref]
    if is_lit[ref].all():
        return lit[ref].tobytes()
    raise CycleError("%d positions never reach a literal" % int((~is_lit[ref]).sum()))


# ---- shapes -------------------------------------------------------------------------------------------------------------------
class _Layout:
    """factor spans and the literal bytes of one proposal"""

    def __init__(self, n, rng, alphabet=None):
        self.n = n
        if alphabet is None:
            self.lits = rng.integers(1, 255, size=n, dtype=np.uint8)          # 1..254
        else:
            self.lits = rng.choice(np.asarray(alphabet, dtype=np.uint8), size=n)
        self.lits[n - 1] = 0
        self.pos, self.src, self.len = [], [], []

    def add(self, p, s, l):
        self.pos.append(int(p)); self.src.append(None if s is None else int(s)); self.len.append(int(l))


def _assign_sources(L, rng, forward_share, extreme_share=0.0, overlap_share=0.0):
    """Sources for the spans of L (whose src entries are None) that keep the list acyclic by construction: a forward factor
    (src > pos) moves every chain that runs through it to a later position, a backward one (src < pos) to an earlier one, so a
    chain can only cycle by entering a forward factor from a backward one.  Backward sources therefore avoid the forward spans."""
    n = L.n
    z = len(L.pos)
    fwd = np.zeros(z, dtype=bool)
    for i in range(z):
        p, l = L.pos[i], L.len[i]
        can_fwd = p + 1 + l <= n - 1
        fwd[i] = can_fwd and (p == 0 or rng.random() < forward_share)
    fmask = np.zeros(n + 1, dtype=np.int64)
    for i in np.nonzero(fwd)[0]:
        fmask[L.pos[i]:L.pos[i] + L.len[i]] = 1
    fsum = np.concatenate([[0], np.cumsum(fmask)])

    def clean(s, l):                                                    # no forward span in [s, s + l)
        return fsum[s + l] - fsum[s] == 0

    keep = np.ones(z, dtype=bool)
    for i in range(z):
        p, l = L.pos[i], L.len[i]
        hi = n - 1 - l                                                  # the sentinel is never copied
        if fwd[i]:
            r = rng.random()
            if r < extreme_share:
                s = hi                                                  # src = n - len - 1
            elif r < extreme_share + overlap_share:
                s = p + int(rng.integers(1, 4))                         # forward self-overlap
                s = min(s, hi)
            else:
                s = int(rng.integers(p + 1, hi + 1))
            L.src[i] = s
            continue
        cands = []
        r = rng.random()
        if r < extreme_share:
            cands.append(0)
        elif r < extreme_share + overlap_share:
            cands.append(p - int(rng.integers(1, 4)))                   # backward self-overlap
        cands += [int(rng.integers(0, p)) for _ in range(24)] if p > 0 else []
        for s in cands:
            if 0 <= s < p and s + l <= n - 1 and clean(s, l):
                L.src[i] = s
                break
        else:
            keep[i] = False                                             # no clean source: the span stays literal
    L.pos = [x for x, k in zip(L.pos, keep) if k]
    L.src = [x for x, k in zip(L.src, keep) if k]
    L.len = [x for x, k in zip(L.len, keep) if k]


def _no_factors(n, rng):
    return _Layout(n, rng)


def _one_literal(n, rng):
    x = int(rng.integers(1, 255))
    L = _Layout(n, rng, alphabet=[x])
    if n >= 3:
        L.add(1, 0, n - 2)
    return L


def _one_literal_len1(n, rng):
    """every position after the first a factor of length 1 copying the position before it: a staircase of n - 2 factors"""
    x = int(rng.integers(1, 255))
    L = _Layout(n, rng, alphabet=[x])
    for p in range(1, n - 1):
        L.add(p, p - 1, 1)
    return L


def _equal_lengths(n, rng, flen):
    L = _Layout(n, rng)
    p = int(rng.integers(1, 64))
    while True:
        p += int(rng.integers(0, 4))
        if p + flen > n - 1:
            break
        L.add(p, None, flen)
        p += flen
    _assign_sources(L, rng, forward_share=0.15, overlap_share=0.2)
    return L


def _extreme_sources(n, rng, p0=0):
    L = _Layout(n, rng)
    p = p0                                                              # (a factor at position 0 is a forward one)
    while True:
        l = int(rng.choice([1, 2, 3, 7, 16, 64, 300]))
        if p + l > n - 1 - 8:
            break
        L.add(p, None, l)
        p += l + int(rng.integers(0, 12))
    _assign_sources(L, rng, forward_share=0.4, extreme_share=0.5)
    return L


def _overlap_runs(n, rng):
    """backward runs src = pos - d and forward runs src = pos + d (d = 1..3), each forward run followed by >= d literals"""
    L = _Layout(n, rng)
    p = 64
    k = 0
    while True:
        d = int(rng.integers(1, 4))
        l = int(rng.integers(1000, 20000))
        if p + l + 8 > n - 1:
            break
        if k % 2 == 0:
            L.add(p, p - d, l)                                          # p - d .. p - 1 are literals (the gap before)
        else:
            L.add(p, p + d, l)                                          # runs out onto the literals behind it
        p += l + 3 + int(rng.integers(0, 4))
        k += 1
    return L


def _staircase(n, rng, K=2000, flen=16):
    """factor k copies factor k - 1 exactly: every factor waits for the final source of the one before (one flatten round each)"""
    n = 64 + K * (flen + 2) + 2
    L = _Layout(n, rng)
    s0 = int(rng.integers(0, 64 - flen + 1))
    p = 64
    for k in range(K):
        L.add(p, s0 if k == 0 else L.pos[-1], flen)
        p += flen + int(rng.integers(0, 3))
    return L


def _forward_chain(n, rng, K=3000, flen=16):
    """factor k copies factor k + 1, the last one a literal block before the sentinel: chains through all later factors"""
    n = 16 + K * (flen + 2) + flen + 1
    L = _Layout(n, rng)
    p = 16
    for k in range(K):
        L.add(p, None, flen)
        p += flen + int(rng.integers(0, 3))
    for k in range(K - 1):
        L.src[k] = L.pos[k + 1]
    L.src[K - 1] = n - 1 - flen
    return L


MILLION = 1 << 20


def _million_steps(n, rng, big=MILLION):
    """one factor F = (P, P + 1, big) -- a forward self-overlap that runs out onto the literal behind it -- and short factors
    before and after it whose sources lie near F's start: each flattens through ~big single steps"""
    P = 256 + 4 * 20
    n = P + big + 64 + 4 * 20 + 32
    L = _Layout(n, rng)
    p = 256
    for _ in range(4):                                                  # before F (F is a later factor for them)
        l = int(rng.integers(2, 9))
        L.add(p, P + int(rng.integers(0, 8)), l)
        p += 20
    L.add(P, P + 1, big)
    p = P + big + 64
    for _ in range(4):                                                  # after F (F is final when they need it)
        l = int(rng.integers(2, 9))
        L.add(p, P + int(rng.integers(0, 8)), l)
        p += 20
    return L


def million_steps_expected(pos, src, length, big=MILLION):
    """final sources and depths of million_steps' short factors: a copy of len l at offset d0 in F steps one position at a time
    while d + l <= big, so it ends at offset big - l + 1 after big - l + 1 - d0 steps"""
    i = int(np.nonzero(np.asarray(length) == big)[0][0])
    P = int(pos[i])
    fin, dep = np.asarray(src, dtype=np.int64).copy(), np.zeros(len(pos), dtype=np.int64)
    for k in range(len(pos)):
        if k == i:
            continue
        l, d0 = int(length[k]), int(src[k]) - P
        fin[k] = P + big - l + 1
        dep[k] = big - l + 1 - d0
    return fin, dep


def _deep_decode(n, rng, direction):
    """one position chain through the whole text: src = pos - 1 (back) or src = pos + 1 (fwd), cut into factors of MAX_FACTOR"""
    L = _Layout(n, rng)
    if direction == "back":
        p = 1
        while p < n - 1:
            l = min(MAX_FACTOR, n - 1 - p)
            L.add(p, p - 1, l)
            p += l
    else:
        p = 0
        while p < n - 2:
            l = min(MAX_FACTOR, n - 2 - p)
            L.add(p, p + 1, l)
            p += l
    return L


def _run(n, rng, longest):
    """near-incompressible literals in runs of 1..512 between backward factors; the longest run is exactly `longest`: for 512 an
    inner run and the tail run, for 513 the tail run alone (the header's fdist_max counts the tail, sentinel included)"""
    runs, flens = [], []
    total = 0
    while total < n:
        r = int(rng.integers(1, 513))
        l = int(rng.integers(4, 65))
        runs.append(r); flens.append(l)
        total += r + l
    runs[len(runs) // 2] = 512
    tail = longest
    n = sum(runs) + sum(flens) + tail
    L = _Layout(n, rng)
    p = 0
    for r, l in zip(runs, flens):
        p += r
        L.add(p, int(rng.integers(0, p - l + 1)) if p >= l else 0, l)
        p += l
    assert n - p == tail
    return L


def _random_mix(n, rng):
    L = _Layout(n, rng)
    p = int(rng.integers(0, 3))
    cap = min(MAX_FACTOR, max(4, n // 32))
    while True:
        kind = rng.random()
        if kind < 0.25:
            l = 1
        elif kind < 0.6:
            l = int(rng.integers(2, 32))
        elif kind < 0.97:
            l = int(rng.integers(32, 512))
        else:
            l = int(rng.integers(512, cap + 1)) if cap > 512 else int(rng.integers(2, cap + 1))
        if p + l > n - 2:
            break
        L.add(p, None, l)
        p += l + int(rng.choice([0, 0, 1, 2, 5, 40]))
    _assign_sources(L, rng, forward_share=0.3, extreme_share=0.05, overlap_share=0.15)
    return L


_SHAPES = {
    "no_factors": lambda n, rng, **k: _no_factors(n, rng),
    "one_literal": lambda n, rng, **k: _one_literal(n, rng),
    "one_literal_len1": lambda n, rng, **k: _one_literal_len1(n, rng),
    "equal_lengths": lambda n, rng, **k: _equal_lengths(n, rng, k["flen"]),
    "extreme_sources": lambda n, rng, **k: _extreme_sources(n, rng, **k),
    "overlap_runs": lambda n, rng, **k: _overlap_runs(n, rng),
    "staircase": lambda n, rng, **k: _staircase(n, rng, **k),
    "forward_chain": lambda n, rng, **k: _forward_chain(n, rng, **k),
    "million_steps": lambda n, rng, **k: _million_steps(n, rng, **k),
    "deep_decode": lambda n, rng, **k: _deep_decode(n, rng, k["direction"]),
    "run_512": lambda n, rng, **k: _run(n, rng, 512),
    "run_513": lambda n, rng, **k: _run(n, rng, 513),
    "random_mix": lambda n, rng, **k: _random_mix(n, rng),
}
SHAPES = tuple(_SHAPES)


def make_case(shape, n, seed=1, **kw):
    """(text, pos, src, len) of one shape: text is bytes (escaped, 0-terminated), the list uint32 arrays sorted by position.
    A proposal that `resolve` rejects is drawn again from the next seed of the stream, never returned."""
    rng = np.random.default_rng([seed, n, SHAPES.index(shape)])
    for _ in range(16):
        L = _SHAPES[shape](n, rng, **kw)
        pos, src, length = (np.asarray(a, dtype=np.uint32) for a in (L.pos, L.src, L.len))
        try:
            text = resolve(L.n, L.lits, pos, src, length)
        except CycleError:
            continue
        assert text[-1] == 0 and text.count(0) == 1, shape
        return text, pos, src, length
    raise RuntimeError("make_case(%s): no acyclic proposal in 16 draws" % shape)


def cases(scale="gpu"):
    """(case id, shape, n, kwargs) of the suite.  scale "cpu" shrinks the large shapes to what the oracle checks in seconds."""
    big = scale == "gpu"
    out = [("no_factors-n%d" % n, "no_factors", n, {}) for n in (1, 2, 513, 70_000)]
    out += [("one_literal-n%d" % n, "one_literal", n, {}) for n in ((3, 70_000, MAX_FACTOR + 2) if big else (3, 70_000))]
    out += [("one_literal_len1-n2000", "one_literal_len1", 2000, {})]
    out += [("equal_lengths-L%d" % l, "equal_lengths", max(20_000, 48 * (l + 2)), {"flen": l}) for l in (1, 2, 255, 256, 4096, 4097)]
    out += [("extreme_sources-n%d" % n, "extreme_sources", n, {"p0": p0}) for n, p0 in ((5_000, 0), (300_000, 5))]
    out += [("overlap_runs", "overlap_runs", 200_000, {})]
    out += [("staircase", "staircase", 0, {"K": 2000 if big else 300})]
    out += [("forward_chain", "forward_chain", 0, {"K": 3000 if big else 300})]
    out += [("million_steps", "million_steps", 0, {"big": MILLION if big else 1 << 14})]
    nd = (1 << 24) if big else (1 << 16)
    out += [("deep_decode-%s" % d, "deep_decode", nd, {"direction": d}) for d in ("back", "fwd")]
    nr = (1 << 22) if big else (1 << 15)
    out += [("run_512", "run_512", nr, {}), ("run_513", "run_513", nr, {})]
    out += [("random_mix-n%d-s%d" % (n, s), "random_mix", n, {}) for n, s in
            (((1 << 10, 1), (1 << 10, 2), (1 << 14, 3), (1 << 18, 4), (1 << 22, 5)) if big else ((1 << 10, 1), (1 << 10, 2), (1 << 14, 3)))]
    return out


def case_seed(case_id):
    return sum(case_id.encode()) * 7919 + len(case_id)
