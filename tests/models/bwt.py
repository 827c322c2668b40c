"""Executable model of the bwt compressor (tudocomp_amd/csrc/bwt.hip).

numpy / pure Python, small texts only.  The inverse follows the data flow of the kernels step by step:
  1. byte histogram -> C[c] = number of bytes smaller than c; exactly one 0 byte or the input is refused;
  2. LF[i] = C[b[i]] + #{j < i : b[j] = b[i]} (a stable counting rank: here a stable argsort, inverted);
  3. list heads: row i is a head iff mix(i) < T, where mix is a bijection of [0, 2^m) (2^m >= n) with mix(0) = 0 and
     T = ceil(2^m / S) -- the head's slot in the table IS mix(i), so nothing has to be enumerated or looked up;
  4. bounded walks: every head follows LF until it meets a head (link = that head's slot) or has taken max_steps steps (the row where
     it stops becomes a head of its own, appended behind the hashed slots, and is walked by the next launch);
  5. the heads are ranked by pointer jumping over (link, length) words; the list of slot 0 is cut where it comes back to row 0;
  6. valid iff the jumping converged and the list of slot 0 holds n rows (a permutation with a second cycle does not);
  7. second walk: head with offset r writes the byte of its k-th row to out[n - 2 - (r + k)] (the last row of the cycle holds the 0, which
     goes to out[n - 1]); the byte of a row is the c with C[c] <= LF[row] < C[c + 1].
Malformed input raises Malformed.
"""
import numpy as np

NONE = 0xFFFFFFFF
MUL_A = 0x9E3779B1
MUL_B = 0x85EBCA6B
DEFAULT_SAMPLE = 256
DEFAULT_STEPS_PER_SAMPLE = 4


class Malformed(ValueError):
    pass


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def suffix_array_naive(text):
    t = bytes(text)
    return np.array(sorted(range(len(t)), key=lambda i: t[i:]), dtype=np.int64)


def bwt_from_sa(text, sa):
    """BWTCompressor::compress: out[i] = T[SA[i] - 1], T[n - 1] where SA[i] = 0"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(t)
    return t[(np.asarray(sa, dtype=np.int64) - 1) % n].tobytes() if n else b""


def bwt_forward(text):
    return bwt_from_sa(text, suffix_array_naive(text))


# ---- the plain loop (decode_bwt, ds/bwt.hpp:77-98) ----------------------------------------------------------------------------------
def lf_table(b, reference_bug=False):
    """LF by a stable argsort.  reference_bug: C as compute_LF (bwt.hpp:38) accumulates it -- the loop stops in front of the last byte
    value, so C[255] stays the bare count of byte 254."""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    n = len(a)
    if not reference_bug:
        order = np.argsort(a, kind="stable")
        lf = np.empty(n, dtype=np.int64)
        lf[order] = np.arange(n, dtype=np.int64)
        return lf
    cnt = np.bincount(a, minlength=256).astype(np.int64)
    C = np.zeros(256, dtype=np.int64)
    for c in range(256):
        C[c] = cnt[c - 1] if c else 0
    for c in range(1, 255):
        C[c] += C[c - 1]
    seen = np.zeros(256, dtype=np.int64)
    lf = np.empty(n, dtype=np.int64)
    for i in range(n):
        lf[i] = C[a[i]] + seen[a[i]]
        seen[a[i]] += 1
    return lf


def inverse_loop(b, reference_bug=False):
    """The reference's walk, one byte per step; no validation (it prints whatever it meets)"""
    n = len(b)
    if n <= 1:
        return b""
    lf = lf_table(b, reference_bug)
    out = bytearray(n)
    i = 0
    for j in range(1, n):
        out[n - 1 - j] = b[i]
        i = int(lf[i]) % n          # (the reference's table can point anywhere; the model keeps the index inside the buffer)
    out[n - 1] = 0
    return bytes(out)


# ---- the device formulation ---------------------------------------------------------------------------------------------------------
def mix_params(n):
    m = max(1, int(n - 1).bit_length())
    return m, (1 << m) - 1, (m + 1) // 2


def mix(i, n):
    """bijection of [0, 2^m) with mix(0) = 0: multiply by an odd constant, fold the upper half down, twice"""
    m, mask, h = mix_params(n)
    x = (i * MUL_A) & mask
    x ^= x >> h
    x = (x * MUL_B) & mask
    x ^= x >> h
    return x


def _inv_odd(a, mask):
    x = a & mask
    for _ in range(6):
        x = (x * (2 - a * x)) & mask
    return x


def unmix(k, n):
    m, mask, h = mix_params(n)
    x = k ^ (k >> h)
    x = (x * _inv_odd(MUL_B, mask)) & mask
    x ^= x >> h
    return (x * _inv_odd(MUL_A, mask)) & mask


def head_threshold(n, sample):
    m, _, _ = mix_params(n)
    return ((1 << m) + sample - 1) // sample


def inverse_device(b, sample=0, max_steps=0, stats=None):
    """The inverse as bwt.hip computes it.  sample / max_steps: 0 = the product's choice.  stats (dict, optional) receives heads,
    launches, rounds, longest and lf."""
    n = len(b)
    if n <= 1:
        return b""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    cnt = np.bincount(a, minlength=256).astype(np.int64)
    if cnt[0] != 1:
        raise Malformed("a BWT holds exactly one 0 byte")
    C = np.concatenate([[0], np.cumsum(cnt)])
    lf = lf_table(b)
    S = sample or DEFAULT_SAMPLE
    M = max_steps or DEFAULT_STEPS_PER_SAMPLE * S
    T = head_threshold(n, S)
    hrow = [unmix(k, n) for k in range(T)]
    hrow = [r if r < n else NONE for r in hrow]
    assert hrow[0] == 0
    link = [NONE] * T
    length = [0] * T
    active = [k for k in range(T) if hrow[k] != NONE]
    launches = 0
    while active:
        launches += 1
        fresh = []
        for k in active:
            cur, steps = hrow[k], 0
            while True:
                cur = int(lf[cur])
                steps += 1
                if cur == 0:
                    break                                  # back at row 0: the list of slot 0 ends here
                if mix(cur, n) < T:
                    link[k] = mix(cur, n)
                    break
                if steps == M:
                    hrow.append(cur); link.append(NONE); length.append(0)
                    link[k] = len(hrow) - 1
                    fresh.append(len(hrow) - 1)
                    break
            length[k] = steps
        active = fresh
    H = len(hrow)
    # pointer jumping (synchronous here; the device updates in place, which only gets there sooner)
    w = [(link[k], length[k]) for k in range(H)]
    bound = H.bit_length() + 2
    rounds, converged = 0, False
    while rounds < bound:
        rounds += 1
        changed = False
        nw = list(w)
        for k in range(H):
            l, d = w[k]
            if l != NONE:
                l2, d2 = w[l]
                nw[k] = (l2, (d + d2) & 0xFFFFFFFF)
                changed = True
        w = nw
        if not changed:
            converged = True
            break
    if not converged or w[0] != (NONE, n):
        raise Malformed("the LF mapping is not one cycle of length n")
    out = bytearray(n)
    for k in range(H):
        if hrow[k] == NONE:
            continue
        r = n - w[k][1]
        cur = hrow[k]
        for j in range(length[k]):
            nxt = int(lf[cur])
            c = int(np.searchsorted(C, nxt, side="right")) - 1
            t = r + j
            out[n - 2 - t if t <= n - 2 else n - 1] = c
            cur = nxt
    if stats is not None:
        stats.update(heads=sum(1 for r in hrow if r != NONE), launches=launches, rounds=rounds, longest=max(length), lf=lf)
    return bytes(out)
