"""The workgroup formulation of repair over a batch (tudocomp_amd/csrc/repair_batch.hip, DESIGN.md section 5.8 "Batches"), executable.

Every text has its own state -- the live sequence, compacted in place, and a digram table of the layout the kernel uses: a power of two
of slots, linear probing, exact keys, exact overlapping counts, one `last` word per slot that is 0 between rounds -- and nothing else.
What differs from device_grammar() of tests/models/repair.py, the single call's formulation:
  the tie    the table holds exact counts, so the M-th occurrence of a pair that counts M is its LAST one: every position whose pair
             counts M raises last[slot] to itself, and the winner is the pair whose last occurrence is smallest.  No selection, no sort.
  the table  cannot grow.  A recount of m symbols claims fewer than m <= cap / 2 slots; a round inserts at most `fresh` new keys, and a
             round with claimed + fresh > cap / 2 does not apply its deltas: the table is cleared and recounted from the compacted
             sequence.  The rebuild also halves the capacity while `spb` slots per live symbol still fit.  spb = 4, or 2 with option
             repair_batch_table = 1.  assert_invariants() is what the kernel's comment promises: never more than half of the slots
             claimed when a pass inserts, `last` all 0 between rounds.
  slices     run_slice() performs at most `rounds` rounds and leaves the state; batch_grammars() relaunches while a text is unfinished.
  chunks     the square mark and the compaction walk the sequence in chunks of CHUNK positions, ITEMS per thread, with a carry.
tests/test_repair_batch_model.py holds all of it against grammar().
"""
from tests.models.repair import SIGMA

ITEMS, THREADS = 8, 256
CHUNK = ITEMS * THREADS
MIN_CAP = 8
TEXT_MAX = 1 << 24
EMPTY = None
MASK64 = (1 << 64) - 1


class Full(Exception):
    """a probe run passed over every slot: the kernel gives the text TDC_GPU_ERR_INTERNAL"""


def table_slots(n, spb):
    """the slots of a text of n bytes: the power of two from spb * n on (none without a pair)"""
    if n < 2 or n > TEXT_MAX:
        return 0
    cap = MIN_CAP
    while cap < spb * n:
        cap <<= 1
    return cap


def launch_rounds(n, rounds):
    """the rounds of one launch for a text of n bytes: `rounds` up to 128 KiB, divided by n / 64 KiB beyond"""
    by = n >> 16
    return max(1, rounds // by if by > 1 else rounds)


class Text:
    def __init__(self, data, spb):
        self.n = len(data)
        self.S = list(bytes(data))
        self.rules = []
        self.spb = spb
        self.cap = table_slots(self.n, spb)
        self.occupied = 0
        self.done = self.n < 2
        self.tie_rounds = self.rebuilds = self.fills = self.rounds = 0      # fills: the rebuilds a table that could fill asked for
        self.peak = 0.0                                   # the largest share of claimed slots a pass ever inserted into
        if not self.done:
            self._rebuild()

    # ---- the table ---------------------------------------------------------------------------------------------------------------
    def _slot0(self, key):
        k = key[0] << 32 | key[1]
        return ((k * 0x9E3779B97F4A7C15) & MASK64) >> (64 - self.cap.bit_length() + 1)

    def _find(self, key):
        h = self._slot0(key)
        for _ in range(self.cap):
            if self.keys[h] == key:
                return h
            if self.keys[h] is EMPTY:
                return None
            h = (h + 1) & (self.cap - 1)
        return None

    def _add(self, key, d):
        h = self._slot0(key)
        for _ in range(self.cap):
            if self.keys[h] is EMPTY:
                self.keys[h] = key
                self.occupied += 1
            if self.keys[h] == key:
                self.counts[h] += d
                return
            h = (h + 1) & (self.cap - 1)
        raise Full()

    def _sub(self, key, win):
        if key == win:
            return
        h = self._find(key)
        assert h is not None and self.counts[h] > 0
        self.counts[h] -= 1

    def _rebuild(self):
        self.keys, self.counts, self.last = [EMPTY] * self.cap, [0] * self.cap, [0] * self.cap
        self.occupied = 0
        for i in range(len(self.S) - 1):
            self._add((self.S[i], self.S[i + 1]), 1)
        assert 2 * self.occupied <= self.cap              # fewer than m distinct pairs, cap >= 2 m

    def assert_invariants(self):
        assert not any(self.last)
        assert self.cap >= self.spb * max(len(self.S), 2) or self.cap == MIN_CAP
        live = {}
        for i in range(len(self.S) - 1):
            k = (self.S[i], self.S[i + 1])
            live[k] = live.get(k, 0) + 1
        held = {k: c for k, c in zip(self.keys, self.counts) if k is not EMPTY and c}
        assert held == live                               # exact overlapping counts; entries of count 0 stay
        assert self.occupied == sum(1 for k in self.keys if k is not EMPTY)

    # ---- one round ---------------------------------------------------------------------------------------------------------------
    def _mark_square(self, a):
        """run starts by an inclusive max over start markers: per chunk, a thread's ITEMS positions, the max over the threads in front
        of it, the carry of the chunks in front"""
        S, m = self.S, len(self.S)
        taken = [False] * m
        carry = 0
        for c0 in range(0, m, CHUNK):
            runs, marks = [], []
            for t in range(THREADS):
                run, mk = 0, []
                for q in range(ITEMS):
                    i = c0 + t * ITEMS + q
                    inside = 0 < i < m and S[i] == a and S[i - 1] == a
                    run = max(run, 0 if inside or i >= m else i)
                    mk.append(run)
                runs.append(run)
                marks.append(mk)
            pre = 0
            for t in range(THREADS):
                ex = max(carry, pre)                      # exclusive: the threads in front, and the carry
                for q in range(ITEMS):
                    i = c0 + t * ITEMS + q
                    if i < m:
                        rs = max(ex, marks[t][q])
                        taken[i] = i + 1 < m and S[i] == a and S[i + 1] == a and (i - rs) % 2 == 0
                pre = max(pre, runs[t])
            carry = max(carry, pre)
        return taken

    def _compact(self, taken, A):
        """in place: a chunk is read whole, then written at or in front of where it was read"""
        S, m = self.S, len(self.S)
        out = 0
        for c0 in range(0, m, CHUNK):
            chunk = [(A if taken[i] else S[i]) for i in range(c0, min(c0 + CHUNK, m)) if not (i > 0 and taken[i - 1])]
            assert out + len(chunk) <= min(c0 + CHUNK, m)
            S[out:out + len(chunk)] = chunk
            out += len(chunk)
        del S[out:]

    def round(self, max_rules):
        """False: the text is finished"""
        S = self.S
        m = len(S)
        limit = min(max_rules, self.n) if max_rules else self.n
        if m < 2 or len(self.rules) >= limit:
            return False
        M = max(self.counts)
        if M <= 1:
            return False
        tied = [h for h in range(self.cap) if self.counts[h] == M]
        if len(tied) > 1:
            self.tie_rounds += 1
            for i in range(m - 1):
                h = self._find((S[i], S[i + 1]))
                if self.counts[h] == M:
                    self.last[h] = max(self.last[h], i)
            p = min(self.last[h] for h in tied)
            for h in tied:
                self.last[h] = 0
            assert 1 <= p <= m - 2                        # a last occurrence: M >= 2 of them, and a partner follows
            win = (S[p], S[p + 1])
        else:
            win = self.keys[tied[0]]
        l, r = win
        A = SIGMA + len(self.rules)
        taken = [i + 1 < m and S[i] == l and S[i + 1] == r for i in range(m)] if l != r else self._mark_square(l)
        ntaken = sum(taken)
        assert ntaken >= 1 and (l == r or ntaken == M)    # every round removes at least one symbol
        m_new = m - ntaken
        fresh = min(2 * ntaken, 2 * A + 1)
        cap_new = self.cap
        while cap_new > MIN_CAP and cap_new >> 1 >= self.spb * m_new:
            cap_new >>= 1
        full = self.occupied + fresh > self.cap // 2
        rebuild = full or cap_new != self.cap
        if not rebuild:
            before = self.occupied
            self.counts[self._find(win)] = 0
            for i in range(m - 1):
                if not taken[i]:
                    continue
                if i > 0:
                    x = S[i - 1]
                    self._sub((x, S[i]), win)
                    self._add((A if i >= 2 and taken[i - 2] else x, A), 1)
                if i + 2 < m and not taken[i + 2]:
                    y = S[i + 2]
                    self._sub((S[i + 1], y), win)
                    self._add((A, y), 1)
            assert self.occupied - before <= fresh and 2 * self.occupied <= self.cap
            self.peak = max(self.peak, self.occupied / self.cap)
        self._compact(taken, A)
        assert len(S) == m_new
        self.rules.append(win)
        self.rounds += 1
        if rebuild:
            self.cap = cap_new
            self._rebuild()
            self.rebuilds += 1
            self.fills += full
        return True

    def run_slice(self, rounds, max_rules, check=False):
        """at most `rounds` rounds; the state stays"""
        for _ in range(launch_rounds(self.n, rounds)):
            if self.done:
                return
            if not self.round(max_rules):
                self.done = True
                return
            if check:
                self.assert_invariants()
        limit = min(max_rules, self.n) if max_rules else self.n
        if len(self.S) < 2 or len(self.rules) >= limit:
            self.done = True


class BatchStats:
    def __init__(self):
        self.launches = self.tie_rounds = self.rebuilds = self.fills = self.rules = self.replaced = 0
        self.peak = 0.0


def batch_grammars(texts, max_rules=0, rounds=256, table=0, stats=None, check=False):
    """[(rules, start)] of the texts, None for a text beyond the cap: launches of at most `rounds` rounds per text, longest text first,
    until no text is unfinished"""
    st = stats if stats is not None else BatchStats()
    spb = 2 if table else 4
    states = [Text(x, spb) if len(x) <= TEXT_MAX else None for x in texts]
    order = sorted((k for k, s in enumerate(states) if s is not None), key=lambda k: -len(texts[k]))
    while order:
        st.launches += 1
        unfinished = False
        for k in order:
            s = states[k]
            if not s.done:
                s.run_slice(rounds, max_rules, check)
                unfinished |= not s.done
        n_max = max(len(texts[k]) for k in order)
        assert st.launches <= n_max // launch_rounds(n_max, rounds) + 2
        if not unfinished:
            break
    for s in states:
        if s is not None:
            st.tie_rounds += s.tie_rounds
            st.rebuilds += s.rebuilds
            st.fills += s.fills
            st.rules += len(s.rules)
            st.replaced += s.n - len(s.S)
            st.peak = max(st.peak, s.peak)
    return [None if s is None else (list(s.rules), list(s.S)) for s in states]
