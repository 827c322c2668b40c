"""Sequential model of repair = RePairCompressor<coder> (compressors/RePairCompressor.hpp:96-336).

grammar() restates the reference's two loops per round literally; device_grammar() is the formulation repair.hip runs (DESIGN.md section
5.8) written as its passes -- digram table, argmax, tie pass, mark, deltas, compaction -- and tests/test_repair_model.py holds the two
against each other.  encode() writes a grammar through the field writers of tests/models/lzss_coders.py (bit, gamma, delta, ascii),
sequential_decode() is the reference's decode loop with the refusals of tdc_repair_decode.

Symbols: 0 .. 255 are terminals, 256 + k is rule k.  A grammar is (rules, start): rules[k] = (l, r), start = the sequence that is left.
The empty input, on which the reference is undefined (n - 1 wraps, :133), is DEFINED as no rules and no symbols.
"""
from tests.models.lz78_decode import BitWriter as _FieldBits      # the bit order of io/BitOStream.hpp, for encode_fields()
from tests.models.lzss_coders import Malformed, Reader, Sink, WRITERS, bits_for, terminate

CODERS = ("bit", "gamma", "delta", "ascii")
SIGMA = 256
TEXT_MAX = 0xFFFFFFFE
MASK64 = (1 << 64) - 1
LEN_MAX = 0xFFFFFFFF                                              # len_r = TypeRange<len_t>


class TooLarge(Exception):
    pass


# ---- :96-178 -------------------------------------------------------------------------------------------------------------------------
def grammar(data, max_rules=0):
    text = list(bytes(data))
    n = len(text)
    if n == 0:
        return [], []
    nxt = list(range(1, n + 1))
    limit = max_rules if max_rules else 1 << 62
    rules = []
    while True:
        count = {}
        best, best_count = None, 0
        i = 0
        while i < n - 1:                                          # :133
            j = nxt[i]
            if j >= n:
                break
            di = (text[i], text[j])
            c = count.get(di, 0) + 1
            count[di] = c
            if c > best_count:                                    # :144 strictly: the pair that reaches the largest count first
                best, best_count = di, c
            i = j
        if best_count <= 1:                                       # :155
            break
        new_sym = SIGMA + len(rules)
        rules.append(best)
        i = 0
        while i < n - 1:                                          # :160
            j = nxt[i]
            if j >= n:
                break
            if (text[i], text[j]) == best:
                text[i] = new_sym
                nxt[i] = nxt[j]
            i = nxt[i]                                            # :173 behind the pair
        if len(rules) >= limit:                                   # :178
            break
    start = []
    i = 0
    while i < n:
        start.append(text[i])
        i = nxt[i]
    return rules, start


# ---- the device formulation (repair.hip) ---------------------------------------------------------------------------------------------
class DeviceStats:
    def __init__(self):
        self.rounds = self.tie_rounds = self.replaced = self.rebuilds = 0


def _recount(S):
    table = {}
    for i in range(len(S) - 1):
        k = (S[i], S[i + 1])
        table[k] = table.get(k, 0) + 1
    return table


def device_grammar(data, max_rules=0, recount=False, stats=None):
    """Pass by pass, as the kernels of repair.hip do it.  The table holds the exact overlapping count of every pair of the live sequence
    (entries of count 0 stay, as on the device); recount=True rebuilds it from S in every round instead of applying the deltas."""
    st = stats if stats is not None else DeviceStats()
    S = list(bytes(data))
    rules = []
    limit = max_rules if max_rules else 1 << 62
    table = _recount(S)
    while len(rules) < limit:
        m = len(S)
        # argmax: M, the number T of entries that hold it
        M = max(table.values(), default=0)
        if M <= 1:
            break
        tied = [k for k, c in table.items() if c == M]
        st.rounds += 1
        if len(tied) > 1:
            # tie pass: positions whose pair counts M, in position order; stable sort by key; every group has M members, the last one is
            # the pair's M-th occurrence; the group whose last position is smallest wins
            st.tie_rounds += 1
            pos = [i for i in range(m - 1) if table[(S[i], S[i + 1])] == M]
            assert len(pos) == len(tied) * M
            pos.sort(key=lambda i: (S[i], S[i + 1]))              # (stable)
            last = [pos[g * M + M - 1] for g in range(len(tied))]
            p = min(last)
            win = (S[p], S[p + 1])
        else:
            win = tied[0]
        l, r = win
        A = SIGMA + len(rules)
        rules.append(win)
        # mark
        taken = [False] * m
        if l != r:
            for i in range(m - 1):
                taken[i] = S[i] == l and S[i + 1] == r
        else:
            marker = [0 if (S[i] == l and i > 0 and S[i - 1] == l) else i for i in range(m)]
            run_start, run = [0] * m, 0
            for i in range(m):                                    # inclusive max
                run = max(run, marker[i])
                run_start[i] = run
            for i in range(m - 1):
                taken[i] = S[i] == l and S[i + 1] == l and (i - run_start[i]) % 2 == 0
        # deltas: a taken occurrence owns its left boundary, and its right one unless the pair behind it is taken too
        if not recount:
            def add(k, d):
                if k == win:
                    return                                        # deltas that name the winner are dropped: its entry is cleared
                table[k] = table.get(k, 0) + d
            for i in range(m - 1):
                if not taken[i]:
                    continue
                if i > 0:
                    if i >= 2 and taken[i - 2]:
                        add((S[i - 1], S[i]), -1)
                        add((A, A), +1)
                    else:
                        add((S[i - 1], S[i]), -1)
                        add((S[i - 1], A), +1)
                if i + 2 < m and not (i + 2 < m - 1 and taken[i + 2]):
                    add((S[i + 1], S[i + 2]), -1)
                    add((A, S[i + 2]), +1)
            table[win] = 0
            assert all(c >= 0 for c in table.values())
        # compact
        out = []
        for i in range(m):
            if i > 0 and taken[i - 1]:
                continue
            out.append(A if taken[i] else S[i])
        st.replaced += m - len(out)
        S = out
        if recount:
            table = _recount(S)
    return rules, S


# ---- :208-263 ------------------------------------------------------------------------------------------------------------------------
def _walk(rules, start, w):
    w.integer(len(rules), 0, LEN_MAX)                             # len_r

    def sym(x, hi):
        if x < SIGMA:
            w.flag(False)
            w.literal(x)
        else:
            w.flag(True)
            w.integer(x - SIGMA, 0, hi)
    for i, (l, r) in enumerate(rules):
        sym(l, i)                                                 # Range(i)
        sym(r, i)
    for x in start:
        sym(x, len(rules))                                        # Range(rules)


def encode_bits(rules, start, coder):
    s = Sink()
    _walk(rules, start, WRITERS[coder](s))
    return s.bits()


def encode(rules, start, coder):
    return terminate(encode_bits(rules, start, coder))


def encode_fields(rules, start):
    """coder=bit once more, through the BitWriter of tests/models/lz78_decode.py: the stream bytes"""
    bw = _FieldBits()
    bw.write(len(rules), 32)

    def sym(x, hi):
        if x < SIGMA:
            bw.write(x, 9)
        else:
            bw.write(1, 1)
            bw.write(x - SIGMA, bits_for(hi))
    for i, (l, r) in enumerate(rules):
        sym(l, i)
        sym(r, i)
    for x in start:
        sym(x, len(rules))
    return bw.finish()


def compress(data, coder="bit", max_rules=0):
    return encode(*grammar(data, max_rules), coder)


# ---- :287-336 ------------------------------------------------------------------------------------------------------------------------
class _Reader(Reader):
    def __init__(self, stream):
        Reader.__init__(self, stream)
        self.over = False

    def int(self, nb):
        if self.pos + nb > self.total:
            self.over = True
        return Reader.int(self, nb)


def parse(stream, coder):
    """the grammar a stream holds: (rules, start); Malformed where tdc_repair_decode returns TDC_GPU_ERR_ARG"""
    r = _Reader(bytes(stream))
    if coder == "bit":
        flag, literal = r.bit, lambda: r.int(8)

        def integer(hi):
            return r.int(bits_for(hi))
    elif coder == "ascii":
        def flag():
            return r.int(8) != ord("0")

        def literal():
            return r.int(8)

        def integer(hi):
            v, digits = 0, 0
            c = r.int(8)
            while ord("0") <= c <= ord("9"):
                v, digits = (v * 10 + c - ord("0")) & MASK64, digits + 1
                if r.eof():
                    break
                c = r.int(8)
            if not digits:
                raise Malformed("integer expected")
            return v
    else:
        code = r.gamma if coder == "gamma" else r.delta
        flag, literal = r.bit, lambda: code() & 0xFF

        def integer(hi):
            return code()

    def sym(hi, limit):
        if flag():
            v = integer(hi)
            if r.over:
                raise Malformed("cut-off field")
            if v >= limit:
                raise Malformed("rule index out of range")
            return SIGMA + v
        c = literal()
        if r.over:
            raise Malformed("cut-off field")
        return c
    nrules = integer(LEN_MAX)
    if r.over:
        raise Malformed("cut-off field")
    if nrules > 2 * len(stream):                                  # a rule takes two symbols of at least two bits each
        raise Malformed("more rules than the stream can hold")
    rules = []
    for i in range(nrules):
        l = sym(i, i)
        rr = sym(i, i)
        rules.append((l, rr))
    start = []
    while not r.eof():
        start.append(sym(nrules, nrules))
    return rules, start


def expansion_lengths(rules):
    """length of every rule's expansion, saturating at 2^64 - 1"""
    ln = []
    for l, r in rules:
        a = 1 if l < SIGMA else ln[l - SIGMA]
        b = 1 if r < SIGMA else ln[r - SIGMA]
        ln.append(min(a + b, MASK64))
    return ln


def sequential_decode(stream, coder):
    rules, start = parse(stream, coder)
    ln = expansion_lengths(rules)
    total = 0
    for x in start:
        total = min(total + (1 if x < SIGMA else ln[x - SIGMA]), MASK64)
    if total > TEXT_MAX:
        raise TooLarge()
    out = bytearray()
    for x in start:                                               # :274-284 with an explicit stack
        stack = [x]
        while stack:
            y = stack.pop()
            if y < SIGMA:
                out.append(y)
            else:
                l, r = rules[y - SIGMA]
                stack.append(r)
                stack.append(l)
    return bytes(out)
