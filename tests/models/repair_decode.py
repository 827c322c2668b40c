"""The device decoder of repair (repair_decode.hip, DESIGN.md section 5.8 "Device decoder"), pass by pass, built on tests/models/repair.py.

parse_device() is the parse: the host reads the count field (and, under bit, the rules below HOST_RULES), then segments of at most seg_bits
bit positions -- the tokens that start in a segment, found by walking next() from its first bit --, each read with ONE index width under
bit and cut after the tokens its stretch of equal width still holds.  lengths() and first_occurrences() are the two round loops in their
slowest schedule (every round reads the values of the round before: the device, which also sees values of the running round, never needs
more rounds), items() makes the literals and the factor list, resolve() copies the references.  decode() strings them together and hands
the stream to repair.sequential_decode where the device does: a gamma / delta field beyond its caps, or more rounds than the cap.

A token is (class, end, is_rule, value); the classes are those of the kernels: OK, BAD (the host loop refuses it too), WIDE (beyond a cap).
"""
from tests.models import repair as R
from tests.models.lzss_coders import Malformed, bits_for, payload_bits

HOST_RULES = 4096
ROUNDS = 1024                                                     # option repair_dec_rounds
NONE = 0xFFFFFFFF
LEN_SAT = 0xFFFFFFFF
OK, BAD, WIDE = 0, 1, 2


class ToHost(Exception):
    """the host loop has the verdict on this stream"""


class Bits:
    def __init__(self, stream):
        stream = bytes(stream)
        self.total = payload_bits(stream)
        self.s = format(int.from_bytes(stream, "big"), "0%db" % (8 * len(stream)))[:self.total] if stream else ""

    def peek(self, x, nb=64):
        """nb bits from x on, zeros behind the end"""
        return int(self.s[x:x + nb].ljust(nb, "0"), 2) if nb else 0


def _field(b, y, coder, cap):
    """one gamma / delta field: (class, bits used, value); cap = most value bits"""
    w = b.peek(y)
    if not w:
        return (BAD if y + 64 > b.total else WIDE), 0, 0
    z = 64 - w.bit_length()                                       # leading zeros
    used = z + 1
    if coder == "delta":
        if z > 6:
            return WIDE, 0, 0
        width = b.peek(y + used, z)
        used += z
        z = width
    if z > cap:
        return WIDE, 0, 0
    return OK, used + z, b.peek(y + used, z)


def token(b, x, coder, w):
    """the token that starts at bit x, an index read in w bits under bit"""
    if x >= b.total:
        return BAD, x, 0, 0
    rule = b.peek(x, 1)
    y = x + 1
    if coder == "bit":
        nb = w if rule else 8
        val = b.peek(y, nb)
        y += nb
    else:
        cls, used, val = _field(b, y, coder, 32 if rule else 8)
        if cls != OK:
            return cls, x, rule, 0
        y += used
    if y > b.total:
        return BAD, x, rule, 0
    return OK, y, rule, val


def _host_code(b, coder, pos):
    """one gamma / delta code of at most 32 value bits as the host part reads it: (value, end); ToHost where it does not"""
    def gamma(cap, pos):
        z = 0
        while True:
            if pos >= b.total or z > cap:
                raise ToHost("count field")
            pos += 1
            if b.peek(pos - 1, 1):
                break
            z += 1
        if pos + z > b.total:
            raise ToHost("count field")
        return b.peek(pos, z), pos + z
    if coder == "gamma":
        return gamma(32, pos)
    width, pos = gamma(6, pos)
    if width > 32 or pos + width > b.total:
        raise ToHost("count field")
    return b.peek(pos, width), pos + width


def stretch(t, nrules):
    """token ordinal t under bit: (index width, tokens its stretch still holds; None: the start sequence)"""
    if t >= 2 * nrules:
        return bits_for(nrules), None
    i = t >> 1
    w = bits_for(i)
    stop = min(2 if i < 2 else 1 << w, nrules)
    return w, 2 * stop - t


def parse_device(stream, coder, seg_bits=1 << 30, host_rules=HOST_RULES, log=None):
    """(rules, start) as the device parses them.  log (a list) receives one (x_in, t_in, width, tokens kept) per segment."""
    b = Bits(stream)
    if coder == "bit":
        if b.total < 32:
            raise Malformed("cut-off field")
        nrules, x = b.peek(0, 32), 32
    else:
        nrules, x = _host_code(b, coder, 0)
    if nrules > 2 * len(stream):
        raise Malformed("more rules than the stream can hold")
    sym = []
    if coder == "bit":                                            # the host's part of the rules
        for t in range(2 * min(nrules, host_rules)):
            cls, end, rule, val = token(b, x, coder, bits_for(t >> 1))
            if cls != OK:
                raise Malformed("cut-off field")
            if rule and val >= t >> 1:
                raise Malformed("rule index out of range")
            sym.append(R.SIGMA + val if rule else val)
            x = end
    rate = 0.0
    while x < b.total:
        m = min(seg_bits, b.total - x)
        w, left = 0, None
        if coder == "bit":
            w, left = stretch(len(sym), nrules)
            if left is not None:
                if rate == 0:
                    rate = 1.0 + max(8, w)
                m = min(m, int(left * rate * (1.0 + 1.0 / 64) + 4096.0))
        toks, y = [], x                                           # the orbit of the segment's first bit under next()
        while y < x + m:
            tk = token(b, y, coder, w)
            toks.append(tk)
            if tk[0] != OK:
                break
            y = tk[1]
        keep = len(toks) if left is None else min(len(toks), left)
        t0 = len(sym)
        for j, (cls, end, rule, val) in enumerate(toks[:keep]):
            t = t0 + j
            limit = t >> 1 if t < 2 * nrules else nrules
            if cls == WIDE:
                raise ToHost("field beyond a device cap")
            if cls == BAD or (rule and val >= limit):
                raise Malformed("malformed or cut-off token, or a rule index out of range")
            sym.append(R.SIGMA + val if rule else val)
        if log is not None:
            log.append((x, t0, w, keep))
        rate = (toks[keep - 1][1] - x) / keep
        x = toks[keep - 1][1]
    if len(sym) < 2 * nrules:
        raise Malformed("cut-off field")
    return [(sym[2 * k], sym[2 * k + 1]) for k in range(nrules)], sym[2 * nrules:]


def lengths(rules, cap=ROUNDS):
    """(len[], rounds): 0 = not known yet, 32-bit saturating; ToHost after cap rounds without a quiet one"""
    ln = [0] * len(rules)
    if not rules:
        return ln, 0
    for rounds in range(1, cap + 1):
        prev = list(ln)
        changed = False
        for k, (l, r) in enumerate(rules):
            if prev[k]:
                continue
            a = 1 if l < R.SIGMA else prev[l - R.SIGMA]
            c = 1 if r < R.SIGMA else prev[r - R.SIGMA]
            if a and c:
                ln[k] = min(a + c, LEN_SAT)
                changed = True
        if not changed:
            return ln, rounds
    raise ToHost("length rounds")


def positions(start, ln):
    """exclusive scan of the start symbols' lengths: (pos[], n)"""
    pos, n = [], 0
    for x in start:
        pos.append(n)
        n += 1 if x < R.SIGMA else ln[x - R.SIGMA]
    return pos, n


def first_occurrences(rules, start, ln, pos, cap=ROUNDS):
    """(first[], rounds): the leftmost text position at which every rule is expanded, NONE for a rule that never is"""
    first = [NONE] * len(rules)
    if not rules:
        return first, 0
    for x, q in zip(start, pos):
        if x >= R.SIGMA:
            first[x - R.SIGMA] = min(first[x - R.SIGMA], q)
    for rounds in range(1, cap + 1):
        prev = list(first)
        changed = False
        for k, (l, r) in enumerate(rules):
            f = prev[k]
            if f == NONE:
                continue
            if l >= R.SIGMA and f < first[l - R.SIGMA]:
                first[l - R.SIGMA] = f
                changed = True
            if r >= R.SIGMA:
                q = f + (1 if l < R.SIGMA else ln[l - R.SIGMA])
                if q < first[r - R.SIGMA]:
                    first[r - R.SIGMA] = q
                    changed = True
        if not changed:
            return first, rounds
    raise ToHost("first-occurrence rounds")


def items(rules, start, ln, pos, first):
    """(literals [(q, byte)], factors [(q, src, len)]) of the m + 2 * rules items"""
    its = list(zip(start, pos))
    for k, (l, r) in enumerate(rules):
        if first[k] != NONE:
            its.append((l, first[k]))
            its.append((r, first[k] + (1 if l < R.SIGMA else ln[l - R.SIGMA])))
    lits, facs = [], []
    for c, q in its:
        if c < R.SIGMA:
            lits.append((q, c))
        elif first[c - R.SIGMA] != q:
            assert first[c - R.SIGMA] + ln[c - R.SIGMA] <= q       # two occurrences of one rule never overlap
            facs.append((q, first[c - R.SIGMA], ln[c - R.SIGMA]))
    return lits, facs


def resolve(n, lits, facs):
    text = [None] * n
    ref = [None] * n
    for q, c in lits:
        assert text[q] is None and ref[q] is None
        text[q] = c
    for q, src, length in facs:
        for j in range(length):
            assert text[q + j] is None and ref[q + j] is None     # every position is written once
            ref[q + j] = src + j
    for p in range(n):                                            # (every source lies in front of its target)
        if ref[p] is not None:
            text[p] = text[ref[p]]
    assert None not in text
    return bytes(text)


def decode(stream, coder, seg_bits=1 << 30, cap=ROUNDS, host_rules=HOST_RULES, stats=None):
    """the text, through the device passes or -- ToHost -- the host loop; Malformed / repair.TooLarge as repair.sequential_decode"""
    st = stats if stats is not None else {}
    st.update(device=0, segments=0, len_rounds=0, first_rounds=0, factors=0)
    try:
        log = []
        rules, start = parse_device(stream, coder, seg_bits, host_rules, log)
        ln, st["len_rounds"] = lengths(rules, cap)
        pos, n = positions(start, ln)
        if n > R.TEXT_MAX:
            raise R.TooLarge()
        first, st["first_rounds"] = first_occurrences(rules, start, ln, pos, cap)
        lits, facs = items(rules, start, ln, pos, first)
        st.update(device=1, segments=len(log), factors=len(facs), rules=len(rules))
        return resolve(n, lits, facs)
    except ToHost:
        st.update(device=0, segments=0, len_rounds=0, first_rounds=0, factors=0)
        return R.sequential_decode(stream, coder)
