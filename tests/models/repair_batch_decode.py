"""The batch decoder of repair streams (repair_batch_decode.hip, DESIGN.md section 5.8 "Batch decoder"), pass by pass, built on
tests/models/repair.py and tests/models/repair_decode.py.

walk() is what one wave does with one stream: the count field, 2 R tokens, start symbols until the stream ends, every index checked
against its OWN stream, every token read by repair_decode.token with the device caps -- a token beyond a cap (WIDE) is refused like a
cut-off one, because the batch has no host loop to hand the stream to.  decode_batch() strings the passes together over the forest: the
symbols rebased, the lengths in the strict schedule with the cap on the height, `nothing` in place of a refused stream's start symbols,
the sizes and the refusals, first occurrences from the global positions, and the items over the concatenated text, where
repair_decode.resolve asserts that every position is written exactly once.

expected() is the verdict of the specification on one stream alone -- repair.sequential_decode -- with the two deviations the header
states: the caps (computed here from the stream: the first token the walk does not read is WIDE and the host loop does not refuse the
stream) and the height.
"""
from tests.models import repair as R
from tests.models import repair_decode as RD
from tests.models.lzss_coders import Malformed, bits_for

OK, ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = 0, -2, -4, -5, -6
CODERS = ("bit", "gamma", "delta")
ROUNDS = RD.ROUNDS                                                # option repair_dec_rounds
TEXT_MAX = R.TEXT_MAX
TOKEN_LIMIT = 0xFFFFFFFE - 256                                    # 2^32 - 258 tokens and more: 256 + a global rule index leaves 32 bits
NONE = RD.NONE
LEN_SAT = RD.LEN_SAT


def walk(stream, coder):
    """(verdict, rules, start, wide): wide = the token that ended the walk crosses a device cap.  A refused stream has no tokens."""
    stream = bytes(stream)
    bad = (ERR_ARG, [], [], False)
    if not stream or (len(stream) == 1 and stream[0] & 7 >= 6):   # the stream of no bytes; the cut-off terminator
        return bad
    b = RD.Bits(stream)
    if coder == "bit":
        if b.total < 32:
            return bad
        nrules, x = b.peek(0, 32), 32
    else:
        cls, used, nrules = RD._field(b, 0, coder, 32)            # the count is read with the cap of an index
        if cls != RD.OK or used > b.total:
            return (ERR_ARG, [], [], cls == RD.WIDE)
        x = used
    if nrules > 2 * len(stream):
        return bad
    sym, t = [], 0
    while t < 2 * nrules or x < b.total:                          # every turn takes at least one bit, or ends the walk
        limit = t >> 1 if t < 2 * nrules else nrules              # own-stream limits: a rule in front of this one / below R_k
        cls, end, rule, val = RD.token(b, x, coder, bits_for(limit))
        if cls != RD.OK:
            return (ERR_ARG, [], [], cls == RD.WIDE)
        if rule and val >= limit:
            return bad
        sym.append(R.SIGMA + val if rule else val)
        x, t = end, t + 1
    return OK, [(sym[2 * k], sym[2 * k + 1]) for k in range(nrules)], sym[2 * nrules:], False


def heights(rules):
    """a byte has height 0, a rule 1 + the larger height of its sides"""
    h = []
    for l, r in rules:
        h.append(1 + max(0 if l < R.SIGMA else h[l - R.SIGMA], 0 if r < R.SIGMA else h[r - R.SIGMA]))
    return h


def strict_lengths(rules, cap):
    """(len[], rounds): at most cap rounds, each from the values of the round before; 0 = still unknown, i.e. higher than cap"""
    ln = [0] * len(rules)
    rounds = 0
    while rules and rounds < cap:
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
        rounds += 1
        if not changed:
            break
    return ln, rounds


def call_limits(tokens, total):
    """the call-level refusals from the two 64-bit totals the host reads back: tokens first (before the grammar is allocated), then text"""
    if tokens >= TOKEN_LIMIT:
        return ERR_TOO_LARGE
    if total > TEXT_MAX:
        return ERR_TOO_LARGE
    return OK


def decode_batch(streams, coder, cap=ROUNDS, out_cap=None, stats=None):
    """(rc, texts, statuses, out_off).  rc: OK, ERR_TOO_LARGE (the call-level limits) or ERR_OOM (out_cap given and too small); texts is
    None unless rc is OK.  Raises what the argument check refuses as ValueError."""
    if coder not in CODERS:
        raise ValueError("coder")
    st = stats if stats is not None else {}
    count = len(streams)
    walks = [walk(s, coder) for s in streams]
    status = [w[0] for w in walks]
    # ---- scans, the symbols rebased: one forest
    rule_off, start_off = [0], [0]
    for v, rules, start, _ in walks:
        rule_off.append(rule_off[-1] + len(rules))
        start_off.append(start_off[-1] + len(start))
    nr, m = rule_off[-1], start_off[-1]
    if call_limits(2 * nr + m, 0):
        return ERR_TOO_LARGE, None, status, None
    nothing = R.SIGMA + nr                                        # the rule behind the last one: length 0, no sides
    rules, start, owner = [], [], []
    for k, (v, rk, sk, _) in enumerate(walks):
        def reb(x, ro=rule_off[k]):
            return x + ro if x >= R.SIGMA else x
        rules += [(reb(l), reb(r)) for l, r in rk]
        start += [reb(x) for x in sk]
        owner += [k] * len(sk)
        for i, (l, r) in enumerate(rk):                           # nothing in front of a stream's own rules is reachable
            assert all(x < R.SIGMA or rule_off[k] <= reb(x) - R.SIGMA < rule_off[k] + i for x in (l, r))
    # ---- lengths in the strict schedule; a stream that owns a rule still unknown is higher than cap
    ln, st["len_rounds"] = strict_lengths(rules, cap)
    hs = heights(rules)
    assert all((ln[i] == 0) == (hs[i] > cap) for i in range(nr))
    for k in range(count):
        if any(ln[i] == 0 for i in range(rule_off[k], rule_off[k + 1])):
            status[k] = ERR_UNSUPPORTED
    ln.append(0)                                                  # len[R]: nothing
    # ---- nothing for the refused, advances, one scan, the sizes
    start = [nothing if status[owner[j]] else x for j, x in enumerate(start)]
    S, acc = [], 0
    for x in start:
        S.append(acc)
        acc += 1 if x < R.SIGMA else ln[x - R.SIGMA]
    S.append(acc)
    tlen = []
    for k in range(count):
        tl = S[start_off[k + 1]] - S[start_off[k]]
        if status[k]:
            tl = 0
        elif tl > TEXT_MAX:
            status[k], tl = ERR_TOO_LARGE, 0
        tlen.append(tl)
    out_off = [0]
    for tl in tlen:
        out_off.append(out_off[-1] + tl)
    n = out_off[-1]
    st["rules"] = sum(rule_off[k + 1] - rule_off[k] for k in range(count) if not status[k])
    # the start symbols move to their text's slot; those of the refused (now all of them known) become nothing at position 0
    pos = []
    for j in range(m):
        k = owner[j]
        if status[k]:
            start[j] = nothing
            pos.append(0)
        else:
            pos.append(S[j] - S[start_off[k]] + out_off[k])
    if call_limits(2 * nr + m, n):
        return ERR_TOO_LARGE, None, status, out_off
    if out_cap is not None and n > out_cap:
        return ERR_OOM, None, status, out_off
    # ---- first occurrences from the global positions: seeded by the accepted streams alone (nothing seeds the rule nothing, which has no sides)
    first = [NONE] * (nr + 1)
    for x, q in zip(start, pos):
        if x >= R.SIGMA:
            first[x - R.SIGMA] = min(first[x - R.SIGMA], q)
    rounds = 0
    while nr and n:
        prev = list(first)
        changed = False
        for k, (l, r) in enumerate(rules):
            f = prev[k]
            if f == NONE:
                continue
            for x, q in ((l, f), (r, f + (1 if l < R.SIGMA else ln[l - R.SIGMA]))):
                if x >= R.SIGMA and q < first[x - R.SIGMA]:
                    first[x - R.SIGMA] = q
                    changed = True
        rounds += 1
        if not changed:
            break
        assert rounds <= cap + 1, "the first occurrences of grammars no higher than cap rest within cap + 1 rounds"
    st["first_rounds"] = rounds
    for k in range(count):                                        # the rules of a refused stream are never seeded
        if status[k]:
            assert all(first[i] == NONE for i in range(rule_off[k], rule_off[k + 1]))
    # ---- the items over the concatenated text
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
            assert c != nothing
            facs.append((q, first[c - R.SIGMA], ln[c - R.SIGMA]))
    st["factors"] = len(facs)
    text = RD.resolve(n, lits, facs)                              # (asserts: every position of the concatenated text is written once)
    return OK, [text[out_off[k]:out_off[k + 1]] for k in range(count)], status, out_off


def host(stream, coder):
    """(status, text) of the specification, repair.sequential_decode (tdc_repair_decode), on one stream"""
    try:
        return OK, R.sequential_decode(bytes(stream), coder)
    except Malformed:
        return ERR_ARG, b""
    except R.TooLarge:
        return ERR_TOO_LARGE, b""


def expected(stream, coder, cap=ROUNDS, decode=True):
    """(status, text, excepted) for one stream alone: the host's verdict but for the two deviations.  excepted: the caps made the
    difference.  decode=False leaves the text of an accepted stream out (None): for claims nobody wants expanded."""
    v, rules, start, wide = walk(stream, coder)
    if v:                                                         # the walk refuses: so does the host, unless a cap is in the way
        try:
            R.parse(bytes(stream), coder)
            refuses = False
        except Malformed:
            refuses = True
        assert refuses or wide, "only a cap may separate the walk from the host's parse"
        return ERR_ARG, b"", not refuses
    assert (rules, start) == R.parse(bytes(stream), coder)
    if rules and max(heights(rules)) > cap:
        return ERR_UNSUPPORTED, b"", False
    ln = R.expansion_lengths(rules)
    if sum(1 if x < R.SIGMA else ln[x - R.SIGMA] for x in start) > TEXT_MAX:
        return ERR_TOO_LARGE, b"", False
    return OK, (R.sequential_decode(bytes(stream), coder) if decode else None), False
