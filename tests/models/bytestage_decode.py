"""Model of the device decoders of rle, mtf and encode(huff) (csrc/bytestages_decode.hip): the PARALLEL formulations,
not the serial loops -- those are the host decoders (T.rle_decode, T.mtf_decode, T.huff_decode_literals), against which the tests
compare these functions, refusals included.  Tile and group sizes are parameters so that small inputs cross many borders.

  mtf:   a chunk of ranks run on the identity list yields its permutation and a symbolic output (indices into the list the chunk starts
         from); permutations compose associatively, (a o b)[j] = a[b[j]]; reduce over groups, bring the lists back down, gather.
  huff:  next(x) = x + code length at bit x; per tile the exit of every entry offset < longest; tiles compose; codes per tile, scan, emit.
  rle:   nodes (x, eq): eq = "this data byte equals the previous data byte", a vbyte follows; the same tile scheme with 2 x 11 states;
         run lengths, scan, and a fill in which every piece of the output finds its run through a maximum scan over piece borders.
"""
import numpy as np

NONE = -1
M64 = (1 << 64) - 1
STAGE_MAX = (1 << 32) - 2


class Refused(ValueError):
    pass


# ---- tile exits -> tile entries, any number of levels -------------------------------------------------------------------------------
def entries_from_exits(exits, group, e0=0):
    """exits[t][o] = state in which the chain that enters tile t in state o enters tile t + 1 (NONE: it ends in t).  Returns the entry
    state of every tile; groups of `group` tiles are composed level by level until one group is left (the hand-over between groups is
    what the device does between its three levels)."""
    n = len(exits)
    if n <= group:
        out, e = [], e0
        for t in range(n):
            out.append(e)
            e = exits[t][e] if e != NONE else NONE
        return out
    S = len(exits[0])
    hi = []
    for g in range(0, n, group):
        row = []
        for o in range(S):
            e = o
            for t in range(g, min(g + group, n)):
                if e == NONE:
                    break
                e = exits[t][e]
            row.append(e)
        hi.append(row)
    top = entries_from_exits(hi, group, e0)
    out = []
    for gi, g in enumerate(range(0, n, group)):
        e = top[gi]
        for t in range(g, min(g + group, n)):
            out.append(e)
            e = exits[t][e] if e != NONE else NONE
    return out


# ---- mtf ---------------------------------------------------------------------------------------------------------------------------
def mtf_chunk(ranks):
    """the chunk on the identity list: (permutation = the list it leaves behind, symbolic output)"""
    L = list(range(256))
    sym = []
    for r in ranks:
        c = L.pop(r)
        L.insert(0, c)
        sym.append(c)
    return np.array(L, dtype=np.uint8), bytes(sym)


def compose(a, b):
    return a[b]


def mtf_lists(rows, group, seed=None):
    """the list in front of every row's chunk: reduce per group, recurse, come back down"""
    ident = np.arange(256, dtype=np.uint8)
    seed = ident if seed is None else seed
    if len(rows) <= group:
        out, w = [], seed
        for r in rows:
            out.append(w)
            w = compose(w, r)
        return out
    tot = []
    for g in range(0, len(rows), group):
        w = ident
        for r in rows[g:g + group]:
            w = compose(w, r)
        tot.append(w)
    parents = mtf_lists(tot, group, seed)
    out = []
    for gi, g in enumerate(range(0, len(rows), group)):
        out += mtf_lists(rows[g:g + group], group, parents[gi])
    return out


def mtf_decode(data, chunk=16, group=4):
    parts = [mtf_chunk(data[i:i + chunk]) for i in range(0, len(data), chunk)]
    lists = mtf_lists([p for p, _ in parts], group)
    return b"".join(bytes(lists[i][np.frombuffer(sym, dtype=np.uint8)]) for i, (_, sym) in enumerate(parts))


# ---- encode(huff) --------------------------------------------------------------------------------------------------------------------
class _Bits:
    """io/BitIStream.hpp: MSB first, `total` bits in front of the terminator, zeros at the end without moving on"""

    def __init__(self, data, total):
        self.d, self.total, self.pos = data, total, 0

    def bit_at(self, x):
        return (self.d[x >> 3] >> (7 - (x & 7))) & 1 if x < self.total else 0

    def bit(self):
        if self.pos >= self.total:
            return 0
        b = self.bit_at(self.pos)
        self.pos += 1
        return b

    def int(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def cint(self):
        v, i = 0, 0
        while True:
            more = self.bit()
            v |= (self.int(7) << ((7 * i) & 63)) & M64       # (64-bit shift as the host executes it)
            i += 1
            if not more:
                return v


def huff_total_bits(s):
    if not s:
        raise Refused("no header")
    u = s[-1] & 7
    if u >= 6 and len(s) < 2:
        raise Refused("no header")
    total = (len(s) - 2) * 8 + u if u >= 6 else (len(s) - 1) * 8 + u
    if total < 1:
        raise Refused("no header")
    return total


def huff_header(s, total):
    """None (no table, body at bit 1) or (longest, numl, first, prefix, order, sigma, first body bit); the checks of huff_decode_literals"""
    if not s[0] & 0x80:
        return None
    probe = _Bits(s, total)
    need = 1

    def group():
        nonlocal need
        v = probe.cint()
        need += 8
        x = v >> 7
        while x:
            need += 8
            x >>= 7
        return v

    probe.bit()
    longest = group() & 0xFF
    i = 0
    while i < longest and need <= total:
        group()
        i += 1
    sigma = group() if need <= total else 0
    need += 8 * sigma
    if need > total or not longest or sigma > 256:
        raise Refused("header cut off or inconsistent")
    b = _Bits(s, total)
    b.bit()
    longest = b.cint() & 0xFF
    numl = [b.cint() & 0xFF for _ in range(longest)]
    sigma = b.cint()
    order = [b.int(8) for _ in range(sigma)]
    first = [0] * longest
    for i in range(longest - 1, 0, -1):
        first[i - 1] = ((first[i] + numl[i]) & M64) // 2
    prefix, acc = [], 0
    for l in range(longest):
        prefix.append(acc)
        acc += numl[l]
    return longest, numl, first, prefix, order, sigma, b.pos


def huff_code(bits, hdr, x):
    """huffman_decode at bit x: (length, symbol), length 0 = no code of the table"""
    if hdr is None:
        return 8, sum(bits.bit_at(x + k) << (7 - k) for k in range(8))
    longest, numl, first, prefix, order, sigma, _ = hdr
    value, length = 0, 0
    while True:
        value = ((value << 1) + bits.bit_at(x + length)) & M64
        length += 1
        if not (length <= longest and value < first[length - 1]):
            break
    if length > longest:
        return 0, 0
    length -= 1
    off = (value - first[length]) & M64
    if off >= numl[length] or prefix[length] + off >= sigma:
        return 0, 0
    return length + 1, order[prefix[length] + off]


def huff_decode(s, tile=64, group=4):
    s = bytes(s)
    total = huff_total_bits(s)
    hdr = huff_header(s, total)
    bits = _Bits(s, total)
    hb = 1 if hdr is None else hdr[6]
    la = 8 if hdr is None else hdr[0]
    tile = max(tile, la)
    m = total - hb
    if m <= 0:
        return b""
    # next(x) - x of every body position (0: no code), exits per tile for the entry offsets < la
    nxl = [huff_code(bits, hdr, hb + i)[0] for i in range(m)]
    ntiles = (m + tile - 1) // tile
    exits = []
    for t in range(ntiles):
        row = []
        for o in range(la):
            e, res = t * tile + o, NONE
            while True:
                if e >= (t + 1) * tile:
                    res = e - (t + 1) * tile
                    break
                if e >= m or not nxl[e]:
                    break
                e += nxl[e]
            row.append(res)
        exits.append(row)
    entry = entries_from_exits(exits, group)
    # count per tile, scan, emit
    out = []
    for t in range(ntiles):
        if entry[t] == NONE:
            continue
        x, end = t * tile + entry[t], min((t + 1) * tile, m)
        while x < end:
            l, sym = huff_code(bits, hdr, hb + x)
            if not l:
                raise Refused("code outside the table")
            out.append(sym)
            x += l
    if len(out) > STAGE_MAX:
        raise Refused("too large")
    return bytes(out)


# ---- rle -----------------------------------------------------------------------------------------------------------------------------
RLE_TOK = 11
CLAMP = 1 << 33


def rle_token(s, x, eq, offset):
    """the token at data byte x in state eq: (output length, next data byte, its state) or None (malformed)"""
    n, nx, length = len(s), x + 1, 1
    if eq:
        v, k = 0, 0
        while True:
            if nx >= n or k == 10:
                return None
            b = s[nx]
            nx += 1
            v |= ((b & 0x7F) << (7 * k)) & M64
            k += 1
            if not b & 0x80:
                break
        if v < offset:
            return None
        length = 1 + min(v - offset, CLAMP)
    return length, nx, int(nx < n and s[nx] == s[x])


def rle_decode(s, offset=0, tile=16, group=4, piece=8, limit=STAGE_MAX):
    s = bytes(s)
    n = len(s)
    if not n:
        return b""
    tile = max(tile, RLE_TOK)
    ntiles = (n + tile - 1) // tile
    exits = []
    for t in range(ntiles):
        row = []
        for st in range(2 * RLE_TOK):
            x, eq, res = t * tile + (st >> 1), st & 1, NONE
            while True:
                if x >= (t + 1) * tile:
                    res = (x - (t + 1) * tile) * 2 + eq
                    break
                if x >= n:
                    break
                tok = rle_token(s, x, eq, offset)
                if tok is None:
                    break
                _, x, eq = tok
            row.append(res)
        exits.append(row)
    entry = entries_from_exits(exits, group)        # the orbit of (0, 0); a group's exit is the next group's entry

    def tokens(t):
        if entry[t] == NONE:
            return
        x, eq, end = t * tile + (entry[t] >> 1), entry[t] & 1, min((t + 1) * tile, n)
        while x < end:
            tok = rle_token(s, x, eq, offset)
            if tok is None:
                raise Refused("malformed vbyte")
            yield s[x], tok[0]
            _, x, eq = tok

    sums = [min(sum(l for _, l in tokens(t)), CLAMP) for t in range(ntiles)]
    total = sum(sums)
    if total > limit:
        raise Refused("decodes to more than the limit")
    out = bytearray(total)
    npieces = total // piece + 1
    head, info = [0] * npieces, [None] * npieces
    p = 0
    for t in range(ntiles):
        for c, l in tokens(t):
            end, border = p + l, (p + piece - 1) // piece * piece
            if p < min(end, border):
                out[p:min(end, border)] = bytes([c]) * (min(end, border) - p)
            if border < end:
                head[border // piece] = border // piece + 1
                info[border // piece] = (end, c)
            p = end
    hmax = np.maximum.accumulate(np.array(head, dtype=np.int64)) if npieces else []
    for ot in range(npieces):                       # every piece on its own: no loop over a run
        if ot * piece >= total or not hmax[ot]:
            continue
        end, c = info[hmax[ot] - 1]
        lim = min(end, (ot + 1) * piece)
        if ot * piece < lim:
            out[ot * piece:lim] = bytes([c]) * (lim - ot * piece)
    return bytes(out)
