"""Crafted encode(huff) streams for the stage decoder tests (tests/test_huff_tables.py on the CPU, tests/test_gpu_huff_tables.py on the
device): complete streams built from ARBITRARY canonical tables, with codes of up to 255 bits -- a depth no real text reaches (a code of
d bits from real counts needs about fib(d) input bytes), but one that a stream header is free to claim and the host decoder accepts.
numpy only; the project's encoder is not involved.

The decoder's convention (HuffmanCoder::Decoder of host/tdc_coders.hpp): numl[l - 1] codes of l bits, first[longest - 1] = 0 and
first[i - 1] = (first[i] + numl[i]) / 2 upwards; the codes of l bits are the values first[l - 1] + off, off < numl[l - 1], MSB first, and
stand for order[prefix[l - 1] + off].  The decoder reads bits while value < first[length - 1].  What follows from the halving:

  * a level above the deepest block whose first is 1 and that has no code halves to 0, and every shorter code becomes unreachable: a
    usable table has a code at every length above its deepest block.
  * a deepest value v is reached only if v >> k < first[longest - 1 - k] for every k.  With D codes at the deepest level and nothing
    between them and the single codes above, first is D >> k there: all D values are reached only if D is a power of two, otherwise
    the first 2^floor(log2 D) of them (Table.usable says which symbols a stream can hold).
  * value - first < numl holds wherever the loop stops below the first level (value < 2 first[length - 2] <= first + numl), and
    first[longest - 1] = 0 stops it at the deepest: the decoder can refuse a bit string only at length 1 (no code "1": top = False
    below), or through a symbol index >= sigma (short_sigma).

Code values stay below 2^16 in every table here: a code is zeros followed by at most 16 significant bits, which is how stream() writes
it without a loop over codes."""
import numpy as np

HD_T = 2048                  # bit positions per tile of the device decoder (csrc/bytestages_decode.hip), counted from the first body bit
HD_CH = 16384                # ... per workgroup of its exit pass
DX_G = 512                   # tiles per group of dx_entries (csrc/tile_chain.hpp)
VALUE_BITS = 16

CHAIN_DEPTHS = (12, 13, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 255)
BUSHY_SHAPES = ((200, 32), (100, 128), (70, 20))


def _codes(numl):
    """first[] as the decoder computes it, and (lengths, values) of the codes by symbol index"""
    numl = np.asarray(numl, dtype=np.int64)
    L = len(numl)
    first = [0] * L
    for i in range(L - 1, 0, -1):
        first[i - 1] = (first[i] + int(numl[i])) // 2
    length = np.repeat(np.arange(1, L + 1), numl)
    prefix = np.concatenate([[0], np.cumsum(numl)[:-1]])
    value = np.asarray(first, dtype=np.int64)[length - 1] + (np.arange(len(length)) - prefix[length - 1])
    assert not len(value) or int(value.max()) < 1 << VALUE_BITS
    return first, length, value


class Table:
    """numl[], order[] and sigma as the header states them, and what the decoder makes of them: per symbol index (canonical order:
    by length, then by value) the code's length and value, and whether a stream can hold it (usable: reachable and index < sigma)"""

    def __init__(self, name, numl, order=None, sigma=None):
        self.name = name
        self.numl = np.asarray(numl, dtype=np.int64)
        assert 1 <= len(self.numl) <= 255 and self.numl.min() >= 0 and self.numl.max() <= 255
        self.longest = L = len(self.numl)
        ncodes = int(self.numl.sum())
        self.sigma = ncodes if sigma is None else sigma
        assert self.sigma <= 256
        self.order = np.asarray(order if order is not None else (np.arange(self.sigma) * 37 + 11) % 256, dtype=np.uint8)
        assert len(self.order) == self.sigma
        first, self.length, self.value = _codes(self.numl)
        self.first = first
        reach = np.ones(ncodes, dtype=bool)
        for j in range(ncodes):
            l, v = int(self.length[j]), int(self.value[j])
            reach[j] = all((v >> k) < first[l - 1 - k] for k in range(1, l))
        self.usable = reach & (np.arange(ncodes) < self.sigma)
        self.symbols = np.flatnonzero(self.usable)            # the symbol indices a sequence may draw from
        self.deepest = self.symbols[self.length[self.symbols] == L]

    def bytes_of(self, idx):
        """the bytes the decoder returns for these symbol indices"""
        return self.order[np.asarray(idx)].tobytes()


def chain(L):
    """numl = [1] * (L - 1) + [2]: the codes 0^(l-1) 1 for l < L, 0^L and 0^(L-1) 1; sigma = L + 1"""
    return Table("chain(%d)" % L, [1] * (L - 1) + [2])


def bushy(L, D, top=True):
    """D codes at depth L and one code at each length 1 .. L - floor(log2 D) (2 .. with top = False: then the bit string "1" is no code
    of the table, the one unassigned code this decoder's tables can have).  The deepest codes stand under the prefix 0^(L - floor(log2 D))."""
    d = int(D).bit_length() - 1
    numl = [1] * (L - d) + [0] * (d - 1) + [D]
    if not top:
        numl[0] = 0
    return Table("bushy(%d,%d)%s" % (L, D, "" if top else "-open"), numl)


def short_sigma(table, sigma):
    """the same lengths under a header whose sigma is smaller than sum(numl): the symbol indices >= sigma are refused"""
    assert sigma < int(table.numl.sum())
    return Table("%s-sigma%d" % (table.name, sigma), table.numl, table.order[:sigma], sigma)


def tables():
    return ([chain(L) for L in CHAIN_DEPTHS] + [bushy(L, D) for L, D in BUSHY_SHAPES] + [bushy(70, 20, top=False), short_sigma(chain(129), 100)])


# ---- the stream -------------------------------------------------------------------------------------------------------------------------
def _groups(v):
    """write_compressed_int: 7 bits per group, low group first, a leading 1 where another follows"""
    out = []
    while True:
        cur, v = v & 127, v >> 7
        out.append((0x80 if v else 0) | cur)
        if not v:
            return out


def header_bytes(numl, order, sigma):
    """the header without its leading bit 1: whole bytes"""
    g = _groups(len(numl))
    for x in numl:
        g += _groups(int(x))
    g += _groups(int(sigma))
    return np.concatenate([np.array(g, dtype=np.uint8), np.frombuffer(bytes(bytearray(order)), dtype=np.uint8)])


def code_list(numl):
    """(lengths, values) of the table's codes by symbol index"""
    return _codes(numl)[1:]


def stream(numl, order, symbol_indices, sigma=None, codes=None):
    """(bytes, hb, total, code_starts): the encode(huff) stream of the codes with these indices under the table (numl, order, sigma;
    sigma = len(order) unless given).  codes = (lengths, values) replaces the table's code list, for bit strings that are no code of
    it.  hb: first body bit, total: bits in front of the terminator, code_starts: the bit at which every code starts."""
    sigma = len(order) if sigma is None else sigma
    lengths, values = (np.asarray(x, dtype=np.int64) for x in (code_list(numl) if codes is None else codes))
    assert (values >> np.minimum(lengths, 62) == 0).all()     # every value fits its length
    idx = np.asarray(symbol_indices, dtype=np.intp)
    head = np.unpackbits(header_bytes(numl, order, sigma))
    hb = 1 + len(head)
    ln = lengths.astype(np.uint8)[idx]
    ends = np.add.accumulate(ln.astype(np.int64))
    total = hb + (int(ends[-1]) if len(ends) else 0)
    bits = np.zeros(total + 16, dtype=np.uint8)               # (room for the terminator)
    bits[0] = 1
    bits[1:hb] = head
    for b in range(VALUE_BITS):                               # bit b of every code that has one there: b positions in front of its end
        has = ((values >> b) & 1).astype(bool) & (lengths > b)
        if has.any():
            pos = ends[has[idx]]
            pos += hb - 1 - b
            bits[pos] = 1
    # BitOStream::finish: 3 bits "number of bits used in the last byte" -- in that byte if it has room, else in a byte of its own
    u = total % 8
    nbytes = total // 8 + 1 if u < 6 else total // 8 + 2
    for k in range(3):
        bits[nbytes * 8 - 3 + k] |= (u >> (2 - k)) & 1
    starts = ends - ln
    starts += hb
    return np.packbits(bits[:nbytes * 8]).tobytes(), hb, total, starts


def table_stream(table, symbol_indices, codes=None):
    return stream(table.numl, table.order, symbol_indices, table.sigma, codes)


# ---- sequences --------------------------------------------------------------------------------------------------------------------------
def _fill(table, gaps):
    """for every gap (bits) the numbers (a, b) of shortest and second-shortest codes that fill it exactly"""
    s, s2 = (int(x) for x in table.symbols[:2])
    ls = int(table.length[s])
    assert int(table.length[s2]) == ls + 1
    b = gaps % ls
    a = (gaps - b * (ls + 1)) // ls
    assert (a >= 0).all()
    return s, s2, a, b


def border_sweep(table, borders):
    """symbol indices: short codes and deepest codes such that for k = 1 .. borders a deepest code starts at body bit
    2048 k - (L - o_k), o_k = (k - 1) mod L, and so the chain enters tile k at offset o_k.  The deepest codes alternate between the
    two lowest (0^L and 0^(L-1) 1): the bit that tells them apart lies behind the border whenever o_k > 0."""
    L = table.longest
    assert borders >= max(2 * L, 520) and len(table.deepest) >= 2
    k = np.arange(1, borders + 1, dtype=np.int64)
    o = (k - 1) % L
    start = HD_T * k - (L - o)
    prev_end = np.concatenate([[0], start[:-1] + L])
    s, s2, a, b = _fill(table, start - prev_end)
    deep = table.deepest[:2][(k - 1) % 2]
    per = np.stack([np.full(borders, s2), np.full(borders, s), deep], axis=1).ravel()
    cnt = np.stack([b, a, np.ones(borders, dtype=np.int64)], axis=1).ravel()
    return np.concatenate([np.repeat(per, cnt), np.full(7, s)])


def uniform(table, nbits, rng):
    """symbol indices uniform over the table's usable symbols, about L / 2 bits a code: as many codes as fit into nbits body bits"""
    n = int(nbits // max(1, int(table.length[table.symbols].mean())) * 2 + 16)
    idx = table.symbols[rng.integers(0, len(table.symbols), size=n)]
    return idx[:int(np.searchsorted(np.cumsum(table.length[idx]), nbits, side="right"))]


def geometric(table, ncodes, rng):
    """the l-th usable symbol with probability 2^-l (the last one takes the rest): about 2 bits a code under a chain table"""
    l = 1 - np.frexp(rng.random(ncodes, dtype=np.float32))[1]          # u in [2^-l, 2^(1-l)) with probability 2^-l
    return table.symbols[np.minimum(l, len(table.symbols)) - 1]


def ending_with_deepest(table, nbits, rng, which=0):
    """a uniform sequence and one deepest code behind it: the last code ends exactly at `total`"""
    return np.concatenate([uniform(table, nbits, rng), table.deepest[which:which + 1]])


# ---- what a sequence covers, from the generator's own positions --------------------------------------------------------------------------
def entry_offsets(code_starts, hb, total):
    """the offset at which the chain of codes enters every tile it reaches (tile 0: offset 0)"""
    rel = np.asarray(code_starts, dtype=np.int64) - hb
    ntiles = (total - hb + HD_T - 1) // HD_T
    border = HD_T * np.arange(ntiles, dtype=np.int64)
    at = np.searchsorted(rel, border, side="left")
    ok = at < len(rel)
    return rel[at[ok]] - border[ok]


def straddles(code_starts, lengths, period, hb=0):
    """which codes have bits on both sides of a multiple of `period` (body bits; code_starts are stream bits, hb the first body bit)"""
    rel = np.asarray(code_starts, dtype=np.int64) - hb
    return rel // period != (rel + np.asarray(lengths) - 1) // period


# ---- streams the decoders must refuse -----------------------------------------------------------------------------------------------------
def refusal_streams(rng):
    """(name, refused stream, the same stream without the refused code): the bit string "1" under bushy(70, 20) without a code of
    length 1, and a symbol index >= sigma under a short-sigma table (a code of 111 bits: the walk refuses it behind its 64th bit) --
    as the first code, in tile 1, in tile 513 and as the last code, in the last tile"""
    out = []
    for table, bad in ((bushy(70, 20, top=False), None), (short_sigma(chain(129), 100), 110)):
        lengths, values = code_list(table.numl)
        if bad is None:                                      # one more entry in the code list: length 1, value 1
            bad = len(lengths)
            lengths, values = np.append(lengths, 1), np.append(values, 1)
        base = uniform(table, 520 * HD_T, rng)
        good = table_stream(table, base)
        rel = good[3] - good[1]
        end = good[2] - good[1]
        if end % HD_T + int(lengths[bad]) > HD_T:            # (the last code must not begin in front of the last tile)
            s, s2, a, b = _fill(table, np.array([HD_T - end % HD_T]))
            base = np.concatenate([base, np.full(int(b[0]), s2), np.full(int(a[0]), s)])
        for where, at in (("first", 0), ("tile1", int(np.searchsorted(rel, HD_T))), ("tile513", int(np.searchsorted(rel, 513 * HD_T))),
                          ("last", len(base))):
            s, hb, total, starts = table_stream(table, np.insert(base, at, bad), (lengths, values))
            tile = int(starts[at] - hb) // HD_T
            assert tile == {"first": 0, "tile1": 1, "tile513": 513}.get(where, (total - hb - 1) // HD_T)
            out.append(("%s %s" % (table.name, where), s, good[0]))
    return out
