"""Executable model of the device decoder of lz78(coder=gamma) streams (tudocomp_amd/csrc/lz78_decode.hip).

numpy / pure Python, small streams only.  It follows the data flow of the kernels step by step:
  1. the stream's bit length under the BitIStream terminator rule (io/BitIStream.hpp:27-63, :191-193);
  2. next(x) for EVERY bit position x: where the pair gamma(id) gamma(c) that would start at x ends, or "none";
  3. the orbit of position 0 under next(): the real pair starts (segment by segment, the exit of one is the entry of the next);
  4. every pair decoded and validated on its own (id field <= 32 bits, char field <= 64 bits, not cut off, id_k <= k);
  5. phrase lengths by pointer jumping over the parent links (len_k = 1 + len_{id_k - 1});
  6. an exclusive scan of the lengths = phrase starts; the factor list (start_k, start_{id_k - 1}, len_k - 1) + the literals;
  7. the references resolved by pointer jumping (decode.hip resolve_and_download) and the text copied from the literal positions.
Malformed input raises Malformed; a text of more than 2^32 - 2 bytes raises TooLarge (before the text exists).
"""
import numpy as np

NONE = -1
MAX_TEXT = 2**32 - 2


class Malformed(ValueError):
    pass


class TooLarge(ValueError):
    pass


def stream_bits(stream):
    """(bits as a uint8 array, total) -- the MSB-first bits of the stream and how many of them are data"""
    n = len(stream)
    if n == 0:
        return np.zeros(0, dtype=np.uint8), 0
    fb = stream[-1] & 7
    if fb >= 6:
        if n < 2:
            raise Malformed("truncated stream")
        total = 8 * (n - 2) + fb
    else:
        total = 8 * (n - 1) + fb
    bits = np.unpackbits(np.frombuffer(bytes(stream), dtype=np.uint8))
    return bits, total


def pair_at(bits, total, x):
    """The pair that starts at bit x: (end, id, char) or None (read_elias_gamma<u32>, read_elias_gamma<u8>; zeros behind the end)"""
    def bit(i):
        return int(bits[i]) if i < total else 0

    b1 = 0
    while b1 <= 32 and bit(x + b1) == 0:
        b1 += 1
    if b1 > 32:
        return None                                   # id field wider than 32 bits (or the stream ends in zeros)
    ident = 0
    for i in range(b1):
        ident = (ident << 1) | bit(x + b1 + 1 + i)
    y = x + 2 * b1 + 1
    b2 = 0
    while b2 <= 64 and bit(y + b2) == 0:
        b2 += 1
    if b2 > 64:
        return None                                   # char field wider than 64 bits
    end = y + 2 * b2 + 1
    if end > total:
        return None                                   # cut off by the end of the stream
    ch = 0
    for i in range(b2):
        ch = ((ch << 1) | bit(y + b2 + 1 + i)) & 0xFF  # read_int<uint8_t>: the low 8 bits
    return end, ident, ch


def next_array(bits, total, x_in, m):
    """next() of the segment [x_in, x_in + m) as offsets: m where the pair leaves the segment or there is none"""
    nxt = np.full(m, m, dtype=np.int64)
    for i in range(m):
        p = pair_at(bits, total, x_in + i)
        if p is not None and p[0] - x_in < m:
            nxt[i] = p[0] - x_in
    return nxt


def orbit_of_zero(nxt):
    m = len(nxt)
    mark = np.zeros(m, dtype=bool)
    i = 0
    while i < m:
        mark[i] = True
        i = int(nxt[i])
    return mark


def parse_pairs(stream, seg=1 << 30):
    """All pairs of the stream as (ids, chars) -- the device's next() / orbit / decode passes, segment by segment"""
    bits, total = stream_bits(stream)
    ids, chars = [], []
    x_in = 0
    while x_in < total:
        m = min(seg, total - x_in)
        starts = np.flatnonzero(orbit_of_zero(next_array(bits, total, x_in, m))) + x_in
        exit_bit = None
        for x in starts:                              # (side by side on the device)
            k = len(ids)
            p = pair_at(bits, total, int(x))
            if p is None:
                raise Malformed("malformed or cut-off pair at bit %d" % x)
            end, ident, ch = p
            if ident > k:
                raise Malformed("pair %d names phrase %d" % (k, ident))
            ids.append(ident)
            chars.append(ch)
            exit_bit = end
        if exit_bit >= total:
            break
        x_in = exit_bit
    return np.array(ids, dtype=np.int64), np.array(chars, dtype=np.uint8)


def phrase_lengths(ids):
    """len_k by synchronous pointer jumping over the parent links; returns (lengths, rounds)"""
    z = len(ids)
    link = np.where(ids > 0, ids - 1, NONE).astype(np.int64)
    acc = np.ones(z, dtype=np.int64)
    rounds = 0
    while (link != NONE).any():
        rounds += 1
        live = link != NONE
        tgt = link[live]
        acc[live] = acc[live] + acc[tgt]
        link[live] = link[tgt]
    return acc, rounds


def factor_list(ids, lengths):
    """starts (exclusive scan, 64-bit), the factor list and the literal positions; TooLarge before any text-sized array"""
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(np.int64) if len(lengths) else np.zeros(0, dtype=np.int64)
    n = int(lengths.sum()) if len(lengths) else 0
    if n > MAX_TEXT:
        raise TooLarge("text of %d bytes" % n)
    fsrc = np.where(ids > 0, starts[np.maximum(ids - 1, 0)], 0)
    return n, starts, fsrc, lengths - 1


def resolve(n, fpos, fsrc, flen, chars):
    """ref[] scatter, pointer jumping to the literal positions, copy pass"""
    text = np.zeros(n, dtype=np.uint8)
    ref = np.full(n, NONE, dtype=np.int64)
    text[fpos + flen] = chars
    for p, s, ln in zip(fpos, fsrc, flen):
        if ln:
            ref[p:p + ln] = np.arange(s, s + ln)
    while True:
        open_ = ref != NONE
        hop = np.where(open_, ref, 0)
        deeper = open_ & (ref[hop] != NONE)
        if not deeper.any():
            break
        ref[deeper] = ref[ref[deeper]]
    lit = ref != NONE
    text[lit] = text[ref[lit]]
    return text.tobytes()


def sequential_decode(stream):
    """The reference's loop restated (LZ78Compressor.hpp:142-160): pairs read one after another from bit 0, every phrase expanded
    along its parent chain.  Not the device formulation -- the yardstick it is compared with.  Same rejections (Malformed)."""
    bits, total = stream_bits(stream)
    parent, chars, out = [], [], bytearray()
    x = 0
    while x < total:
        p = pair_at(bits, total, x)
        if p is None:
            raise Malformed("malformed or cut-off pair at bit %d" % x)
        end, ident, ch = p
        if ident > len(parent):
            raise Malformed("pair %d names phrase %d" % (len(parent), ident))
        phrase = [ch]
        q = ident
        while q:
            phrase.append(chars[q - 1])
            q = parent[q - 1]
        out += bytes(reversed(phrase))
        parent.append(ident)
        chars.append(ch)
        x = end
    return bytes(out)


def decode(stream, seg=1 << 30):
    ids, chars = parse_pairs(stream, seg)
    if len(ids) == 0:
        return b""
    lengths, _ = phrase_lengths(ids)
    n, fpos, fsrc, flen = factor_list(ids, lengths)
    return resolve(n, fpos, fsrc, flen, chars)


class BitWriter:
    """MSB-first writer with the BitOStream terminator (io/BitOStream.hpp:53-64): builds streams by hand"""

    def __init__(self):
        self.bits = []

    def write(self, value, nbits):
        for i in range(nbits - 1, -1, -1):
            self.bits.append((value >> i) & 1)

    def gamma(self, v, width=None):
        """gamma(v) as BitOStream::write_elias_gamma writes it; `width` forces the field width (malformed streams)"""
        b = width if width is not None else max(1, int(v).bit_length())
        self.write(0, b)
        self.write(1, 1)
        self.write(v, b)

    def pair(self, ident, ch, id_width=None, ch_width=None):
        self.gamma(ident, id_width)
        self.gamma(ch, ch_width)

    def finish(self):
        total = len(self.bits)
        b = list(self.bits) + [0] * ((-total) % 8)
        out = bytearray(np.packbits(np.array(b, dtype=np.uint8)).tobytes()) if b else bytearray()
        u = total & 7
        if u <= 5:
            if u == 0:
                out.append(0)
            out[-1] |= u
        else:
            out.append(u)
        return bytes(out)
