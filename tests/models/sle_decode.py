"""Executable model of the device parse of lcpcomp(coder=sle) streams (tudocomp_amd/csrc/decode.hip: dec_token with SleTab, the
next() / orbit / count / scan / emit passes).

Pure Python / numpy, small streams only.  It follows the data flow of the kernels step by step:
  1. the stream's bit length under the BitIStream terminator rule (io/BitIStream.hpp:27-63, :191-193); bits behind it read as zeros;
  2. the header, sequentially (the host does this for the device as well): the ranking of the extended alphabet -- per rank one byte
     or a k-mer tagged 0xFF in its top byte (coders/SLECoder.hpp:325-340) --, then n, flen_min, flen_max, fdist_max;
  3. token_at(x) for EVERY bit position x of a segment: where the token that would start at x ends (next), or "no token";
  4. the orbit of the segment's entry under next(): the real token starts; the exit of one segment is the entry of the next;
  5. every token decoded on its own (literals, source, length), an exclusive scan of what the tokens produce = their text positions;
  6. the references resolved by pointer jumping and the text copied from the literal positions.

The three points where the SLE token differs from the Huffman one (dec_token in decode.hip):
  * a literal code yields 1 or k literals; a k-mer that would run past the run's r-th literal is cut there, the rest is dropped;
  * the factor length is a MinDistributedRange field (:425-444): lbits plain bits if lbits <= 5, else a 2-bit class and 3 / 3 / 4 /
    lbits bits;
  * eof() is false inside a k-mer (:358-366): a last run that ends inside one is followed by a factor all the same, read from the
    zeros behind the end if need be -- what the sequential parser does with the same bytes (sequential_decode below restates it).
Malformed input raises Malformed, nothing else.
"""
import numpy as np

NONE = -1
MAX_RANKS = 4096
MAX_RUN = 512               # DEC_MAX_RUN of decode.hip: streams with longer literal runs keep the sequential parse


class Malformed(ValueError):
    pass


def bits_for(v):
    return max(1, int(v).bit_length())


class Bits:
    """the stream's data bits, MSB first, as one integer; reads behind the end give zeros"""

    PAD = 256

    def __init__(self, stream):
        n = len(stream)
        if n == 0:
            self.total = 0
        else:
            fb = stream[-1] & 7
            if fb >= 6:
                if n < 2:
                    raise Malformed("truncated stream")
                self.total = 8 * (n - 2) + fb
            else:
                self.total = 8 * (n - 1) + fb
        allbits = int.from_bytes(bytes(stream), "big") if n else 0
        self.v = (allbits >> (8 * n - self.total)) << self.PAD if self.total else 0

    def read(self, x, nbits):
        if nbits == 0 or x >= self.total:
            return 0
        assert nbits <= self.PAD
        return (self.v >> (self.total + self.PAD - x - nbits)) & ((1 << nbits) - 1)


class Reader:
    def __init__(self, bits, pos=0):
        self.b, self.pos = bits, pos

    def read(self, nbits):
        v = self.b.read(self.pos, nbits)
        self.pos += nbits
        return v

    def eof(self):
        return self.pos >= self.b.total

    def compressed_int(self):                          # io/BitIStream.hpp:174-188: 7-bit groups, at most 10 of them
        v, i = 0, 0
        while True:
            more = self.read(1)
            v |= self.read(7) << (7 * i)
            i += 1
            if not more or i >= 10:
                return v & ((1 << 64) - 1)


def parse_header(bits, k):
    """the header fields and the table of the literal codes: table[rank] = the bytes the code stands for (1 or k of them)"""
    if not 1 <= k <= 7:
        raise Malformed("kmer out of range")
    r = Reader(bits)
    sigma = r.compressed_int()
    if sigma == 0 or sigma > MAX_RANKS:
        raise Malformed("corrupt SLE ranking")
    table = []
    for _ in range(sigma):
        x = r.compressed_int()
        if (x >> 56) == 0xFF:
            table.append(bytes((x >> (8 * (k - 1 - j))) & 0xFF for j in range(k)))
        else:
            table.append(bytes([x & 0xFF]))
    n = r.read(32)
    W = bits_for(n)
    flen_min, flen_max, fdist_max = r.read(W), r.read(W), r.read(W)
    if n == 0 or n >= 0x7FFFFFFF:
        raise Malformed("text length out of range")
    H = {"k": k, "sigma": sigma, "sb": bits_for(sigma - 1), "table": table, "n": n, "W": W, "flen_min": flen_min, "flen_max": flen_max,
         "fdist_max": fdist_max, "lbits": bits_for((flen_max - flen_min) & ((1 << 64) - 1)), "dbits": bits_for(fdist_max), "x0": r.pos}
    # what the stream can hold at most (a code gives at most k literals, a factor costs at least W bits): before any text-sized array
    total = 8 * ((bits.total + 7) // 8 + 2)
    if n > total * k + (total // W + 1) * max(flen_max, 1):
        raise Malformed("text length out of range")
    return H


def read_rank(r, sb):                                  # SLECoder.hpp:368-404
    if sb < 4:
        return r.read(sb)
    if sb < 6:
        return r.read(sb) if r.read(1) else r.read(2)
    if sb == 6:
        c = r.read(2)
        return r.read(3) if c == 0 else 8 + r.read(3) if c == 1 else 16 + r.read(4) if c == 2 else r.read(sb)
    c = r.read(3)
    if c < 4:
        return 4 * c + r.read(2)
    if c < 7:
        return 16 + 8 * (c - 4) + r.read(3)
    return r.read(sb)


def read_length(r, lbits):                             # MinDistributedRange, :425-444
    if lbits <= 5:
        return r.read(lbits)
    c = r.read(2)
    return r.read(3) if c == 0 else 8 + r.read(3) if c == 1 else 16 + r.read(4) if c == 2 else r.read(lbits)


def code_max(sb):
    return sb if sb < 4 else 1 + sb if sb < 6 else 8 if sb == 6 else 3 + sb


def longest_token(H):
    """la_bits of decode.hip: the longest token a candidate may read"""
    lenf = H["lbits"] if H["lbits"] <= 5 else 2 + H["lbits"]
    return 1 + H["dbits"] + H["fdist_max"] * code_max(H["sb"]) + H["W"] + lenf


def token_at(bits, H, x):
    """The token that starts at bit x: (status, next, literals, src, len) with status 0: literals + factor, 1: literals, then the
    stream ends; or None: no token.  A function of the bits behind x alone."""
    if x >= bits.total:
        return None
    r = Reader(bits, x)
    lits = bytearray()
    open_kmer = False
    if r.read(1):
        run = r.read(H["dbits"])
        if run > H["fdist_max"]:
            return None                                # (bounds the work of a candidate)
        while len(lits) < run:
            rank = read_rank(r, H["sb"])
            if rank >= H["sigma"]:
                return None
            e = H["table"][rank]
            take = min(len(e), run - len(lits))
            lits += e[:take]
            open_kmer = take < len(e)                  # cut k-mer: the rest is dropped, eof() is false here
    if not open_kmer and r.eof():
        return 1, r.pos, bytes(lits), 0, 0
    src = r.read(H["W"])
    length = H["flen_min"] + read_length(r, H["lbits"])
    return 0, r.pos, bytes(lits), src, length


def next_array(bits, H, x_in, m):
    """next() of the segment [x_in, x_in + m) as offsets: m where the token leaves the segment or there is none"""
    nxt = np.full(m, m, dtype=np.int64)
    for i in range(m):
        t = token_at(bits, H, x_in + i)
        if t is not None and t[1] - x_in < m:
            assert 0 < t[1] - (x_in + i) <= longest_token(H)
            nxt[i] = t[1] - x_in
    return nxt


def orbit_of_zero(nxt):
    m = len(nxt)
    mark = np.zeros(m, dtype=bool)
    i = 0
    while i < m:
        mark[i] = True
        i = int(nxt[i])
    return mark


def parse_tokens(stream, k, seg=1 << 30):
    """(H, tokens) -- every token of the stream as (literals, src, len), len 0 for the last token if it carries no factor"""
    bits = Bits(stream)
    H = parse_header(bits, k)
    tokens = []
    x_in = H["x0"]
    produced = 0
    while x_in < bits.total:
        m = min(seg, bits.total - x_in)
        starts = np.flatnonzero(orbit_of_zero(next_array(bits, H, x_in, m))) + x_in
        exit_bit, status = None, 0
        for x in starts:                               # (side by side on the device)
            t = token_at(bits, H, int(x))
            if t is None:
                raise Malformed("malformed token at bit %d" % x)
            status, exit_bit, lits, src, length = t
            if status == 0 and length == 0:
                raise Malformed("factor of length 0 at bit %d" % x)
            produced += len(lits) + length
            if produced > H["n"]:
                raise Malformed("length mismatch")
            tokens.append((lits, src, length))
        if status == 1 or exit_bit >= bits.total:
            break
        if exit_bit <= x_in:
            raise Malformed("token chain")
        x_in = exit_bit
    if produced != H["n"]:
        raise Malformed("length mismatch")
    return H, tokens


def resolve(n, literals, fpos, fsrc, flen):
    """ref[] scatter, pointer jumping to the literal positions, copy pass (decode.hip resolve_and_download)"""
    text = np.array(literals, dtype=np.uint8)
    ref = np.full(n, NONE, dtype=np.int64)
    for p, s, ln in zip(fpos, fsrc, flen):
        ref[p:p + ln] = np.arange(s, s + ln)
    for _ in range(41):
        open_ = ref != NONE
        hop = np.where(open_, ref, 0)
        deeper = open_ & (ref[hop] != NONE)
        if not deeper.any():
            break
        ref[deeper] = ref[ref[deeper]]
    else:
        raise Malformed("reference cycle")
    lit = ref != NONE
    text[lit] = text[ref[lit]]
    return text.tobytes()


def decode(stream, k, seg=1 << 30):
    if parse_header(Bits(stream), k)["fdist_max"] > MAX_RUN:
        return sequential_decode(stream, k)            # (as the library does: a candidate would decode thousands of codes)
    H, tokens = parse_tokens(stream, k, seg)
    n = H["n"]
    literals = np.zeros(n, dtype=np.uint8)
    fpos, fsrc, flen = [], [], []
    p = 0                                              # (the exclusive scan of literals + length over the tokens)
    for lits, src, length in tokens:
        literals[p:p + len(lits)] = np.frombuffer(lits, dtype=np.uint8)
        p += len(lits)
        if length:
            if src + length > n:
                raise Malformed("factor out of range")
            fpos.append(p); fsrc.append(src); flen.append(length)
            p += length
    return resolve(n, literals, fpos, fsrc, flen)


def sequential_decode(stream, k):
    """The sequential parser restated (decode.hip parse_lzss_sle_stream; SLECoder.hpp:351-453 under decode_text_internal): fields
    read one after another with the decoder's k-mer read state.  Not the device formulation -- the yardstick it is compared with."""
    bits = Bits(stream)
    H = parse_header(bits, k)
    n = H["n"]
    r = Reader(bits, H["x0"])
    literals = np.zeros(n, dtype=np.uint8)
    fpos, fsrc, flen = [], [], []
    kmer, kread = b"", None

    def eof():
        return False if kread is not None and kread < k else r.eof()

    p = 0
    while not eof():
        kread = None
        num = r.read(H["dbits"]) if r.read(1) else 0
        if p + num > n:
            raise Malformed("too many literals")
        for _ in range(num):
            if kread is not None and kread < k:
                ch = kmer[kread]
                kread += 1
            else:
                rank = read_rank(r, H["sb"])
                if rank >= H["sigma"]:
                    raise Malformed("rank out of range")
                e = H["table"][rank]
                ch = e[0]
                if len(e) == k and k > 1:
                    kmer, kread = e, 1
            literals[p] = ch
            p += 1
        if not eof():
            kread = None
            src = r.read(H["W"])
            length = H["flen_min"] + read_length(r, H["lbits"])
            if length == 0 or p + length > n or src + length > n:
                raise Malformed("factor out of range")
            fpos.append(p); fsrc.append(src); flen.append(length)
            p += length
    if p != n:
        raise Malformed("length mismatch")
    return resolve(n, literals, fpos, fsrc, flen)


class BitWriter:
    """MSB-first writer with the BitOStream terminator (io/BitOStream.hpp:53-64): builds streams by hand"""

    def __init__(self):
        self.bits = []

    def write(self, value, nbits):
        for i in range(nbits - 1, -1, -1):
            self.bits.append((value >> i) & 1)

    def compressed_int(self, v):
        while True:
            more = 1 if v >> 7 else 0
            self.write(more, 1)
            self.write(v & 0x7F, 7)
            v >>= 7
            if not more:
                return

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
