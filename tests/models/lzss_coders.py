"""Sequential model of the lzss token stream (lzss::encode_text, compressors/lzss/LZSSCoding.hpp:18-92; decode_text_internal,
compressors/LCPCompressor.hpp:23-76) under the coders without a table: BitCoder, EliasGammaCoder, EliasDeltaCoder
(coders/BitCoder.hpp, coders/EliasGammaCoder.hpp:26-29, coders/EliasDeltaCoder.hpp:26-29, io/BitOStream.hpp:105-135).

The token walk is generic over a field writer -- an object with flag(bit), integer(v, lo, hi), literal(byte) that appends (value,
width) pairs to a bit sink -- so that the same walk rendered with an ASCII writer can be pinned against the oracle's ASCIICoder
stream.  encode() is the specification; encode_fast() builds the same fields with numpy for texts of a few MiB; decode() is the
host loop tdc_lzss_decode restates (reads zeros behind the end, refuses what that loop refuses).

A factor list is a sequence of (pos, src, len), sorted by pos, as everywhere in the tests.
"""
import numpy as np

INDEX_MAX = 0xFFFFFFFF
CODERS = ("bit", "gamma", "delta")


class Malformed(Exception):
    pass


def bits_for(v):
    return max(1, int(v).bit_length())


# ---- bit sink + the BitOStream terminator (io/BitOStream.hpp:53-64) ---------------------------------------------------------------
class Sink:
    def __init__(self):
        self.parts = []

    def put(self, v, nb):
        if nb:
            self.parts.append(format(int(v) & ((1 << nb) - 1), "0%db" % nb))

    def bits(self):
        return "".join(self.parts)


def terminate(bits):
    """bit string -> stream: u = bits used in the last byte; u <= 5: the count goes into that byte, else into a byte of its own"""
    u = len(bits) % 8
    body = bits + "0" * (-len(bits) % 8)
    out = bytearray(int(body[i:i + 8], 2) for i in range(0, len(body), 8))
    if u == 0:
        out.append(0)
    elif u <= 5:
        out[-1] |= u
    else:
        out.append(u)
    return bytes(out)


def payload_bits(stream):
    """number of bits in front of the terminator, as io/BitIStream.hpp:27-63 counts them"""
    n = len(stream)
    if n == 0:
        return 0
    fb = stream[-1] & 7
    if n == 1:
        return fb
    return 8 * (n - 2) + fb if fb >= 6 else 8 * (n - 1) + fb


# ---- field writers ------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """Coder.hpp:60-77: Range(lo, hi) -> v - lo in bits_for(hi - lo) bits, truncated like write_int; a literal is a TypeRange<u8>"""
    name = "bit"

    def __init__(self, sink):
        self.s = sink

    def flag(self, b):
        self.s.put(1 if b else 0, 1)

    def integer(self, v, lo, hi):
        self.s.put(v - lo, bits_for(hi - lo))

    def literal(self, c):
        self.s.put(c, 8)


class GammaWriter(BitWriter):
    """every Range but the BitRange: gamma(v) = bits_for(v) zeros, a one, v in bits_for(v) bits; the range is ignored"""
    name = "gamma"

    def code(self, v):
        b = bits_for(v)
        self.s.put(0, b)
        self.s.put(1, 1)
        self.s.put(v, b)

    def integer(self, v, lo, hi):
        self.code(v)

    def literal(self, c):
        self.code(c)


class DeltaWriter(GammaWriter):
    """delta(v) = gamma(bits_for(v)), then v in bits_for(v) bits"""
    name = "delta"

    def code(self, v):
        b = bits_for(v)
        GammaWriter.code(self, b)
        self.s.put(v, b)


class AsciiWriter(BitWriter):
    """coders/ASCIICoder.hpp:29-50, for the cross-check against the oracle: decimal digits + ':', '0' / '1', raw literals"""
    name = "ascii"

    def flag(self, b):
        self.s.put(ord("1" if b else "0"), 8)

    def integer(self, v, lo, hi):
        for ch in str(int(v)) + ":":
            self.s.put(ord(ch), 8)


WRITERS = {"bit": BitWriter, "gamma": GammaWriter, "delta": DeltaWriter, "ascii": AsciiWriter}


# ---- the token walk (LZSSCoding.hpp:18-92) -----------------------------------------------------------------------------------------
def header_values(n, factors):
    """flen_min, flen_max, fdist_max: FactorBuffer's running values (LZSSFactors.hpp:34-47) and the longest literal run"""
    flen_min, flen_max, fdist_max, p = INDEX_MAX, 0, 0, 0
    for pos, _, ln in factors:
        flen_min, flen_max, fdist_max = min(flen_min, ln), max(flen_max, ln), max(fdist_max, pos - p)
        p = pos + ln
    return flen_min, flen_max, max(fdist_max, n - p)


def walk(text, factors, w):
    n = len(text)
    factors = [(int(a), int(b), int(c)) for a, b, c in factors]
    flen_min, flen_max, fdist_max = header_values(n, factors)
    w.integer(n, 0, INDEX_MAX)                                  # len_r
    for v in (flen_min, flen_max, fdist_max):
        w.integer(v, 0, n)                                      # Range(n)
    p = 0
    for pos, src, ln in factors:
        if pos == p:
            w.flag(False)
        else:
            w.flag(True)
            w.integer(pos - p, 0, fdist_max)
        while p < pos:
            w.literal(text[p])
            p += 1
        w.integer(src, 0, n)
        w.integer(ln, flen_min, flen_max)                       # MinDistributedRange(flen_min, flen_max)
        p += ln
    if p < n:
        w.flag(True)
        w.integer(n - p, 0, fdist_max)
    while p < n:
        w.literal(text[p])
        p += 1


def encode_bits(text, factors, coder):
    s = Sink()
    walk(bytes(text), factors, WRITERS[coder](s))
    return s.bits()


def encode(text, factors, coder):
    return terminate(encode_bits(text, factors, coder))


# ---- the same fields with numpy ----------------------------------------------------------------------------------------------------
def _np_bits_for(v):
    v = v.astype(np.uint64)
    b = np.zeros(v.shape, dtype=np.int64)
    x = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        m = x >= (np.uint64(1) << np.uint64(s))
        b[m] += s
        x[m] >>= np.uint64(s)
    return b + 1                                               # (v = 0: 1)


def _np_code(v, coder, width=None, lo=0):
    """(values, widths) of one field per entry of v (values below 2^31: at most 63 bits each)"""
    v = np.asarray(v, dtype=np.uint64)
    if coder == "bit":
        return v - np.uint64(lo), np.full(v.shape, width, dtype=np.int64)
    b = _np_bits_for(v)
    ub = b.astype(np.uint64)
    if coder == "gamma":
        return (np.uint64(1) << ub) | v, 2 * b + 1
    bb = _np_bits_for(ub)
    gam = (np.uint64(1) << bb.astype(np.uint64)) | ub
    return (gam << ub) | v, 2 * bb + 1 + b


def encode_fast(text, factors, coder):
    text = np.frombuffer(bytes(text), dtype=np.uint8)
    n = len(text)
    f = np.asarray([(int(a), int(b), int(c)) for a, b, c in factors], dtype=np.int64).reshape(-1, 3)
    pos, src, ln = f[:, 0], f[:, 1], f[:, 2]
    z = len(f)
    flen_min, flen_max, fdist_max = header_values(n, f.tolist())
    head = Sink()
    w = WRITERS[coder](head)
    w.integer(n, 0, INDEX_MAX)
    for v in (flen_min, flen_max, fdist_max):
        w.integer(v, 0, n)
    hb = head.bits()
    ends = pos + ln
    starts = np.concatenate(([0], ends[:-1])) if z else np.zeros(0, dtype=np.int64)     # where the gap in front of factor i begins
    gap = pos - starts
    tail_at = int(ends[-1]) if z else 0
    covered = np.zeros(n + 1, dtype=np.int64)
    np.add.at(covered, pos, 1)
    np.add.at(covered, ends, -1)
    lit_pos = np.flatnonzero(np.cumsum(covered)[:n] == 0)
    W, lb, db = bits_for(n), bits_for(flen_max - flen_min), bits_for(fdist_max)
    keys, vals, wid = [], [], []

    def add(at, order, vw):
        keys.append(np.asarray(at, dtype=np.int64) * 8 + order)
        vals.append(vw[0])
        wid.append(vw[1])

    add(starts, 0, ((gap > 0).astype(np.uint64), np.ones(z, dtype=np.int64)))
    g = gap > 0
    add(starts[g], 1, _np_code(gap[g], coder, db))
    add(lit_pos, 2, _np_code(text[lit_pos], coder, 8))
    add(pos, 3, _np_code(src, coder, W))
    add(pos, 4, _np_code(ln, coder, lb, flen_min if coder == "bit" else 0))
    if tail_at < n:
        add([tail_at], 0, (np.ones(1, dtype=np.uint64), np.ones(1, dtype=np.int64)))
        add([tail_at], 1, _np_code([n - tail_at], coder, db))
    keys, vals, wid = np.concatenate(keys), np.concatenate(vals).astype(np.uint64), np.concatenate(wid)
    order = np.argsort(keys, kind="stable")
    vals, wid = vals[order], wid[order]
    first = np.cumsum(wid) - wid
    total = int(wid.sum())
    idx = np.repeat(np.arange(len(wid)), wid)
    shift = (wid[idx] - 1 - (np.arange(total) - first[idx])).astype(np.uint64)
    body = ((vals[idx] >> shift) & np.uint64(1)).astype(np.uint8)
    allbits = np.concatenate((np.frombuffer(hb.encode(), dtype=np.uint8) - ord("0"), body))
    u = len(allbits) % 8
    out = bytearray(np.packbits(allbits).tobytes())
    if u == 0:
        out.append(0)
    elif u <= 5:
        out[-1] |= u
    else:
        out.append(u)
    return bytes(out)


# ---- decode_text_internal with the coder's Decoder (the host loop) ------------------------------------------------------------------
class Reader:
    """io/BitIStream.hpp: MSB first, zeros behind the last payload bit"""

    def __init__(self, stream):
        self.total = payload_bits(stream)
        self.bits = format(int.from_bytes(stream, "big"), "0%db" % (8 * len(stream)))[:self.total] if stream else ""
        self.pos = 0

    def eof(self):
        return self.pos >= self.total

    def bit(self):
        return self.int(1)

    def int(self, nb):
        chunk = self.bits[self.pos:self.pos + nb]               # (a read at the end yields zeros and does not move)
        self.pos += len(chunk)
        return int(chunk, 2) << (nb - len(chunk)) if chunk else 0

    def gamma(self):
        one = self.bits.find("1", self.pos)
        b = (one if one >= 0 else self.total) - self.pos        # zeros in front of the one, or up to the end
        if one < 0 or b > 64:
            raise Malformed("unary prefix")
        self.pos = one + 1
        return self.int(b)

    def delta(self):
        b = self.gamma()
        if b > 64:
            raise Malformed("delta width")
        return self.int(b)


MIN_FACTOR_BITS = {"gamma": 4, "delta": 5}


def decode(stream, coder):
    r = Reader(bytes(stream))
    if coder == "bit":
        def integer(lo, hi):
            return lo + r.int(bits_for(hi - lo))

        def literal():
            return r.int(8)
    else:
        code = r.gamma if coder == "gamma" else r.delta

        def integer(lo, hi):
            return code()

        def literal():
            return code() & 0xFF
    n = integer(0, INDEX_MAX)
    if n >= 0x7FFFFFFF:
        raise Malformed("text length")
    flen_min, flen_max, fdist_max = integer(0, n), integer(0, n), integer(0, n)
    bits = 8 * len(stream)
    if n > bits + (bits // MIN_FACTOR_BITS.get(coder, bits_for(n)) + 1) * (flen_max or 1):
        raise Malformed("text length")
    flen_hi = max(flen_max, flen_min)
    text = bytearray(n)
    ref = {}
    p = 0
    while not r.eof():
        num = integer(0, fdist_max) if r.bit() else 0
        if p + num > n:
            raise Malformed("too many literals")
        for _ in range(num):
            text[p] = literal()
            p += 1
        if not r.eof():
            src, ln = integer(0, n), integer(flen_min, flen_hi)
            if ln == 0 or p + ln > n or src + ln > n:
                raise Malformed("factor out of range")
            ref[p] = (src, ln)
            p += ln
    if p != n:
        raise Malformed("length mismatch")
    src_of = np.full(n, -1, dtype=np.int64)
    for q, (src, ln) in ref.items():
        src_of[q:q + ln] = np.arange(src, src + ln)
    out = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    root = np.where(src_of >= 0, src_of, np.arange(n))         # pointer jumping: a literal position is its own root
    for _ in range(bits_for(n) + 1):
        root = root[root]
    if (src_of[root] >= 0).any():
        raise Malformed("reference cycle")
    return out[root].tobytes()
