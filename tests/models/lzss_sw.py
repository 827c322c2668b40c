"""Sequential model of lzss = LZSSSlidingWindowCompressor<coder> (compressors/LZSSSlidingWindowCompressor.hpp:39-143).

reference_loop() restates the reference's compress loop literally -- the buffer of 2 * window bytes, `ahead`, the erase per text byte --
and parse() is the closed form the library implements (tdc_lzss_sw_factors on the host, lzss_sw.hip on the device): what the buffer
holds at text position p is a function of p, n and w alone.  Both return the token list; tests/test_lzss_sw_model.py holds them against
each other.  encode() writes the tokens through the field writers of tests/models/lzss_coders.py, decode() is the reference's decode
loop with the refusals of tdc_lzss_sw_decode.

A token is (p, None, byte) for a literal and (p, s, j) for a factor of j bytes at p copied from s.
"""
import numpy as np

from tests.models.lzss_coders import Malformed, Reader, Sink, WRITERS, bits_for, terminate

CODERS = ("ascii", "bit", "gamma", "delta")
TEXT_MAX = 0xFFFFFFFE
MASK64 = (1 << 64) - 1
WINDOWS = (1, 2, 3, 4, 5, 8, 16)
THRESHOLDS = (0, 1, 2, 3, 5)


def sweep(seed, count):
    """the cases of the CPU tests: random texts over 1 - 3 letters, n in [0, 6w + 8), every window x threshold pair in turn"""
    rng = np.random.default_rng(seed)
    for i in range(count):
        w = WINDOWS[i % len(WINDOWS)]
        t = THRESHOLDS[(i // len(WINDOWS)) % len(THRESHOLDS)]
        n = int(rng.integers(0, 6 * w + 8))
        sigma = int(rng.integers(1, 4))
        yield (rng.integers(0, sigma, size=n, dtype=np.uint8) + ord("a")).tobytes(), w, t


class TooLarge(Exception):
    pass


def reference_loop(data, w, t):
    """:39-118, line by line: `ins` is the input stream, buf the sliding buffer"""
    data = bytes(data)
    ins = iter(data)
    tokens = []
    buf = []
    ahead = 0
    buf_off = 0
    while len(buf) < 2 * w:                                       # :53 initially fill the buffer
        c = next(ins, None)
        if c is None:
            break
        buf.append(c)
    pos = 0
    eof = False
    while ahead < len(buf):                                       # :63
        fpos = fsrc = fnum = 0
        for k in range(ahead - w if ahead > w else 0, ahead):     # :67 walk back buffer
            j = 0
            while ahead + j < len(buf) and buf[k + j] == buf[ahead + j]:
                j += 1
            if j >= t and j > fnum:                               # :75
                fpos, fsrc, fnum = buf_off + ahead, buf_off + k, j
        if fnum > 0:
            tokens.append((fpos, fsrc, fnum))
            advance = fnum
        else:
            tokens.append((pos, None, buf[ahead]))
            advance = 1
        pos += advance
        for _ in range(advance):                                  # :102 advance buffer
            if ahead < w:
                ahead += 1                                        # case 1: still reading the first w symbols
            else:
                c = None if eof else next(ins, None)
                if c is not None:                                 # case 2: read a new symbol
                    del buf[0]
                    buf.append(c)
                    buf_off += 1
                else:                                             # case 3: EOF, read rest of buffer
                    eof = True
                    ahead += 1
    return tokens


def look_ahead(p, n, w):
    """L(p): how far the buffer reaches behind text position p"""
    end = n if n < 2 * w else min(max(p - w, 0), n - 2 * w) + 2 * w
    return end - p


def parse(data, w, t):
    """the closed form: candidates s in [max(0, p - w), p) ascending, match min(lce(s, p), L(p)), strict improvement from t (0 acts as 1)"""
    data = bytes(data)
    n = len(data)
    t = max(int(t), 1)
    tokens = []
    p = 0
    while p < n:
        L = look_ahead(p, n, w)
        best, bsrc = 0, 0
        for s in range(max(0, p - w), p):
            j = 0
            while j < L and data[s + j] == data[p + j]:
                j += 1
            if j >= t and j > best:
                best, bsrc = j, s
        if best:
            tokens.append((p, bsrc, best))
            p += best
        else:
            tokens.append((p, None, data[p]))
            p += 1
    return tokens


def factors(data, w, t):
    """the factors of parse() as (pos, src, len), sorted by pos"""
    return [tok for tok in parse(data, w, t) if tok[1] is not None]


def truncates(data, w, t):
    """coder=bit would drop bits of a length: write_int(len, bits_for(w)) with len >= 2^bits_for(w)"""
    return any(j >> bits_for(w) for _, s, j in parse(data, w, t) if s is not None)


def encode_bits(tokens, coder, w):
    sink = Sink()
    wr = WRITERS[coder](sink)
    for p, s, v in tokens:
        if s is None:
            wr.flag(False)                                        # :94-95
            wr.literal(v)
        else:
            wr.flag(True)                                         # :87-89
            wr.integer(p - s, 0, p)
            wr.integer(v, 0, w)
    return sink.bits()


def encode(tokens, coder, w):
    return terminate(encode_bits(tokens, coder, w))


class _Reader(Reader):
    """the bit reader with the note tdc_lzss_sw_decode takes: a bit was asked for behind the end"""

    def __init__(self, stream):
        Reader.__init__(self, stream)
        self.over = False

    def int(self, nb):
        if self.pos + nb > self.total:
            self.over = True
        return Reader.int(self, nb)


def decode(stream, coder, w=16):
    """:120-143; Malformed / TooLarge where tdc_lzss_sw_decode returns TDC_GPU_ERR_ARG / TDC_GPU_ERR_TOO_LARGE"""
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

        def integer(hi):                                          # coders/ASCIICoder.hpp:53-84 as tdc_coders.hpp restates it
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
    text = bytearray()
    while not r.eof():
        if flag():
            dist = integer(len(text))
            num = integer(w)
            if r.over:
                raise Malformed("cut-off factor")
            if dist == 0 or dist > len(text):
                raise Malformed("factor source out of range")
            if num > TEXT_MAX - len(text):
                raise TooLarge()
            src = len(text) - dist
            for i in range(num):
                text.append(text[src + i])
        else:
            c = literal()
            if r.over:
                raise Malformed("cut-off literal")
            if len(text) >= TEXT_MAX:
                raise TooLarge()
            text.append(c)
    return bytes(text)
