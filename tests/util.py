import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def pack_fields(fields):
    """(value, bits) pairs -> bytes, MSB first (test::assert_eq_binary of the reference, test/test/util.hpp)."""
    bits = []
    for v, b in fields:
        bits.extend((v >> i) & 1 for i in range(b - 1, -1, -1))
    while len(bits) % 8:
        bits.append(0)
    return bytes(sum(bit << (7 - j) for j, bit in enumerate(bits[i:i + 8])) for i in range(0, len(bits), 8))


def sha256(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def naive_suffix_array(text):
    return np.array(sorted(range(len(text)), key=lambda i: text[i:]), dtype=np.uint32)


def factors_struct(pos, src, length):
    from oracle import oracle as O
    f = np.empty(len(pos), dtype=O.FACTOR_DTYPE)
    f["pos"], f["src"], f["len"] = pos, src, length
    return f


def decode_sequence_case(k):
    """a literal / factor(src, len) sequence of the reference's decode-buffer tests (golden/reference_kats.json "decode_sequences")
    -> (0-terminated text the sequence must decode to, its factors as a FACTOR_DTYPE array in position order).  The literals of the
    sequence are checked against the expected text on the way."""
    want = k["expected"].encode()
    pos, src, length, p = [], [], [], 0
    for tok in k["tokens"]:
        if tok[0] == "lit":
            assert want[p:p + 1] == tok[1].encode(), (k["source"], p)
            p += 1
        else:
            pos.append(p); src.append(tok[1]); length.append(tok[2])
            p += tok[2]
    assert p == len(want)
    return want + b"\0", factors_struct(pos, src, length)


class Bits:
    """MSB-first bit reader (io/BitIStream.hpp) for stream headers."""

    def __init__(self, data):
        self.d, self.p = data, 0

    def bit(self):
        b = (int(self.d[self.p >> 3]) >> (7 - (self.p & 7))) & 1
        self.p += 1
        return b

    def int(self, bits):
        v = 0
        for _ in range(bits):
            v = (v << 1) | self.bit()
        return v

    def compressed_int(self, b=7):            # io/BitIStream.hpp read_compressed_int: b-bit groups, each preceded by a "more" bit
        v, shift = 0, 0
        while True:
            more = self.bit()
            v |= self.int(b) << shift
            shift += b
            if not more:
                return v


def huff_header(stream):
    """The header of a lcpcomp(coder=huff) stream: the Huffman table (huffmantable_encode, HuffmanCoder.hpp:264-273) -- "longest"
    (0 without a table), "numl" (codes per length), "sigma" (literal symbols) -- and the fields behind it (LZSSCoding.hpp:27-41):
    "n", "flen_min", "flen_max", "fdist_max"."""
    from oracle import oracle as O
    r = Bits(stream)
    h = {"longest": 0, "numl": [], "sigma": 0}
    if r.bit():
        h["longest"] = r.compressed_int()
        h["numl"] = [r.compressed_int() for _ in range(h["longest"])]
        h["sigma"] = r.compressed_int()
        for _ in range(h["sigma"]):
            r.int(8)
    h["n"] = r.int(32)
    w = O.bits_for(h["n"])
    h["flen_min"], h["flen_max"], h["fdist_max"] = r.int(w), r.int(w), r.int(w)
    return h
