"""Model of the byte-stream compressors behind bwt in the reference's `bwtzip = bwt:rle:mtf:encode(huff)` chain.

rle   compressors/RunLengthEncoder.hpp:15-50 with util/vbyte.hpp: what the loop emits on x86-64, where `char` is signed and
      istream::peek() yields 0 .. 255 -- only bytes below 0x80 extend a run -- and the loop cut off at the end of an input that ends
      in 0xFF 0xFF (the reference does not terminate there: peek() == EOF == (char)0xFF for ever)
mtf   compressors/MTFCompressor.hpp:16-43, and the chunk-summary formulation the device kernels use
encode(huff) is oracle.huff_encode_literals(data, interleave=False).
Plain Python, no GPU."""


def vbyte(v):
    out = bytearray()
    while v >= 128:
        out.append(0x80 | (v & 0x7F))
        v >>= 7
    out.append(v)
    return bytes(out)


def read_vbyte(data, i):
    """(value, next index); ValueError if the vbyte runs off the end or is longer than ten bytes"""
    v = 0
    for k in range(11):
        if i >= len(data):
            raise ValueError("vbyte runs off the end")
        if k == 10:
            raise ValueError("vbyte longer than ten bytes")
        b = data[i]
        i += 1
        v |= (b & 0x7F) << (7 * k)
        if not b & 0x80:
            return v, i
    raise AssertionError


def rle_encode(data, offset=0):
    data = bytes(data)
    out = bytearray()
    i, n = 0, len(data)
    while i < n:
        c = data[i]
        k = 1
        while i + k < n and data[i + k] == c:
            k += 1
        if c < 0x80:
            out.append(c)
            if k > 1:
                out.append(c)
                out += vbyte(k - 2 + offset)
        else:                                   # never extends a run: every repeated byte is a pair of its own
            out.append(c)
            out += (bytes([c]) + vbyte(offset)) * (k - 1)
        i += k
    return bytes(out)


def rle_decode(data, offset=0):
    data = bytes(data)
    out = bytearray()
    if not data:
        return b""
    prev = data[0]
    out.append(prev)
    i = 1
    while i < len(data):
        c = data[i]
        i += 1
        if c == prev:
            v, i = read_vbyte(data, i)
            if v < offset:
                raise ValueError("run length below the offset")
            out += bytes([c]) * (v - offset)
        out.append(c)
        prev = c
    return bytes(out)


def mtf_encode(data, lst=None):
    lst = list(range(256)) if lst is None else lst
    out = bytearray()
    for c in bytes(data):
        j = lst.index(c)
        out.append(j)
        del lst[j]
        lst.insert(0, c)
    return bytes(out)


def mtf_decode(data):
    lst = list(range(256))
    out = bytearray()
    for j in bytes(data):
        c = lst.pop(j)
        out.append(c)
        lst.insert(0, c)
    return bytes(out)


def chunk_summary(chunk):
    """the distinct bytes of the chunk, last occurrence first (walked backwards with a seen set)"""
    seen, out = set(), []
    for c in reversed(bytes(chunk)):
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def compose(earlier, later):
    """summary of `earlier` followed by `later`: associative"""
    s = set(later)
    return list(later) + [c for c in earlier if c not in s]


def mtf_encode_chunked(data, chunk):
    """mtf_encode through summaries: the list in front of chunk k is the composed summary of chunks 0 .. k - 1, then what is left of
    0 .. 255 in its old order; every chunk is then encoded from its own list, independently of the others"""
    data = bytes(data)
    out = bytearray()
    prefix = []
    for a in range(0, len(data), chunk):
        part = data[a:a + chunk]
        out += mtf_encode(part, compose(list(range(256)), prefix))
        prefix = compose(prefix, chunk_summary(part))
    return bytes(out)


def rle_encode_np(data, offset=0):
    """rle_encode with numpy, for inputs of megabytes (the tests check it against rle_encode).  A unit is a maximal run of bytes below
    0x80 or one byte from 0x80 up; every unit emits its byte, a run of two and more a second copy and vbyte(k - 2 + offset), a byte
    from 0x80 up that repeats its predecessor vbyte(offset)."""
    import numpy as np
    s = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n = len(s)
    if n == 0:
        return b""
    same = np.zeros(n, dtype=bool)
    same[1:] = s[1:] == s[:-1]
    heads = np.flatnonzero(~same | (s >= 0x80))
    k = np.diff(np.append(heads, n)).astype(np.uint64)
    c = s[heads]
    low = c < 0x80
    has_v = np.where(low, k > 1, same[heads])
    val = np.where(low, k - np.uint64(2) + np.uint64(offset), np.uint64(offset))
    val = np.where(has_v, val, np.uint64(0))
    vlen = np.ones(len(heads), dtype=np.int64)
    t = val >> np.uint64(7)
    while t.any():
        vlen += t > 0
        t >>= np.uint64(7)
    size = 1 + (low & (k > 1)) + np.where(has_v, vlen, 0)
    off = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    out = np.zeros(int(size.sum()), dtype=np.uint8)
    out[off] = c
    two = low & (k > 1)
    out[off[two] + 1] = c[two]
    vpos = off + 1 + two
    for j in range(10):
        m = has_v & (vlen > j)
        if not m.any():
            break
        more = (vlen[m] > j + 1).astype(np.uint8) << 7
        out[vpos[m] + j] = ((val[m] >> np.uint64(7 * j)) & np.uint64(0x7F)).astype(np.uint8) | more
    return out.tobytes()
