"""Executable model of lzw(coder=bit | gamma) (tudocomp_amd/csrc/lzw_host.cpp, lzw.hip).

numpy / pure Python, small inputs only:
  * parse(): LZWCompressor::compress (compressors/LZWCompressor.hpp:39-108) -- roots 0 .. 255, node 256 + k = phrase k + next byte;
  * encode(): BitCoder (code k in bits_for(k + 256) bits, Coder.hpp:61-63) or EliasGammaCoder, with the BitOStream terminator;
  * sequential_decode(): LZWCompressor::decompress with lzw::decode_step (lzw/LZWDecoding.hpp:12-99) restated;
  * decode(): the device formulation -- closed-form code offsets S(k) (bit) or the next() / orbit parse (gamma), phrase lengths by
    pointer jumping over k -> c_k - 256, starts by a scan, the factor list (start_k, start_{c_k - 256}, len_k), reference resolution.
Malformed input raises Malformed; a text of more than 2^32 - 2 bytes raises TooLarge (before the text exists).
"""
import numpy as np

from tests.models.lz78_decode import BitWriter, Malformed, TooLarge, stream_bits, orbit_of_zero, MAX_TEXT, NONE

__all__ = ["parse", "encode", "encode_fast", "compress", "sequential_decode", "decode", "offset", "width", "code_at", "Malformed", "TooLarge"]


def bits_for(v):
    """util.hpp:194"""
    return max(1, int(v).bit_length())


def parse(data):
    """the code list of LZWCompressor::compress (the left-over phrase included; none for the empty input)"""
    codes = []
    if not data:
        return codes
    trie = {}
    node = data[0]
    for c in data[1:]:
        child = trie.get((node, c))
        if child is None:
            trie[(node, c)] = 256 + len(codes)
            codes.append(node)
            node = c
        else:
            node = child
    codes.append(node)
    return codes


def encode(codes, coder="bit"):
    """coder.encode(code_k, Range(k + 256)) for every k, then the terminator"""
    w = BitWriter()
    for k, c in enumerate(codes):
        if coder == "bit":
            w.write(c, bits_for(k + 256))
        else:
            w.gamma(c)
    return w.finish()


def encode_fast(codes, coder="bit"):
    """encode() for long code lists: the same bits, placed with numpy (one pass per bit of a code word)"""
    c = np.asarray(codes, dtype=np.int64)
    if len(c) == 0:
        return encode([], coder)
    if coder == "bit":
        w = np.floor(np.log2(np.arange(len(c), dtype=np.float64) + 256)).astype(np.int64) + 1
        val, nb = c, w                                    # the value in w bits
    else:
        b = np.maximum(1, np.floor(np.log2(np.maximum(c, 1).astype(np.float64))).astype(np.int64) + 1)
        val, nb = (np.int64(1) << b) | c, 2 * b + 1       # b zeros, a one, the value in b bits
    end = np.cumsum(nb)
    total = int(end[-1])
    bits = np.zeros(total + ((-total) % 8), dtype=np.uint8)
    for i in range(int(nb.max())):
        m = nb > i
        bits[end[m] - 1 - i] = (val[m] >> i) & 1
    out = bytearray(np.packbits(bits).tobytes())
    u = total & 7
    if u <= 5:
        if u == 0:
            out.append(0)
        out[-1] |= u
    else:
        out.append(u)
    return bytes(out)


def compress(data, coder="bit"):
    codes = parse(data)
    return encode(codes, coder) if len(codes) < 4096 else encode_fast(codes, coder)


# ---- coder=bit: closed-form offsets ---------------------------------------------------------------------------------------------
def width(k):
    return bits_for(k + 256)


def width_base(w):
    """bits in front of the first code of width w: sum_{v=9}^{w-1} v 2^(v-1)"""
    return (w - 2) * (1 << (w - 1)) - 1792


def offset(k):
    """S(k): the bit offset of code k"""
    w = width(k)
    return width_base(w) + (k - ((1 << (w - 1)) - 256)) * w


def code_at(x):
    """(k, w): the code that holds bit x -- the inverse of S"""
    w = 9
    while width_base(w + 1) <= x:
        w += 1
    return ((1 << (w - 1)) - 256) + (x - width_base(w)) // w, w


def _bit_codes(bits, total):
    z, _ = code_at(total)
    if offset(z) != total:
        raise Malformed("cut-off code")
    codes = np.zeros(z, dtype=np.int64)
    for k in range(z):                                    # (side by side on the device)
        x, w = offset(k), width(k)
        v = 0
        for b in bits[x:x + w]:
            v = (v << 1) | int(b)
        if v > 255 + k:
            raise Malformed("invalid compressed code %d at step %d" % (v, k))
        codes[k] = v
    return codes


# ---- coder=gamma: next() of every bit, orbit of bit 0 ------------------------------------------------------------------------------
def _gamma_at(bits, total, x):
    """(end, value) of the gamma code that starts at bit x, or None (field wider than 32 bits, or cut off)"""
    b = 0
    while b <= 32 and (x + b >= total or bits[x + b] == 0):
        b += 1
    if b > 32:
        return None
    end = x + 2 * b + 1
    if end > total:
        return None
    v = 0
    for i in range(b):
        v = (v << 1) | int(bits[x + b + 1 + i])
    return end, v


def _gamma_codes(bits, total, seg):
    codes = []
    x_in = 0
    while x_in < total:
        m = min(seg, total - x_in)
        nxt = np.full(m, m, dtype=np.int64)
        for i in range(m):
            p = _gamma_at(bits, total, x_in + i)
            if p is not None and p[0] - x_in < m:
                nxt[i] = p[0] - x_in
        exit_bit = None
        for x in np.flatnonzero(orbit_of_zero(nxt)) + x_in:
            p = _gamma_at(bits, total, int(x))
            if p is None:
                raise Malformed("malformed or cut-off code at bit %d" % x)
            if p[1] > 255 + len(codes):
                raise Malformed("invalid compressed code %d at step %d" % (p[1], len(codes)))
            codes.append(p[1])
            exit_bit = p[0]
        if exit_bit >= total:
            break
        x_in = exit_bit
    return np.array(codes, dtype=np.int64)


# ---- phrases -> text ---------------------------------------------------------------------------------------------------------------
def phrase_lengths(codes):
    """len_k = 1 for a literal, 1 + len_{c_k - 256} else: synchronous pointer jumping; returns (lengths, rounds)"""
    link = np.where(codes >= 256, codes - 256, NONE).astype(np.int64)
    acc = np.ones(len(codes), dtype=np.int64)
    rounds = 0
    while (link != NONE).any():
        rounds += 1
        live = link != NONE
        tgt = link[live]
        acc[live] = acc[live] + acc[tgt]
        link[live] = link[tgt]
    return acc, rounds


def factor_list(codes, lengths):
    """(n, starts, sources, factor lengths): a literal is a factor of length 0; TooLarge before anything of the text's size"""
    n = int(lengths.sum())
    if n > MAX_TEXT:
        raise TooLarge("text of %d bytes" % n)
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(np.int64)
    ref = codes >= 256
    fsrc = np.where(ref, starts[np.where(ref, codes - 256, 0)], 0)
    return n, starts, fsrc, np.where(ref, lengths, 0)


def resolve(n, codes, fpos, fsrc, flen):
    """literals scattered, ref[] scatter, pointer jumping to the literal positions, copy pass (decode.hip resolve_and_download)"""
    text = np.zeros(n, dtype=np.uint8)
    ref = np.full(n, NONE, dtype=np.int64)
    lit = codes < 256
    text[fpos[lit]] = codes[lit]
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
    cp = ref != NONE
    text[cp] = text[ref[cp]]
    return text.tobytes()


def decode_codes(stream, coder="bit", seg=1 << 30):
    bits, total = stream_bits(stream)
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    return _bit_codes(bits, total) if coder == "bit" else _gamma_codes(bits, total, seg)


def decode(stream, coder="bit", seg=1 << 30):
    """the device formulation"""
    codes = decode_codes(stream, coder, seg)
    if len(codes) == 0:
        return b""
    lengths, _ = phrase_lengths(codes)
    n, fpos, fsrc, flen = factor_list(codes, lengths)
    return resolve(n, codes, fpos, fsrc, flen)


def sequential_decode(stream, coder="bit"):
    """decode_step restated: codes read one after another, every string rebuilt along its (previous code, first byte) chain"""
    bits, total = stream_bits(stream)
    entries = []                                          # entry 256 + j = (code j, first byte of string j + 1)

    def rebuild(x):
        s = []
        while x >= 256:
            prev, ch = entries[x - 256]
            s.append(ch)
            x = prev
        s.append(x)
        return bytes(reversed(s))

    out = bytearray()
    x, k, prev = 0, 0, None
    while x < total:
        if coder == "bit":
            w = width(k)
            if x + w > total:
                raise Malformed("cut-off code")
            c = 0
            for b in bits[x:x + w]:
                c = (c << 1) | int(b)
            x += w
        else:
            p = _gamma_at(bits, total, x)
            if p is None:
                raise Malformed("malformed or cut-off code at bit %d" % x)
            x, c = p
        if c > 255 + k:
            raise Malformed("invalid compressed code %d at step %d" % (c, k))
        if k and c == 255 + k:                            # LZWDecoding.hpp:80-84
            entries.append((prev, rebuild(prev)[0]))
            s = rebuild(c)
        else:                                             # :85-91
            s = rebuild(c)
            if k:
                entries.append((prev, s[0]))
        if len(out) + len(s) > MAX_TEXT:
            raise TooLarge("text of more than 2^32 - 2 bytes")
        out += s
        prev = c
        k += 1
    return bytes(out)
