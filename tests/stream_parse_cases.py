"""Hand-built streams for the parse that the device decoders of lz78, lzw, lzss and repair share (tudocomp_amd/csrc/stream_parse.hpp):
bit strings put together field by field, so that a field can be given a width no encoder writes.  Three families:

  cap_cases       fields at the caps of the shared gamma / delta reader, fields that end with the stream, are cut one bit short, or
                  are followed by zeros only
  straddle        a token of natural widths that starts d bits in front of the border of the first 32768-bit tile of a segment
  residue_streams one-byte and two-byte streams for every terminator residue that changes the payload-bit rule

A case is (name, stream, wide): `wide` says that a field lies beyond a cap of the device (lzss refuses such a stream, repair hands it
to the host loop).  tests/test_stream_parse_model.py holds the streams against the Python models and the host loops,
tests/test_gpu_stream_parse.py runs them on the device.
"""
import tudocomp_amd as T
from tests.models import lz78_decode as M78
from tests.models.lzss_coders import bits_for, terminate

ERR_ARG = -2
CID = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
TILE = 32768
DECODERS = ("lzss", "repair", "lz78", "lzw")
CODERS = {"lzss": ("bit", "gamma", "delta"), "repair": ("bit", "gamma", "delta"), "lz78": ("gamma",), "lzw": ("gamma",)}
WINDOW = 16                                   # lzss: the width of a length field under bit is bits_for(WINDOW)
STRADDLE_D = (1, 17, 64, 130)


def host(decoder, stream, coder):
    """(status, text) of the host loop that specifies the decoder; lz78 has none in Python: the model's sequential reading"""
    try:
        if decoder == "lzss":
            return 0, T.lzss_sw_decode(stream, CID[coder], WINDOW)
        if decoder == "repair":
            return 0, T.repair_decode(stream, CID[coder])
        if decoder == "lzw":
            return 0, T.lzw_decode(stream, CID[coder])
        return 0, M78.sequential_decode(stream)
    except (T.TdcGpuError, M78.Malformed) as e:
        return getattr(e, "status", ERR_ARG), None


def gamma(v, b=None):
    """b zeros, a one, v in b bits; b defaults to bits_for(v)"""
    b = bits_for(v) if b is None else b
    assert v < 1 << b
    return "0" * b + "1" + format(v, "0%db" % b)


def delta(v, b=None, wb=None):
    """gamma(b) with wb value bits, then v in b bits"""
    b = bits_for(v) if b is None else b
    assert v < 1 << b
    return gamma(b, wb) + format(v, "0%db" % b)


def code(coder, v, b=None, wb=None):
    if coder == "bit":
        return format(v, "0%db" % b)
    return gamma(v, b) if coder == "gamma" else delta(v, b, wb)


# ---- tokens --------------------------------------------------------------------------------------------------------------------------
def lit(coder, c, b=None, wb=None):
    """lzss and repair: flag 0, the byte"""
    return "0" + code(coder, c, 8 if coder == "bit" else b, wb)


def fac(coder, dist, ln, p=0, **kw):
    """lzss: flag 1, the distance (bits_for(p) bits under bit), the length"""
    if coder == "bit":
        return "1" + code(coder, dist, bits_for(p)) + code(coder, ln, bits_for(WINDOW))
    return "1" + code(coder, dist, kw.get("db"), kw.get("dwb")) + code(coder, ln, kw.get("lb"), kw.get("lwb"))


def rule(coder, i, hi=0, b=None, wb=None):
    """repair: flag 1, the index (bits_for(hi) bits under bit)"""
    return "1" + code(coder, i, bits_for(hi) if coder == "bit" else b, wb)


def repair_head(coder):
    """one rule, ab"""
    count = format(1, "032b") if coder == "bit" else code(coder, 1)
    return count, lit(coder, 97) + lit(coder, 98)


# ---- fields at the caps ---------------------------------------------------------------------------------------------------------------
def cap_cases(decoder, coder):
    """[(name, stream, wide)], coder gamma or delta"""
    assert coder in ("gamma", "delta")
    out = []

    def add(name, bits, wide=False):
        out.append((name, terminate(bits), wide))

    if decoder == "lzss":
        pre, post = lit(coder, 97) + lit(coder, 98), lit(coder, 99)
        whole = pre + fac(coder, 1, 2) + post + fac(coder, 3, 5)
        for vb in (32, 33):
            add("distance of %d value bits" % vb, pre + fac(coder, 1, 2, db=vb) + post, vb > 32)
            add("length of %d value bits" % vb, pre + fac(coder, 1, 2, lb=vb) + post, vb > 32)
        for vb in (8, 9):
            add("literal of %d value bits" % vb, pre + lit(coder, 100, vb) + post, vb > 8)
        if coder == "delta":
            for wb in (4, 5, 6, 7):
                add("width code of %d bits, literal" % wb, pre + lit(coder, 100, 8, wb) + post, wb > 4)
                add("width code of %d bits, distance" % wb, pre + fac(coder, 1, 2, db=8, dwb=wb) + post, wb > 6)
                add("width code of %d bits, length" % wb, pre + fac(coder, 1, 2, lb=8, lwb=wb) + post, wb > 6)
        opens = (("literal", pre + "0"), ("distance", pre + "1"), ("length", pre + "1" + code(coder, 1)))
    elif decoder == "repair":
        count, sides = repair_head(coder)
        pre, post = count + sides + lit(coder, 120), lit(coder, 121)
        whole = pre + rule(coder, 0) + post + rule(coder, 0)
        for vb in (32, 33):
            add("index of %d value bits" % vb, pre + rule(coder, 0, b=vb) + post, vb > 32)
            two = code(coder, 2) + sides + rule(coder, 0, b=vb) + lit(coder, 99)       # the same field as a side of a second rule
            add("rule side of %d value bits" % vb, two + rule(coder, 1) + post, vb > 32)
        for vb in (8, 9):
            add("literal of %d value bits" % vb, pre + lit(coder, 100, vb) + post, vb > 8)
        if coder == "delta":
            for wb in (4, 5, 6, 7):
                add("width code of %d bits, literal" % wb, pre + lit(coder, 100, 8, wb) + post, wb > 6)
                add("width code of %d bits, index" % wb, pre + rule(coder, 0, b=8, wb=wb) + post, wb > 6)
        opens = (("literal", pre + "0"), ("index", pre + "1"))
    else:
        pair = decoder == "lz78"
        item = (lambda i, c, b=None: gamma(i, b) + gamma(c)) if pair else (lambda i, c, b=None: gamma(i, b))
        pre = item(0, 97) + item(1, 98) if pair else item(97, 0) + item(98, 0)
        named = 1 if pair else 256                                # phrase 1 (lz78 ids are 1-based), the first phrase (lzw)
        whole = pre + item(named, 99) + item(2 if pair else 257, 100)
        for vb in (32, 33):
            add("id of %d value bits" % vb, pre + item(named, 99, vb) + item(0 if pair else 100, 101), vb > 32)
        opens = (("id", pre),) + ((("char", pre + gamma(1)),) if pair else ())
    add("the last field ends with the stream", whole)
    add("the last field is cut one bit short", whole[:-1])
    for what, bits in opens:
        for z in (3, 63, 64, 70):
            add("%s: %d zeros up to the end" % (what, z), bits + "0" * z)
    return out


# ---- a token across the border of a tile ----------------------------------------------------------------------------------------------
def fill(target, coins):
    """token lengths out of `coins` (the first ones preferred) that sum to target, or None"""
    prev = [None] * (target + 1)
    prev[0] = 0
    for t in range(1, target + 1):
        for c in coins:
            if t >= c and prev[t - c] is not None:
                prev[t] = c
                break
    if prev[target] is None:
        return None
    out = []
    while target:
        out.append(prev[target])
        target -= prev[target]
    return out


LITERALS = (100, 200, 40, 20, 9, 5, 2, 1)     # one byte per number of value bits: literal tokens of every length


def straddle(decoder, coder, d):
    """(stream, d'): the probe token of the stream starts d' bits in front of the first tile border of a segment; d' = d, or d + 1
    where every token of the format has an even number of bits and d is out of reach.  In front of the probe: literals and the
    shortest token of the other kind, each worth one byte of text (lzss) or one item; more than 1000 of them."""
    head, base, p0 = "", 0, 0                                     # base: the bit at which the segment starts
    if decoder == "lzss":
        if coder == "bit":
            # the segments follow the text position: the one that starts at p = 4096 (bit 9 * 4096) is the first to hold a whole tile
            head = "".join(lit(coder, 97 + i % 23) for i in range(4096))
            base, p0 = len(head), 4096
        else:
            head, p0 = lit(coder, 1), 1                           # (a factor needs text in front of it)
        units = {len(lit(coder, c)): (lambda p, c=c: lit(coder, c)) for c in LITERALS}
        units[len(fac(coder, 1, 1, p0))] = lambda p: fac(coder, 1, 1, p)
        probe, tail = (lambda p: fac(coder, 1000, 15, p)), (lambda p: lit(coder, 33) + fac(coder, 2, 3, p + 16) + lit(coder, 34))
    elif decoder == "repair":
        count, sides = repair_head(coder)
        head = count + sides
        base = len(head) if coder == "bit" else len(count)        # bit: the host reads the first rules as well
        units = {len(lit(coder, c)): (lambda p, c=c: lit(coder, c)) for c in LITERALS}
        units[len(rule(coder, 0, 1))] = lambda p: rule(coder, 0, 1)
        probe, tail = (lambda p: lit(coder, 200)), (lambda p: rule(coder, 0, 1) + lit(coder, 34))
    else:
        item = (lambda i, c: gamma(i) + gamma(c)) if decoder == "lz78" else (lambda i, c: gamma(c if i is None else i))
        first = 0 if decoder == "lz78" else 255                   # lz78: id k names phrase k - 1; lzw: code 256 + k names phrase k
        units = {len(item(0 if first == 0 else None, c)): (lambda p, c=c: item(0 if first == 0 else None, c)) for c in LITERALS}
        probe, tail = (lambda p: item(first + 1000, 200)), (lambda p: item(first + 3, 33) + item(first + p, 34))
    for dd in (d, d + 1):
        lens = fill(TILE - dd - (len(head) - base), sorted(units, reverse=True))
        if lens is not None:
            break
    assert lens is not None and len(lens) > 1000                 # (the probe names item 1000, or the text 1000 bytes back)
    bits, p = head, p0
    for n in lens:
        bits += units[n](p)
        p += 1
    assert len(bits) - base == TILE - dd
    bits += probe(p) + units[max(units)](p) * 40 + tail(p + 40)   # (literals, so that the stream crosses the border for every d)
    assert len(bits) - base > TILE + 100
    return terminate(bits), dd


# ---- terminator residues --------------------------------------------------------------------------------------------------------------
def residue_streams():
    """one and two bytes; the low three bits of the last byte are 0, 5, 6, 7"""
    out = []
    for r in (0, 5, 6, 7):
        for hi in (0b00110, 0b11010, 0b01001):
            last = hi << 3 | r
            out.append(bytes([last]))
            for first in (0x00, 0x35, 0xC4, 0x4F):
                out.append(bytes([first, last]))
    return out
