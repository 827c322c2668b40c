"""The damaged repair streams of tests/test_gpu_repair_decode.py: EVERY cut (the first k payload bits, terminated anew, and the first k
bytes as they are) and EVERY single-bit flip of three short streams per coder -- the known answers `abcdcdab` and `ababab` of tests/golden/repair_kats.json and the grammar of a
text of 20 rules -- and, last, the undamaged streams.  A grammar of 20 rules expands to at most 2^20 bytes whatever one flipped bit makes
of it, and a damaged count field is refused or runs the rules into the end of the stream, so nothing here makes a decoder allocate much."""
from tests.models import repair as M
from tests.models.lzss_coders import payload_bits, terminate
from tests.util import load_json

CODERS = ("bit", "gamma", "delta")
TEXT = b"she sells sea shells by the sea shore; the shells she sells are sea shells, I'm sure. " * 2
KAT_TEXTS = ("abcdcdab", "ababab")

_cache = {}


def good_streams(coder):
    """[(name, stream, text)]"""
    if coder not in _cache:
        out = []
        for case in load_json("repair_kats.json")["cases"]:
            if case["text"] in KAT_TEXTS:
                out.append((case["text"], M.encode([tuple(r) for r in case["rules"]], case["start"], coder), case["text"].encode("latin-1")))
        rules, start = M.grammar(TEXT, 20)
        assert len(rules) == 20
        out.append(("20 rules", M.encode(rules, start, coder), TEXT))
        assert len(out) == 3
        _cache[coder] = out
    return _cache[coder]


def cut(stream, nbits):
    bits = format(int.from_bytes(stream, "big"), "0%db" % (8 * len(stream)))[:nbits]
    return terminate(bits)


def flip(stream, bit):
    b = bytearray(stream)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def damaged_streams(coder):
    """[(name, stream)]: every cut and every flip of the three streams, then the three streams themselves"""
    out = []
    for name, good, _ in good_streams(coder):
        total = payload_bits(good)
        out += [("%s cut@%d" % (name, k), cut(good, k)) for k in range(total)]
        out += [("%s bytes[:%d]" % (name, k), good[:k]) for k in range(len(good))]      # (the last byte left is read as the terminator)
        out += [("%s flip@%d" % (name, k), flip(good, k)) for k in range(total)]
    out += [(name + " good", good) for name, good, _ in good_streams(coder)]
    return out
