"""The damaged lzss streams of tests/test_lzss_sw_decode_model.py and tests/test_gpu_lzss_sw_decode.py: cuts and single-bit flips at
fixed bit indices of one model-coded stream per coder (a text of about 2 KB, window 16, threshold 3), and, last, the undamaged stream.
The indices are chosen so that no damaged stream announces a large text: every one is refused by the host loop or decodes to at most
1 MiB (the CPU test asserts it), so nothing here makes either decoder allocate much."""
from tests.models import lzss_sw as M
from tests.models.lzss_coders import payload_bits, terminate

WINDOW, THRESHOLD = 16, 3
TEXT = (b"abracadabra, said the cat; " * 30 + b"the quick brown fox jumps over the lazy dog. " * 20 + bytes(range(256)) + b"xyzzy" * 9)
TEXT_LIMIT = 1 << 20

_cache = {}


def good_stream(coder):
    if coder not in _cache:
        _cache[coder] = M.encode(M.parse(TEXT, WINDOW, THRESHOLD), coder, WINDOW)
    return _cache[coder]


def cut(stream, nbits):
    """the first nbits payload bits of the stream, terminated anew"""
    bits = format(int.from_bytes(stream, "big"), "0%db" % (8 * len(stream)))[:nbits]
    return terminate(bits)


def flip(stream, bit):
    b = bytearray(stream)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def flip_indices(coder):
    total = payload_bits(good_stream(coder))
    return list(range(5, total - 8, 263))


def cut_indices(coder):
    total = payload_bits(good_stream(coder))
    return [total - 1, total - 3, total - 11, total // 2 + 1, total // 3, 701, 70, 20, 9, 8, 1]


def damaged_streams(coder):
    """[(name, stream)]: the cuts, the flips and, last, the undamaged stream"""
    good = good_stream(coder)
    out = [("cut@%d" % k, cut(good, k)) for k in cut_indices(coder)]
    out += [("flip@%d" % k, flip(good, k)) for k in flip_indices(coder)]
    out.append(("good", good))
    return out
