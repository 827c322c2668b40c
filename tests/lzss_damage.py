"""The damaged lzss_lcp streams of tests/test_lzss_coders_model.py and tests/test_gpu_lzss_lcp_coders.py: a dozen per coder, made
from one model-coded stream -- cuts inside a field, flipped bits (under gamma / delta the first ones sit in unary prefixes), and
factor lists whose sources or lengths leave the text."""
from tests.models import lzss_coders as M

TEXT = (b"abracadabra, said the cat; " * 40 + b"the quick brown fox " * 25 + b"xyzzy") + b"\0"


def factors():
    """a valid factor list (not the greedy parse: any list that copies equal bytes from earlier positions will do)"""
    f, p, n = [], 60, len(TEXT)
    while p + 12 < n:
        src = TEXT.find(TEXT[p:p + 9])
        if 0 <= src < p:
            ln = 9
            while p + ln < n - 1 and ln < 40 and TEXT[src + ln] == TEXT[p + ln]:
                ln += 1
            f.append((p, src, ln))
            p += ln + (3 if len(f) % 4 == 0 else 0)
        else:
            p += 1
    return f


def cut(stream, nbits):
    """the first nbits payload bits of the stream, terminated anew"""
    bits = format(int.from_bytes(stream, "big"), "0%db" % (8 * len(stream)))[:nbits]
    return M.terminate(bits)


def flip(stream, bit):
    b = bytearray(stream)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def damaged_streams(coder):
    """[(name, stream)]: twelve damaged streams and, last, the undamaged one"""
    f = factors()
    good = M.encode(TEXT, f, coder)
    total = M.payload_bits(good)
    n = len(TEXT)
    out = [("cut@%d" % k, cut(good, k)) for k in (total - 3, total - 11, total // 2 + 1, total // 3, 70, 20)]
    # bits 0 and 5: the header's first field, n -- under gamma / delta inside its unary prefix, under bit beyond what a text may have
    # or a small change of n (bit 27); no flip that would announce a text of hundreds of megabytes
    out += [("flip@%d" % k, flip(good, k)) for k in (0, 5 if coder != "bit" else 27, 33, total // 2, total - 9)]
    bad = list(f)
    bad[len(bad) // 2] = (bad[len(bad) // 2][0], n - 3, bad[len(bad) // 2][2])                 # src + len > n
    out.append(("src+len>n", M.encode(TEXT, bad, coder)))
    out.append(("good", good))
    return out
