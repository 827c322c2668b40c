"""Streams for the lzw / lz78 batch decoders (tudocomp_amd/csrc/lz_batch_decode.hip) and what they must yield, from code that is not under
test: tests/models/lzw.py, the host loop tdc_lzw_decode, the oracle's lz78 and tests/models/lz78_decode.py.
tests/test_lz_batch_decode_cli.py checks the expectations on the CPU, tests/test_gpu_lz_batch_decode.py runs the streams."""
import functools
import hashlib
import json
import os
import random

import numpy as np

import tudocomp_amd as T
from oracle import oracle as O
from tests import lz_batches as LB
from tests.models import lz78_decode as D
from tests.models import lzw as M

ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
ALGOS = ("lzw-bit", "lzw-gamma", "lz78")                  # (algorithm, coder) as one name
CODER_ID = {"lzw-bit": T.CODER_BIT, "lzw-gamma": T.CODER_GAMMA, "lz78": T.CODER_GAMMA}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz78_batch_damage.json")
KNOWN = (b"abcabcabcabc", b"", b"the cat sat on the mat, the cat sat")


def coder_of(algo):
    return algo.split("-")[1] if algo != "lz78" else "gamma"


def pack(streams, align=8):
    """the streams in one blob, each at a multiple of `align`, 0xEE in between: (blob, s_off, s_len)"""
    s_off, pos = [], 0
    for s in streams:
        s_off.append(pos)
        pos += -(-len(s) // align) * align if align > 1 else len(s)
    blob = np.full(max(pos, 1), 0xEE, dtype=np.uint8)
    for o, s in zip(s_off, streams):
        blob[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return blob, np.array(s_off, dtype=np.uint64), np.array([len(s) for s in streams], dtype=np.uint64)


def expected(texts, algo):
    """(streams, texts the decoder must return): the model's / the oracle's stream of every text; a text the lz78 compressor refuses has
    the stream b"" and comes back as b"" """
    if algo == "lz78":
        streams = [LB.lz78_stream(x) for x in texts]
        return streams, [b"" if LB.lz78_status(x) else x for x in texts]
    return [LB.lzw_stream(x, coder_of(algo)) for x in texts], list(texts)


def items_of(texts, algo):
    """the items all accepted streams of expected(texts, algo) hold"""
    if algo == "lz78":
        return sum(len(LB.lz78_pairs(x)[0]) for x in texts if not LB.lz78_status(x))
    return sum(len(LB.lzw_codes(x)) for x in texts)


def lz78_of(pairs):
    w = D.BitWriter()
    for ident, ch in pairs:
        w.pair(ident, ch)
    return w.finish()


def host(stream, algo):
    """(status, text) of one stream alone, by the specification: tdc_lzw_decode, or the model of LZ78Compressor::decompress"""
    if algo == "lz78":
        try:
            return 0, D.sequential_decode(stream)
        except D.Malformed:
            return ERR_ARG, b""
    try:
        return 0, T.lzw_decode(stream, CODER_ID[algo])
    except T.TdcGpuError as e:
        return e.status, b""


# ---- an item is counted from its own stream's first item ---------------------------------------------------------------------------------
GOOD = b"abcabcabcabcabcabc"


@functools.lru_cache(maxsize=None)
def own_stream_cases(algo):
    """[(streams, statuses, texts)]: a batch whose middle stream would be valid under a global item count, and the border of the rule
    on both sides"""
    if algo == "lz78":
        good = O.lz78_gamma_compress(GOOD)
        first = lz78_of([(1, 99)])                                            # the first pair names phrase 1
        late = lz78_of([(0, 97), (1, 98), (2, 99), (4, 100)])                 # pair 3 names phrase 4
        chain = [(k, 97) for k in range(700)]                                 # pair k names phrase k, the newest: a^1, a^2, ...
        newest = lz78_of(chain + [(700, 98)])
        beyond = lz78_of(chain + [(701, 98)])
        newest_text = b"".join(b"a" * (k + 1) for k in range(700)) + b"a" * 700 + b"b"
    else:
        coder = coder_of(algo)
        good = M.encode(M.parse(GOOD), coder)
        first = M.encode([256], coder)                                        # the first code names phrase 0
        late = M.encode([97, 98, 99, 259], coder)                             # code 3 names phrase 3: 255 + 3 is the most
        newest = M.encode([97] * 700 + [255 + 700], coder)                    # KwKwK: phrase 699 and its own first byte
        beyond = M.encode([97] * 700 + [256 + 700], coder)
        newest_text = b"a" * 700 + b"aa"
    return ([good, first, good], [0, ERR_ARG, 0], [GOOD, b"", GOOD]), ([good, late, good], [0, ERR_ARG, 0], [GOOD, b"", GOOD]), \
           ([good, newest, beyond, good], [0, 0, ERR_ARG, 0], [GOOD, newest_text, b"", GOOD])


# ---- claims above the format's limit -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def claim_stream(algo, z):
    """z items, each one byte longer than the one before: z (z + 1) / 2 bytes"""
    if algo == "lz78":
        bits = []                                                             # gamma(k) gamma(97) per pair, as BitWriter.pair writes them
        tail = [0] * 7 + [1] + [int(c) for c in format(97, "07b")]
        for k in range(z):
            b = max(1, k.bit_length())
            bits += [0] * b + [1] + [int(c) for c in format(k, "0%db" % b)] + tail
        w = D.BitWriter()
        w.bits = bits
        return w.finish()
    return M.encode_fast(np.concatenate(([97], 256 + np.arange(z - 1))), coder_of(algo))


OVER = 92682          # 92 682 items: 4.29e9 bytes, above 2^32 - 2 (tests/test_gpu_lzw.py::test_oversized_claim)
HALF = 65536          # 65 536 items: 2^31 + 2^15 bytes, valid alone
DEEP = 12000          # 12 000 items: 72 MB of text from some 30 KB of stream
ZEROS = 1 << 20       # lzw gamma: the code 0 is the one bit "1"


@functools.lru_cache(maxsize=None)
def zeros_stream():
    """ZEROS codes 0 under gamma as the decoder also reads them (no encoder writes a field of no value bits): 128 KiB of ones and the
    terminator, ZEROS zero bytes of text"""
    return b"\xff" * (ZEROS // 8) + b"\x00"


# ---- damage ------------------------------------------------------------------------------------------------------------------------------------
LZ78_DAMAGE_N, LZ78_DAMAGE_SEED = 197000, 5


@functools.lru_cache(maxsize=None)
def lz78_base():
    """~200 KB of oracle stream and its text"""
    data = T.gen_english(LZ78_DAMAGE_N, 77).tobytes()
    s = O.lz78_gamma_compress(data)
    assert 190000 <= len(s) <= 215000, len(s)
    return data, s


@functools.lru_cache(maxsize=None)
def lz78_damaged(count=150, seed=LZ78_DAMAGE_SEED):
    """single-bit flips and truncations of the base stream, drawn as tests/lzw_damage.py draws them"""
    _, s = lz78_base()
    rng = random.Random(seed)
    out = []
    for i in range(count):
        b = bytearray(s)
        if i % 3 == 2:                                    # a truncation: the last byte kept becomes the terminator
            del b[rng.randrange(1, len(b)):]
        else:                                             # a single bit; two thirds of them in the second half, where less depends on it
            at = rng.randrange(len(b) // 2, len(b) - 1) if i % 3 else rng.randrange(len(b) - 1)
            b[at] ^= 1 << rng.randrange(8)
        out.append(bytes(b))
    return tuple(out)


def verdict_record(stream):
    """what sequential_decode says of a stream, in the form the golden file keeps: [status, text length, sha256 of the text]"""
    rc, text = host(stream, "lz78")
    return [rc, len(text), hashlib.sha256(text).hexdigest()]


@functools.lru_cache(maxsize=None)
def lz78_damage_verdicts():
    """The verdict of models/lz78_decode.sequential_decode on every stream of lz78_damaged(), recorded (tests/golden/, made by
    `python -m tests.lz_batch_decode_cases`): the model takes half a second per stream, 150 of them more than a minute.
    tests/test_lz_batch_decode_cli.py recomputes a sample of the records on every run."""
    rec = json.load(open(GOLDEN))
    assert (rec["n"], rec["seed"], rec["count"]) == (LZ78_DAMAGE_N, LZ78_DAMAGE_SEED, len(lz78_damaged()))
    assert rec["streams_sha256"] == hashlib.sha256(b"".join(lz78_damaged())).hexdigest()
    return rec["verdicts"]


if __name__ == "__main__":
    streams = lz78_damaged()
    rec = {"n": LZ78_DAMAGE_N, "seed": LZ78_DAMAGE_SEED, "count": len(streams), "streams_sha256": hashlib.sha256(b"".join(streams)).hexdigest(),
           "verdicts": [verdict_record(s) for s in streams]}
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")
    print(sum(1 for v in rec["verdicts"] if v[0] == 0), "accepted of", len(streams))
