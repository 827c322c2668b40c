"""CPU tests of the lzw / lz78 batch decoder interface (no GPU): the two symbols, the facades, the argument refusals that are decided
before the context is looked at, and the expectations tests/test_gpu_lz_batch_decode.py relies on, checked against the models."""
import ctypes

import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batch_decode_cases as C
from tests import lz_batches as LB
from tests import lzw_damage
from tests.models import lz78_decode as D
from tests.models import lzw as M

NAMES = ("tdc_gpu_lzw_decompress_batch", "tdc_gpu_lz78_decompress_batch")


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_and_facades():
    lib = T._native.load()
    for name in NAMES:
        assert name in T.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 11
    for name in ("lzw_decompress_batch", "lzw_decompress_batch_into", "lz78_decompress_batch", "lz78_decompress_batch_into"):
        assert hasattr(T.Context, name)
    assert hasattr(T.LZWCompressor, "decompress_batch") and hasattr(T.LZ78Compressor, "decompress_batch")


@pytest.mark.parametrize("name", NAMES)
def test_refusals_that_need_no_device(name):
    fn = getattr(T._native.load(), name)
    lzw = "lzw" in name
    blob = np.zeros(64, dtype=np.uint8)
    s_off, s_len = np.array([0, 8], dtype=np.uint64), np.array([3, 3], dtype=np.uint64)
    out_off, status = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.int32)

    def call(coder=T.CODER_GAMMA, count=2, **other):
        a = {"blob": ptr(blob), "s_off": ptr(s_off), "s_len": ptr(s_len), "out_off": ptr(out_off), "status": ptr(status)}
        a.update(other)
        return fn(None, a["blob"], a["s_off"], a["s_len"], count, coder, None, 0, a["out_off"], a["status"], None)

    for arg in ("blob", "s_off", "s_len", "out_off", "status"):
        assert call(**{arg: None}) == C.ERR_ARG, arg
    others = (T.CODER_HUFF, T.CODER_ASCII, T.CODER_DELTA, T.CODER_ARITH, T.CODER_SLE, 99) + (() if lzw else (T.CODER_BIT,))
    for coder in others:
        assert call(coder=coder) == C.ERR_UNSUPPORTED, coder
    wrap = np.array([3, 0xFFFFFFFFFFFFFFFE], dtype=np.uint64)                 # a stream whose end overflows
    assert call(s_off=ptr(wrap)) == C.ERR_ARG
    empty = np.array([0, 0], dtype=np.uint64)                                 # no blob is fine where no stream has a byte
    assert call(blob=None, s_len=ptr(empty)) == C.ERR_ARG == call()           # ... so both end at the NULL context
    assert call(count=0, s_off=None, s_len=None, status=None) == C.ERR_ARG    # count = 0 needs out_off alone; then the NULL context
    assert call(count=0, out_off=None) == C.ERR_ARG
    if lzw:
        assert call(coder=T.CODER_BIT) == C.ERR_ARG                           # accepted: the NULL context


@pytest.mark.parametrize("algo", C.ALGOS)
def test_own_stream_cases_against_the_models(algo):
    for streams, statuses, texts in C.own_stream_cases(algo):
        for s, rc, x in zip(streams, statuses, texts):
            assert C.host(s, algo) == (rc, x)
    if algo != "lz78":                                                        # the device formulation of the model agrees
        coder = C.coder_of(algo)
        _, newest, beyond, _ = C.own_stream_cases(algo)[2][0]
        assert M.decode(newest, coder) == b"a" * 702
        with pytest.raises(ValueError):
            M.decode(beyond, coder)


@pytest.mark.parametrize("algo", C.ALGOS)
def test_expected_streams_decode_to_their_texts(algo):
    for name in ("mixed", "ends", "one_two_bytes", "empties", "only_empties", "count0", "abab", "bytes_00_ff", "leftover_7f_80"):
        texts = LB.batch(name)
        streams, want = C.expected(texts, algo)
        for s, x in zip(streams, want):
            assert C.host(s, algo) == (0, x), name
    assert C.host(b"", algo) == (0, b"") == C.host(b"\x00", algo)             # no byte at all, and the terminator alone
    assert C.host(b"\x06", algo)[0] == C.ERR_ARG == C.host(b"\x07", algo)[0]  # a cut-off terminator


def test_the_stream_of_one_bit_codes():
    s = C.zeros_stream()
    assert len(s) == C.ZEROS // 8 + 1 and s[:-1] == b"\xff" * (C.ZEROS // 8)
    assert C.host(s, "lzw-gamma") == (0, bytes(C.ZEROS))


def test_items_of_counts_what_the_streams_hold():
    texts = LB.batch("mixed")
    assert C.items_of(texts, "lzw-bit") == C.items_of(texts, "lzw-gamma") == sum(len(M.parse(x)) for x in texts)
    streams, _ = C.expected(texts, "lz78")
    assert C.items_of(texts, "lz78") == sum(len(D.parse_pairs(s)[0]) for s in streams if s)


@pytest.mark.parametrize("algo", C.ALGOS)
def test_claims(algo):
    """z items, each one byte longer than the one before it: the small ones decode under the model, the sizes are what the names say"""
    for z in (1, 2, 50):
        assert C.host(C.claim_stream(algo, z), algo) == (0, b"".join(b"a" * (k + 1) for k in range(z)))
    assert C.OVER * (C.OVER + 1) // 2 > 2**32 - 2 >= (C.OVER - 1) * C.OVER // 2
    assert C.HALF * (C.HALF + 1) // 2 == 2**31 + 2**15 and 3 * (2**31 + 2**15) > 2**32 - 2
    if algo != "lz78":                                                        # (the lz78 model rebuilds every phrase byte by byte: too slow here)
        assert C.host(C.claim_stream(algo, C.DEEP), algo) == (0, b"a" * (C.DEEP * (C.DEEP + 1) // 2))
    if algo == "lzw-bit":                                                     # (the model reads gamma streams bit by bit: too slow here)
        codes = M.decode_codes(C.claim_stream(algo, C.HALF), C.coder_of(algo))
        assert len(codes) == C.HALF and int(codes[0]) == 97 and (np.asarray(codes[1:]) == 256 + np.arange(C.HALF - 1)).all()


@pytest.mark.parametrize("coder", ("bit", "gamma"))
def test_lzw_damage_has_both_verdicts(coder):
    algo = "lzw-" + coder
    data, base = lzw_damage.base_stream(coder)
    assert C.host(base, algo) == (0, data)
    verdicts = [C.host(s, algo)[0] for s in lzw_damage.damaged_streams(coder)]
    assert len(verdicts) == 150 and set(verdicts) <= {0, C.ERR_ARG} and verdicts.count(C.ERR_ARG) >= 10
    assert coder == "bit" or verdicts.count(0) >= 10                          # (bit: nearly every flip makes a code too large or cuts one)


def test_lz78_damage_record_is_the_models():
    """the recorded verdicts are sequential_decode's: the record fits the streams (their hash), both verdicts occur, and a sample of the
    records -- a flip anywhere, two flips in the second half, three truncations, and a refused stream of every kind drawn -- is computed
    again here"""
    data, base = C.lz78_base()
    streams, rec = C.lz78_damaged(), C.lz78_damage_verdicts()
    assert len(streams) == len(rec) == 150
    status = [v[0] for v in rec]
    assert set(status) <= {0, C.ERR_ARG} and status.count(0) >= 10 and status.count(C.ERR_ARG) >= 10
    assert all(v[1] <= 2 * len(data) for v in rec)                            # no stream claims a text near the format's limit: one kind of defect
    sample = {0, 1, 2, 76, 149}
    sample |= {next(k for k in range(150) if k % 3 == r and status[k] == C.ERR_ARG) for r in range(3) if any(status[k] for k in range(r, 150, 3))}
    for k in sorted(sample):
        assert C.verdict_record(streams[k]) == rec[k], k
