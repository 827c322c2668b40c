"""CPU tests of lzw: the model (tests/models/lzw.py) against the reference's known answers, the host parse (tdc_lzw_factors) and the
host decode loop (tdc_lzw_decode) against the model, the closed-form code offsets, and the model's two decoders against each other."""
import random

import numpy as np
import pytest

import tudocomp_amd as T
from tests import corpus
from tests.coder_borders import LZW_COUNTS, phrase_prefixes, residue, two_letters_64k
from tests.models import lzw as M
from tests.util import load_json

CODERS = ("bit", "gamma")
CODER_ID = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA}


def _inputs():
    rng = random.Random(11)
    out = list(corpus.small_corpus()) + list(corpus.random_small(120, 4711))
    out += [("a^%d" % n, b"a" * n) for n in (1, 2, 3, 6, 7, 500, 5000)]
    out += [("ab^%d" % n, b"ab" * n) for n in (1, 2, 3, 400, 3000)]
    out.append(("all256", bytes(range(256)) + bytes(rng.randrange(256) for _ in range(3000)) + bytes(range(255, -1, -1))))
    return out


INPUTS = _inputs()


def test_kats_model_and_host_parse():
    kats = load_json("lzw_kats.json")["lzw_codes"]
    assert len(kats) == 8
    for k in kats:
        data = bytes.fromhex(k["input_hex"])
        assert M.parse(data) == k["codes"], k["source"]
        assert T.lzw_factors(data).tolist() == k["codes"], k["source"]


def test_host_parse_equals_model():
    for name, data in INPUTS:
        assert T.lzw_factors(data).tolist() == M.parse(data), name


def test_host_parse_larger_texts():
    """table growth and the look-ahead window: 300 KB of English-like text and of DNA"""
    for data in (T.gen_english(300000, 3).tobytes(), T.gen_dna(300000, 4).tobytes()):
        assert T.lzw_factors(data).tolist() == M.parse(data)


def test_closed_form_offsets():
    s = 0
    for k in range((1 << 18) + 1):
        assert M.offset(k) == s, k
        s += M.bits_for(k + 256)
    for x in list(range(0, 5000)) + [M.offset(k) + d for k in (255, 256, 767, 768, 65279, 65280, 1 << 18) for d in (-1, 0, 1)]:
        k, w = M.code_at(x)
        assert w == M.width(k) and M.offset(k) <= x < M.offset(k + 1)


def test_widths():
    codes = [0] * 770
    assert len(M.encode(codes[:256], "bit")) == 256 * 9 // 8 + 1
    total = 256 * 9 + 512 * 10 + 2 * 11
    assert len(M.encode(codes, "bit")) == total // 8 + (1 if total % 8 <= 5 else 2)
    assert M.encode([], "bit") == b"\x00" and M.encode([], "gamma") == b"\x00"          # a constructed-and-destroyed Encoder
    assert M.encode([97], "bit") == bytes([0b00110000, 0b10000001])                      # 9 bits, then the terminator "1 bit used"


@pytest.mark.parametrize("coder", CODERS)
def test_round_trips_and_decoders_agree(coder):
    for name, data in INPUTS:
        stream = M.compress(data, coder)
        assert M.sequential_decode(stream, coder) == data, name
        assert M.decode(stream, coder) == data, name
        assert T.lzw_decode(stream, CODER_ID[coder]) == data, name


def test_fast_encoder_is_the_encoder():
    rng = random.Random(2)
    for z in (1, 7, 255, 256, 257, 767, 768, 769, 5000):
        codes = [rng.randrange(256 + k) for k in range(z)]
        for coder in CODERS:
            assert M.encode_fast(codes, coder) == M.encode(codes, coder), (z, coder)


def test_gamma_segments():
    data = corpus.fib_word(14) + b"xyz" * 50
    stream = M.compress(data, "gamma")
    for seg in (64, 257, 4096):
        assert M.decode(stream, "gamma", seg) == data


def test_kwkwk_depth():
    codes = np.array(M.parse(b"a" * 5000))
    assert (codes[1:] == 255 + np.arange(1, len(codes))).sum() >= len(codes) - 2        # every code but the last names the newest entry
    lengths, rounds = M.phrase_lengths(codes)
    assert lengths[:5].tolist() == [1, 2, 3, 4, 5] and rounds <= 8


@pytest.mark.parametrize("coder", CODERS)
def test_refusals(coder):
    cid = CODER_ID[coder]
    bad = [M.encode([256], coder), M.encode([97, 98, 259], coder), M.encode([97, 257], coder)]
    good = M.compress(b"abracadabra" * 30, coder)
    bad.append(good[:len(good) // 2 - 1] + bytes([good[len(good) // 2 - 1] & 0xF8 | (3 if coder == "bit" else 1)]))   # cut inside a code
    for s in bad:
        for dec in (M.sequential_decode, M.decode):
            with pytest.raises(M.Malformed):
                dec(s, coder)
        with pytest.raises(T.TdcGpuError) as e:
            T.lzw_decode(s, cid)
        assert e.value.status == -2
    assert M.decode(M.encode([97, 256], coder), coder) == b"aaa"                       # equality is KwKwK, not an error


def test_too_large_is_found_before_the_text_exists():
    z = 92682
    codes = np.concatenate(([97], 256 + np.arange(z - 1)))
    lengths, _ = M.phrase_lengths(codes)
    assert int(lengths.sum()) == z * (z + 1) // 2 > 2**32 - 2
    with pytest.raises(M.TooLarge):
        M.factor_list(codes, lengths)


def test_host_loop_refuses_other_coders():
    import ctypes
    s = np.frombuffer(M.encode([97, 256], "bit"), dtype=np.uint8)
    sz = ctypes.c_size_t()
    L = T._native.load()
    assert L.tdc_lzw_decode(s.ctypes.data_as(ctypes.c_void_p), len(s), T.CODER_HUFF, None, 0, ctypes.byref(sz)) == -6
    assert L.tdc_lzw_decode(s.ctypes.data_as(ctypes.c_void_p), len(s), T.CODER_BIT, None, 0, ctypes.byref(sz)) == 0 and sz.value == 3


@pytest.mark.parametrize("coder", CODERS)
def test_differential_seed_shows_something(coder):
    """the damaged streams of tests/test_gpu_lzw.py: fewer than half of them may be refused, else that test shows little"""
    from tests.lzw_damage import damaged_streams
    cases = damaged_streams(coder)
    assert len(cases) == 150
    refused = 0
    for s in cases:
        try:
            T.lzw_decode(s, CODER_ID[coder])
        except T.TdcGpuError:
            refused += 1
    assert refused * 2 < len(cases), refused
    for s in cases[:6]:                                                                  # the host loop is the model's loop
        try:
            want = M.sequential_decode(s, coder)
        except M.Malformed:
            want = None
        try:
            got = T.lzw_decode(s, CODER_ID[coder])
        except T.TdcGpuError:
            got = None
        assert got == want


def test_coder_border_inputs():
    """what tests/test_gpu_lzw.py relies on: a prefix that ends where phrase k ends parses into k codes, and the prefixes of
    tests/coder_borders.py end on both sides of the terminator rule under either coder"""
    text = two_letters_64k()
    residues = {"bit": set(), "gamma": set()}
    for k, prefix in phrase_prefixes(text, M.phrase_lengths(np.asarray(M.parse(text)))[0], LZW_COUNTS):
        assert len(M.parse(prefix)) == k
        for coder in residues:
            residues[coder].add(residue(M.compress(prefix, coder)))
    assert {5, 6} <= residues["bit"] and {5, 6} <= residues["gamma"]
