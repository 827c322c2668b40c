"""CPU tests of the universal coders of lzss_lcp (bit, gamma, delta): the model (tests/models/lzss_coders.py) pinned by hand-derived
bit strings and by what the oracle already writes (its gamma stream of lz78, its ASCIICoder and HuffmanCoder streams of the same token
walk), the model's two encoders and its decoder against each other, and the host loop tdc_lzss_decode against the model on good and
damaged streams."""
import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests import lzss_damage as D
from tests.models import lzss_coders as M
from tests.util import load_json, factors_struct

CODER_ID = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
SMALL = corpus.small_corpus()


def _bits(stream):
    return format(int.from_bytes(stream, "big"), "0%db" % (8 * len(stream)))[:M.payload_bits(stream)]


def _parses():
    """(name, escaped text, factor list) of the small corpus at thresholds 1, 3 and 5: the oracle's greedy parse"""
    out = []
    for name, data in SMALL:
        text = O.escape(data)
        sa = O.suffix_array(text)
        isa, phi, plcp, maxlcp = O.isa_phi_plcp(text, sa)
        lcp = O.lcp_array(sa, plcp)
        for thr in (1, 3, 5):
            out.append(("%s t=%d" % (name, thr), text, O.lzss_lcp_factorize(sa, isa, lcp, thr)))
    return out


@pytest.fixture(scope="module")
def parses():
    return _parses()


def _triples(f):
    return list(zip(f["pos"].tolist(), f["src"].tolist(), f["len"].tolist()))


def test_hand_derived_bit_strings():
    k = load_json("lzss_coder_kats.json")
    text, factors = bytes.fromhex(k["text_hex"]), [tuple(f) for f in k["factors"]]
    assert set(k["payload_bits"]) == set(M.CODERS)
    for coder, want in k["payload_bits"].items():
        assert M.encode_bits(text, factors, coder) == want, coder
        assert _bits(M.encode(text, factors, coder)) == want, coder


def test_gamma_writer_is_the_oracles():
    """the model's gamma code, on the (id, char) pairs of lz78: the stream the oracle writes for lz78(coder=gamma)"""
    for data in (b"abracadabra", b"a" * 300, b"tobeornottobeortobeornot" * 9, corpus.fib_word(12), bytes(range(1, 120)) * 2):
        ids, chars = O.lz78_factors(data)
        s = M.Sink()
        w = M.GammaWriter(s)
        for i, c in zip(ids.tolist(), chars):
            w.code(i)
            w.code(c)
        assert M.terminate(s.bits()) == O.lz78_gamma_compress(data), data[:16]


def test_token_walk_is_the_oracles(parses):
    """the walk rendered with an ASCII field writer: the oracle's lzss::encode_text with ASCIICoder"""
    for name, text, f in parses:
        assert M.encode(text, _triples(f), "ascii") == O.encode_ascii(text, f)[0], name


def test_bit_stream_is_the_raw_literal_huffman_stream():
    """one distinct literal: HuffmanCoder writes a 0 bit and then what BitCoder writes"""
    for m in (2, 9, 300, 70000):
        text = b"a" * m + b"\0"
        factors = [(0, 1, m - 1), (m - 1, 0, 1)]
        huff = O.encode_huff(text, factors_struct(*zip(*factors)))[0]
        assert _bits(huff)[0] == "0" and _bits(huff)[1:] == M.encode_bits(text, factors, "bit"), m


@pytest.mark.parametrize("coder", M.CODERS)
def test_fast_encoder_is_the_encoder(parses, coder):
    for name, text, f in parses:
        assert M.encode_fast(text, f, coder) == M.encode(text, _triples(f), coder), name


@pytest.mark.parametrize("coder", M.CODERS)
def test_model_round_trips(parses, coder):
    for name, text, f in parses:
        assert M.decode(M.encode(text, _triples(f), coder), coder) == text, name
    for text in (b"\0", b"a\0", b"abcdefgh\0"):                                            # the one-byte text; texts without a factor
        assert M.decode(M.encode(text, [], coder), coder) == text
    zero = M.encode_bits(b"ab\0", [], "gamma")
    assert len(zero) == 5 + 65 + 3 + 5 + 1 + 5 + 15 + 15 + 3 and zero[5:70] == '0' * 32 + '1' * 33   # flen_min = 2^32 - 1 takes 65 bits


@pytest.mark.parametrize("coder", M.CODERS)
def test_host_loop_decodes_what_the_model_writes(parses, coder):
    for name, text, f in parses:
        assert T.lzss_decode(M.encode(text, _triples(f), coder), CODER_ID[coder]) == text, name
    for text in (b"\0", b"a\0", b"abcdefgh\0"):
        assert T.lzss_decode(M.encode(text, [], coder), CODER_ID[coder]) == text


@pytest.mark.parametrize("coder", M.CODERS)
def test_host_loop_and_model_agree_on_damaged_streams(coder):
    cases = D.damaged_streams(coder)
    assert len(cases) == 13
    refused = 0
    for name, s in cases:
        try:
            want = M.decode(s, coder)
        except M.Malformed:
            want = None
        try:
            got = T.lzss_decode(s, CODER_ID[coder])
        except T.TdcGpuError as e:
            assert e.status == -2, name
            got = None
        assert got == want, name
        refused += want is None
    assert cases[-1][0] == "good" and T.lzss_decode(cases[-1][1], CODER_ID[coder]) == D.TEXT
    assert 3 <= refused <= 12                                                              # both verdicts occur


def test_host_loop_serves_huff_and_ascii_and_refuses_the_rest(parses):
    name, text, f = parses[20]
    assert T.lzss_decode(O.encode_huff(text, f)[0], T.CODER_HUFF) == text
    assert T.lzss_decode(O.encode_ascii(text, f)[0], T.CODER_ASCII) == text
    for coder in (T.CODER_ARITH, T.CODER_SLE, 7):
        with pytest.raises(T.TdcGpuError) as e:
            T.lzss_decode(b"\0", coder)
        assert e.value.status == -6
