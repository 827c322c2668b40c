"""GPU tests of the device-side parse of the lcpcomp(coder=sle) token stream (pytest -m gpu; decode_text_internal,
compressors/LCPCompressor.hpp:23-76, with SLECoder::Decoder, coders/SLECoder.hpp:301-453; tests/models/sle_decode.py is the same
formulation in numpy).

A context with dec_parse = 2 parses EVERY stream on the device (the default takes streams of 1 MiB and more), under both markings
(dec_lean 1 / 0).  Whether a stream qualifies depends on its longest literal run (fdist_max <= 512: a property of the factorization,
not of the coder) and on the ranking fitting the device table (1024 ranks: what the encoder can write), so the (text, threshold,
flatten) triples whose Huffman streams are asserted to parse on the device in tests/test_gpu_decode.py must do so here for every kmer."""
import functools

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests.util import load_json, decode_sequence_case

pytestmark = pytest.mark.gpu

KMERS = (1, 3, 4, 7)
MARKINGS = ("lean", "general")


def sle(k):
    return T.CODER_SLE | (k << 8)


def _options(marking, **more):
    return dict({"dec_parse": 2, "dec_lean": 1 if marking == "lean" else 0}, **more)


@pytest.fixture(scope="module", params=MARKINGS)
def dev_ctx(request):
    """both markings of the device parse, every stream on the device"""
    ctx = T.Context(0, options=_options(request.param))
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _qualifying_text(name):
    data = {"english_3m": lambda: T.gen_english(3_000_000, 4).tobytes(), "dna_1m": lambda: T.gen_dna(1_000_000, 7).tobytes(),
            "small": lambda: b"abcabcabc hello hello abcabc", "english_3m_21": lambda: T.gen_english(3_000_000, 21).tobytes()}[name]()
    return O.escape(data)


QUALIFYING = (("english_3m", 2), ("dna_1m", 5), ("small", 2), ("english_3m_21", 2))        # (text, threshold), flatten = 1


@functools.lru_cache(maxsize=None)
def _oracle_stream(name, thr, k):
    return O.lcpcomp_sle_compress(_qualifying_text(name), thr, 1, k)[0]


@pytest.mark.parametrize("k", KMERS)
def test_qualifying_streams_parse_on_the_device(dev_ctx, gpu_ctx, k):
    """the test that fails without the device parse: device_parse == 1 for every stream, the oracle's and the device compressor's"""
    for name, thr in QUALIFYING:
        text = _qualifying_text(name)
        stream = _oracle_stream(name, thr, k)
        back, st = dev_ctx.lcpcomp_decompress(stream, sle(k))
        assert back == text, (name, k)
        assert st["device_parse"] == 1, (name, k)
        mine, cst = gpu_ctx.lcpcomp_compress(text, thr, 1, sle(k))
        back, st = dev_ctx.lcpcomp_decompress(mine, sle(k))
        assert back == text and st["device_parse"] == 1 and st["factors"] == cst["factors"], (name, k)


@pytest.mark.parametrize("k", KMERS)
def test_reference_decode_sequences_on_the_device(dev_ctx, k):
    for case in load_json("reference_kats.json")["decode_sequences"]:
        text, f = decode_sequence_case(case)
        stream, _ = O.encode_sle(text, f, k)
        back, st = dev_ctx.lcpcomp_decompress(stream, sle(k))
        assert back == text and st["device_parse"] == 1 and st["factors"] == len(f), (case["source"], k)


def _decodable(stream, text, k):
    try:
        return O.lcpcomp_sle_decompress(stream, k) == text
    except RuntimeError:
        return False


def test_small_corpus_streams_parse_on_the_device(dev_ctx):
    cases = corpus.small_corpus() + [("english_300k", T.gen_english(300_000, 9).tobytes()), ("dna_200k", T.gen_dna(200_000, 7).tobytes())]
    on_device = streams = 0
    for name, data in cases:
        text = O.escape(data)
        for thr, fl in ((1, 1), (2, 0), (2, 1), (5, 1)):
            for k in (1, 3, 7):
                stream, _ = O.lcpcomp_sle_compress(text, thr, fl, k)
                if not _decodable(stream, text, k):
                    try:
                        dev_ctx.lcpcomp_decompress(stream, sle(k))
                    except T.TdcGpuError:
                        pass
                    continue
                back, st = dev_ctx.lcpcomp_decompress(stream, sle(k))
                assert back == text, "%s t=%d flatten=%d kmer=%d" % (name, thr, fl, k)
                on_device += st["device_parse"]
                streams += 1
    print("small corpus: %d of %d sle streams parsed on the device" % (on_device, streams))
    assert on_device > len(cases)                     # (streams whose longest literal run exceeds 512 keep the host parse)


DEEP = (("english", "max_lcp", 3, 2), ("english", "plcppeaks", 3, 2), ("dna", "max_lcp", 1, 5), ("dna", "plcppeaks", 4, 5))


@pytest.mark.parametrize("kind,comp,k,thr", DEEP, ids=["%s-%s-sle%d" % c[:3] for c in DEEP])
def test_deep_unflattened_streams(dev_ctx, kind, comp, k, thr):
    """flatten = 0: source chains through earlier factors (the DEEP shapes of tests/test_gpu_variants.py)"""
    n = (3 << 20) + 4321
    data = T.gen_english(n - 1, 17).tobytes() if kind == "english" else T.gen_dna(n - 1, 19).tobytes()
    text = O.escape(data)
    stream, _ = O.lcpcomp_compress_any(text, thr, 0, "sle", comp, kmer=k)
    _, fst = O.lcpcomp_compress_any(text, thr, 1, "sle", comp, kmer=k)
    assert fst["num_flattened"] > 0 and fst["max_depth_lb"] >= 2, fst
    back, st = dev_ctx.lcpcomp_decompress(stream, sle(k))
    assert back == text and st["rounds"] >= 1
    assert O.lcpcomp_sle_decompress(stream, k) == text


@pytest.mark.parametrize("marking", MARKINGS)
def test_streams_longer_than_one_segment(marking):
    """20 000-bit segments: a 3 MB text takes hundreds of them -- the exit of one segment is the entry of the next"""
    with T.Context(0, options=_options(marking, dec_seg=20000)) as ctx:
        for name, thr in QUALIFYING[:3]:
            for k in (1, 3, 7):
                stream = _oracle_stream(name, thr, k)
                assert name == "small" or len(stream) * 8 > 50 * 20000
                back, st = ctx.lcpcomp_decompress(stream, sle(k))
                assert back == _qualifying_text(name) and st["device_parse"] == 1, (name, k)


def test_decompress_into_caller_buffer(dev_ctx, gpu_ctx):
    text = _qualifying_text("english_3m_21")
    out = T.PinnedBuffer(len(text) + 100)
    try:
        for k in (3, 7):
            stream = _oracle_stream("english_3m_21", 2, k)
            out.a[:] = 0xA5
            n, st = dev_ctx.lcpcomp_decompress_into(stream, out, sle(k))
            assert n == len(text) and out.a[:n].tobytes() == text and st["device_parse"] == 1
            assert bool((out.a[n:] == 0xA5).all())
            small = np.zeros(1000, dtype=np.uint8)
            with pytest.raises(T.TdcGpuError) as e:
                dev_ctx.lcpcomp_decompress_into(stream, small, sle(k))
            assert e.value.status == -5
        # the default context: 3 MB is above the 1 MiB rule, a tiny stream below it
        out.a[:] = 0xA5
        n, st = gpu_ctx.lcpcomp_decompress_into(_oracle_stream("english_3m_21", 2, 3), out, sle(3))
        assert n == len(text) and out.a[:n].tobytes() == text and st["device_parse"] == 1 and bool((out.a[n:] == 0xA5).all())
        tiny = _qualifying_text("small")
        n2, st2 = gpu_ctx.lcpcomp_decompress_into(_oracle_stream("small", 2, 3), out, sle(3))
        assert out.a[:n2].tobytes() == tiny and st2["device_parse"] == 0
    finally:
        out.free()


def test_default_context_takes_large_streams_only(gpu_ctx):
    """dec_parse = 1 (the default): 32 MiB of English on the device, a tiny text on the host; dec_parse = 0: the host for both"""
    data = T.gen_english(1 << 25, 42)
    text = np.concatenate([data, np.zeros(1, dtype=np.uint8)]).tobytes()
    big, cst = gpu_ctx.lcpcomp_compress(text, 2, 1, T.CODER_SLE)
    tiny_text = _qualifying_text("small")
    tiny = _oracle_stream("small", 2, 3)
    back, st = gpu_ctx.lcpcomp_decompress(big, T.CODER_SLE)
    assert back == text and st["device_parse"] == 1 and st["factors"] == cst["factors"]
    back, st = gpu_ctx.lcpcomp_decompress(tiny, T.CODER_SLE)
    assert back == tiny_text and st["device_parse"] == 0
    with T.Context(0, options={"dec_parse": 0}) as host:
        back, st = host.lcpcomp_decompress(big, T.CODER_SLE)
        assert back == text and st["device_parse"] == 0 and st["factors"] == cst["factors"]
        back, st = host.lcpcomp_decompress(tiny, T.CODER_SLE)
        assert back == tiny_text and st["device_parse"] == 0


def _outcome(ctx, stream, k):
    try:
        return ctx.lcpcomp_decompress(stream, sle(k))[0]
    except T.TdcGpuError as e:
        assert e.status in (-2, -5), e.status
        return None


@pytest.mark.parametrize("k", (1, 3, 7))
def test_damaged_streams_device_and_host_parse_agree(dev_ctx, k):
    """differential: the host parser (dec_parse = 0) is the judge of every damaged stream -- both refuse, or both return the same bytes"""
    text = O.escape(T.gen_english(20_000, 3).tobytes())
    good = O.lcpcomp_sle_compress(text, 2, 1, k)[0]
    back, st = dev_ctx.lcpcomp_decompress(good, sle(k))
    assert back == text and st["device_parse"] == 1
    rng = np.random.default_rng(5 + k)
    damaged = []
    for trial in range(150):
        bad = bytearray(good)
        bad[int(rng.integers(0, len(bad)))] ^= 1 << int(rng.integers(0, 8))       # anywhere: ranking, fields, tokens, terminator
        damaged.append(bytes(bad))
    damaged += [b"", b"\x00", good[:1000], good[:len(good) // 2] + b"\x05", good[:-1], good[:-2], good[:len(good) // 3]]
    damaged += [good[:c] for c in range(len(good) - 12, len(good) - 2)]
    refused = 0
    with T.Context(0, options={"dec_parse": 0}) as host:
        for i, bad in enumerate(damaged):
            want = _outcome(host, bad, k)
            got = _outcome(dev_ctx, bad, k)
            assert got == want, "damaged stream %d: device parse %s, host parse %s" % (
                i, "refused" if got is None else "%d bytes" % len(got), "refused" if want is None else "%d bytes" % len(want))
            refused += want is None
    assert refused > 0


def test_block_mode_round_trip(gpu_ctx):
    data = T.gen_english((5 << 20) + 12345, 8).tobytes()
    for k in (0, 1, 7):
        coder = T.CODER_SLE | (k << 8)
        blob, sts = T.blocks_compress(data, 2 << 20, 2, 1, coder=coder, devices=[0])
        assert len(sts) == 3
        assert gpu_ctx.blocks_decompress(blob, coder) == data
