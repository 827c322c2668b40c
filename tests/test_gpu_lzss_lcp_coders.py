"""GPU tests of lzss_lcp with the coders bit, gamma, delta and ascii, both directions.  The expected stream is the model's
(tests/models/lzss_coders.py; for ascii on the larger texts the oracle's ASCIICoder, which tests/test_lzss_coders_model.py pins the
model's token walk against) on the ORACLE's factor list, byte for byte; the expected text of a decompression is the input, or -- for
damaged streams -- what the host loop tdc_lzss_decode makes of the same bytes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from oracle import oracle as O
from tests import corpus
from tests import lzss_damage as D
from tests.models import lzss_coders as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CODER_ID = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA, "ascii": T.CODER_ASCII, "huff": T.CODER_HUFF}
NEW = ("bit", "gamma", "delta", "ascii")
SMALL = corpus.small_corpus()


def _factors(text, thr):
    sa = O.suffix_array(text)
    isa, phi, plcp, maxlcp = O.isa_phi_plcp(text, sa)
    return O.lzss_lcp_factorize(sa, isa, O.lcp_array(sa, plcp), thr)


def _triples(f):
    return list(zip(f["pos"].tolist(), f["src"].tolist(), f["len"].tolist()))


_big = {}


def big(name):
    """(escaped text, {coder: expected stream}) of the texts that span encoder tiles, computed once: 70 001 bytes = 35 tiles of 2048
    positions with a ragged last one; 3 MiB: streams above 1 MiB, which the default options decode on the device"""
    if name not in _big:
        gen, n, seed = {"english": (T.gen_english, 70000, 42), "dna": (T.gen_dna, 70000, 7), "english3M": (T.gen_english, (3 << 20) - 1, 9)}[name]
        text = O.escape(gen(n, seed).tobytes())
        assert len(text) == n + 1
        f = _factors(text, 3)
        want = {c: M.encode_fast(text, f, c) for c in M.CODERS}
        want["ascii"] = O.encode_ascii(text, f)[0]
        _big[name] = (text, want)
    return _big[name]


@pytest.fixture(scope="module")
def seg_ctx():
    """device parse for every stream, 4096-bit segments: the 70 001-byte streams take tens of segments and several 32 768-bit tiles"""
    ctxs = {}
    for lean in (0, 1):
        ctxs[lean] = T.Context(0, options={"dec_parse": 2, "dec_seg": 4096, "dec_lean": lean})
    yield ctxs
    for c in ctxs.values():
        c.close()


_small = []


def small_parses():
    """(name, threshold, escaped text, factor list) of the small corpus, computed once"""
    if not _small:
        for name, data in SMALL:
            text = O.escape(data)
            _small.extend((name, thr, text, _triples(_factors(text, thr))) for thr in (1, 3, 5))
    return _small


@pytest.mark.parametrize("coder", NEW)
def test_compress_small(gpu_ctx, coder):
    for name, thr, text, f in small_parses():
        got, st = gpu_ctx.lzss_lcp_compress(text, thr, CODER_ID[coder])
        assert got == M.encode(text, f, coder), (name, thr)
        assert st["factors"] == len(f) and st["out_len"] == len(got)


@pytest.mark.parametrize("coder", NEW)
@pytest.mark.parametrize("name", ("english", "dna", "english3M"))
def test_compress_tile_borders(gpu_ctx, name, coder):
    text, want = big(name)
    got, _ = gpu_ctx.lzss_lcp_compress(text, 3, CODER_ID[coder])
    assert got == want[coder]
    if name == "english3M":
        return
    n = len(text)
    src, dst = T.PinnedBuffer(n), T.PinnedBuffer(T.lzss_lcp_bound(n, CODER_ID[coder]))
    src.a[:] = np.frombuffer(text, dtype=np.uint8)
    ln, st = gpu_ctx.lzss_lcp_compress_into(src, n, dst, 3, CODER_ID[coder])
    assert dst.a[:ln].tobytes() == want[coder] and st["out_len"] == ln
    short = np.zeros(ln - 1, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.lzss_lcp_compress_into(src, n, short, 3, CODER_ID[coder])
    assert e.value.status == -5 and e.value.required == ln


def test_bound_holds(gpu_ctx):
    rng = np.random.default_rng(3)
    texts = [rng.integers(1, 255, size=6000, dtype=np.uint8).tobytes() + b"\0",       # threshold 1: factors of length 1 between literals
             b"a" * 6000 + b"\0",
             bytes(range(1, 250)) + b"\0"]                                             # no repeat: no factor, the 65-bit header fields
    for text in texts:
        for coder, cid in CODER_ID.items():
            bound = T.lzss_lcp_bound(len(text), cid)
            got, st = gpu_ctx.lzss_lcp_compress(text, 1, cid)
            assert 0 < len(got) <= bound, (coder, len(text))
            if coder in M.CODERS:
                assert got == M.encode(text, _triples(_factors(text, 1)), coder)
    assert texts[2] and gpu_ctx.lzss_lcp_compress(texts[2], 1, T.CODER_GAMMA)[1]["factors"] == 0
    for cid in (T.CODER_ARITH, T.CODER_SLE, 9):
        assert T.lzss_lcp_bound(1000, cid) == 0
        with pytest.raises(T.TdcGpuError) as e:
            gpu_ctx.lzss_lcp_compress(texts[1], 3, cid)
        assert e.value.status == -6


@pytest.mark.parametrize("lean", (0, 1))
@pytest.mark.parametrize("coder", M.CODERS)
@pytest.mark.parametrize("name", ("english", "dna"))
def test_decompress_on_the_device_in_segments(seg_ctx, name, coder, lean):
    text, want = big(name)
    got, st = seg_ctx[lean].lzss_lcp_decompress(want[coder], CODER_ID[coder])
    assert st["device_parse"] == 1 and got == text
    out = np.zeros(len(text), dtype=np.uint8)
    n, st = seg_ctx[lean].lzss_lcp_decompress_into(want[coder], out, CODER_ID[coder])
    assert n == len(text) and out.tobytes() == text and st["device_parse"] == 1


@pytest.mark.parametrize("coder", M.CODERS)
def test_decompress_default_options_take_the_device_above_1MiB(gpu_ctx, coder):
    text, want = big("english3M")
    assert len(want[coder]) > 1 << 20
    got, st = gpu_ctx.lzss_lcp_decompress(want[coder], CODER_ID[coder])
    assert st["device_parse"] == 1 and got == text
    small, _ = big("english")
    got, st = gpu_ctx.lzss_lcp_decompress(big("english")[1][coder], CODER_ID[coder])       # below 1 MiB: the host loop
    assert st["device_parse"] == 0 and got == small


def test_streams_that_keep_the_host_path(seg_ctx):
    rng = np.random.default_rng(5)
    text = rng.integers(1, 255, size=2000, dtype=np.uint8).tobytes() + b"\0"
    f = _factors(text, 3)
    assert M.header_values(len(text), _triples(f))[2] > 512                               # fdist_max above the device parse's longest run
    for coder in M.CODERS:
        got, st = seg_ctx[1].lzss_lcp_decompress(M.encode(text, _triples(f), coder), CODER_ID[coder])
        assert st["device_parse"] == 0 and got == text
    text, want = big("english")
    for coder in ("ascii", "huff"):
        stream = want["ascii"] if coder == "ascii" else O.encode_huff(text, _factors(text, 3))[0]
        got, st = seg_ctx[1].lzss_lcp_decompress(stream, CODER_ID[coder])
        assert got == text and st["device_parse"] == (0 if coder == "ascii" else 1)


@pytest.mark.parametrize("coder", M.CODERS)
def test_damaged_streams_on_the_device(seg_ctx, coder):
    ctx = seg_ctx[1]
    for name, s in D.damaged_streams(coder):
        try:
            want = T.lzss_decode(s, CODER_ID[coder])
        except T.TdcGpuError:
            want = None
        for c in (ctx, seg_ctx[0]):
            try:
                got = c.lzss_lcp_decompress(s, CODER_ID[coder])[0]
            except T.TdcGpuError as e:
                assert e.status == -2, name
                got = None
            assert got is None or got == want, name                                       # the host loop's text, or refused
            if name == "good":
                assert got == D.TEXT
    text, want = big("dna")
    got, st = ctx.lzss_lcp_decompress(want[coder], CODER_ID[coder])                        # the context is usable afterwards
    assert got == text and st["device_parse"] == 1


@pytest.mark.parametrize("coder", ("bit", "gamma", "delta", "ascii", "huff"))
def test_facade_round_trip(seg_ctx, coder):
    data = T.gen_english(30000, 5).tobytes() + b"\x00\xff\x00" + b"q" * 700
    z = T.LZSSLCPCompressor(seg_ctx[1], coder=coder, threshold=5, dec="gpu")
    stream = z.compress(data)
    assert z.decompress(stream) == data
    assert T.LZSSLCPCompressor(None, coder=coder, threshold=5).decompress(stream) == data    # the host loop reads the same stream


def test_cli_round_trip(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    data = T.gen_english(50000, 8).tobytes() + b"\x00\xff"
    f = tmp_path / "in.txt"
    f.write_bytes(data)
    algo = "lzss_lcp(coder=bit,threshold=5)"                                              # line 6 of the reference's default comparison suite
    r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "c.tdc"), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = O.escape(data)
    assert (tmp_path / "c.tdc").read_bytes() == algo.encode() + b"%" + M.encode_fast(text, _factors(text, 5), "bit")
    r = subprocess.run([TDC, "-d", "-o", str(tmp_path / "back"), str(tmp_path / "c.tdc")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "back").read_bytes() == data


def test_nothing_else_moved(gpu_ctx):
    text = O.escape(b"abracadabra" * 20)
    L = T._native.load()
    a = np.frombuffer(text, dtype=np.uint8)
    for cid in (T.CODER_BIT, T.CODER_GAMMA, T.CODER_DELTA):
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        assert L.tdc_gpu_lcpcomp_compress(gpu_ctx._h, a.ctypes.data_as(ctypes.c_void_p), len(a), 5, 1, cid, ctypes.byref(out), ctypes.byref(n), None) == -6
        assert L.tdc_gpu_lcpcomp_decompress_coder(gpu_ctx._h, a.ctypes.data_as(ctypes.c_void_p), len(a), cid, ctypes.byref(out), ctypes.byref(n), None, None) == -6
        assert T._native.load().tdc_gpu_lcpcomp_bound_coder(1000, cid) == 0
