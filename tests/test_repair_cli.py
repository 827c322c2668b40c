"""CPU tests of the repair interface (no GPU): the host loop tdc_repair_grammar and the host decoder tdc_repair_decode against the model
(tests/models/repair.py) on good and damaged streams, the refusals by name, and the `tdc` command line -- -d of model-made files, the
refused spellings, -l."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests.models import repair as M
from tests.models.lzss_coders import terminate
from tests.util import load_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CODER_ID = {"ascii": T.CODER_ASCII, "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
ERR_ARG, ERR_TOO_LARGE, ERR_OOM, ERR_UNSUPPORTED = -2, -4, -5, -6
DOUBLING = [(97, 97)] + [(256 + i, 256 + i) for i in range(39)]          # A_i = A_{i-1} A_{i-1}: 40 rules, 2^40 bytes


@pytest.fixture(scope="module", autouse=True)
def _built():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])


def host_grammar(data, max_rules=0):
    r, s = T.repair_grammar(data, max_rules)
    return [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in r], [int(x) for x in s]


def host_decode(stream, coder):
    """(status, text) of tdc_repair_decode"""
    try:
        return 0, T.repair_decode(stream, CODER_ID[coder])
    except T.TdcGpuError as e:
        return e.status, None


def model_decode(stream, coder):
    try:
        return 0, M.sequential_decode(stream, coder)
    except M.Malformed:
        return ERR_ARG, None
    except M.TooLarge:
        return ERR_TOO_LARGE, None


def texts():
    rng = np.random.default_rng(20261019)
    for k in range(71):
        yield b"a" * k
    for i in range(8):
        for j in range(8):
            yield b"a" * i + b"b" * j + b"a" * j
    for n in range(7):
        for t in itertools.product(b"abc", repeat=n):
            yield bytes(t)
    for sigma in (2, 4, 256):
        for n in (50, 333, 2000):
            yield rng.integers(0, sigma, n, dtype=np.uint8).tobytes()
    yield T.gen_english(4096, 5).tobytes() + b"\x00\xff" * 5


def test_symbols_and_facade():
    lib = T._native.load()
    for name in ("tdc_gpu_repair_compress", "tdc_gpu_repair_compress_into", "tdc_gpu_repair_bound", "tdc_gpu_repair_grammar",
                 "tdc_gpu_repair_decompress", "tdc_gpu_repair_decompress_into", "tdc_repair_grammar", "tdc_repair_decode"):
        assert name in T.SYMBOLS and hasattr(lib, name)
    for name in ("repair_compress", "repair_compress_into", "repair_grammar", "repair_bound", "repair_decompress", "repair_decompress_into"):
        assert hasattr(T.Context, name)
    names = T.option_names()
    assert not {"repair_recount", "repair_table_bits", "repair_log"} & set(names)      # options of the context, not enumerated


def test_host_loop_equals_the_model():
    for data in texts():
        for mr in (0, 1, 2, 7):
            assert host_grammar(data, mr) == M.grammar(data, mr), (data[:30], len(data), mr)
    for c in load_json("repair_kats.json")["cases"]:
        assert host_grammar(c["text"].encode()) == ([tuple(x) for x in c["rules"]], c["start"])
    assert host_grammar(b"") == ([], []) and host_grammar(b"q") == ([], [ord("q")])


def test_host_decode_equals_the_model_on_good_streams():
    for data in itertools.islice(texts(), 0, None, 3):
        for mr in (0, 2):
            g = M.grammar(data, mr)
            for coder in M.CODERS:
                s = M.encode(*g, coder)
                assert host_decode(s, coder) == (0, data) == model_decode(s, coder), (data[:30], mr, coder)
                assert len(s) <= T.repair_bound(len(data), CODER_ID[coder]), (data[:30], mr, coder)
    assert T.repair_bound(100, T.CODER_HUFF) == 0 and T.repair_bound((1 << 30) + 1, T.CODER_BIT) == 0
    assert T.repair_bound(1 << 30, T.CODER_BIT) > 0


@pytest.mark.parametrize("coder", M.CODERS)
def test_refusals_by_name(coder):
    enc = lambda rules, start: M.encode(rules, start, coder)
    assert host_decode(enc([(97, 98), (257, 97)], [257]), coder)[0] == ERR_ARG          # rule 1 names itself
    assert host_decode(enc([(97, 98), (97, 99), (256, 259), (97, 97)], [258]), coder)[0] == ERR_ARG   # rule 2 names rule 3
    assert host_decode(enc([(97, 98)], [256, 257]), coder)[0] == ERR_ARG                # a start symbol that names a rule >= rules
    assert host_decode(enc([], [256]), coder)[0] == ERR_ARG                             # ... with no rule at all
    bits = M.encode_bits([(97, 98)], [256, 99, 256], coder)
    for cut in (1, 3, 7):                                                               # the last field cut off
        s = terminate(bits[:-cut])
        assert model_decode(s, coder)[0] == ERR_ARG and host_decode(s, coder)[0] == ERR_ARG, cut
    big = enc(DOUBLING, [256 + 39])                                                     # 2^40 bytes: refused before any text is made
    assert host_decode(big, coder)[0] == ERR_TOO_LARGE == model_decode(big, coder)[0]
    many = [(97, 97)] + [(256 + i, 256 + i) for i in range(69)]                         # the sum saturates
    assert host_decode(enc(many, [256 + 69] * 3), coder)[0] == ERR_TOO_LARGE
    ok = enc(DOUBLING[:11], [256 + 10, 98])
    assert host_decode(ok, coder) == (0, b"a" * 2048 + b"b")


def test_self_reference_fits_its_field_under_bit():
    # Range(i) holds 0 .. 2^bits_for(i) - 1: rule 4 can name itself in three bits, and the reference would recurse for ever
    rules = [(97, 98), (256, 99), (257, 100), (258, 101), (260, 97)]
    with pytest.raises(M.Malformed, match="rule index"):
        M.sequential_decode(M.encode(rules, [260], "bit"), "bit")
    assert host_decode(M.encode(rules, [260], "bit"), "bit")[0] == ERR_ARG


def test_more_rules_than_the_stream_holds():
    assert host_decode(terminate(format(1000, "032b")), "bit")[0] == ERR_ARG
    assert host_decode(terminate(format(0xFFFFFFFF, "032b") + "0" * 64), "bit")[0] == ERR_ARG
    assert host_decode(b"4000000000:0a0a\x00", "ascii")[0] == ERR_ARG


def test_prefixes_the_field_readers_refuse():
    assert host_decode(terminate("0" * 70 + "1"), "gamma")[0] == ERR_ARG                # a unary prefix above 64
    assert host_decode(terminate("0000"), "gamma")[0] == ERR_ARG                        # ... that runs into the end
    assert host_decode(b"x:\x00", "ascii")[0] == ERR_ARG                                # an integer expected


def test_other_arguments():
    L = T._native.load()
    n = ctypes.c_size_t()
    assert L.tdc_repair_decode(None, 0, T.CODER_HUFF, None, 0, ctypes.byref(n)) == ERR_UNSUPPORTED
    assert L.tdc_repair_decode(None, 0, T.CODER_BIT, None, 0, None) == ERR_ARG
    s = np.frombuffer(M.compress(b"abcabcabc", "bit"), dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint8)
    assert L.tdc_repair_decode(s.ctypes.data, len(s), T.CODER_BIT, out.ctypes.data, 4, ctypes.byref(n)) == ERR_OOM and n.value == 9
    assert not out.any()                                                                # a buffer too small is left alone
    out = np.zeros(9, dtype=np.uint8)
    assert L.tdc_repair_decode(s.ctypes.data, len(s), T.CODER_BIT, out.ctypes.data, 9, ctypes.byref(n)) == 0 and out.tobytes() == b"abcabcabc"
    a = np.frombuffer(b"abc", dtype=np.uint8)
    assert L.tdc_repair_grammar(a.ctypes.data, 3, 0, None, None, None, None) == ERR_ARG
    assert L.tdc_gpu_repair_decompress(None, s.ctypes.data, len(s), T.CODER_BIT, None, ctypes.byref(n)) == ERR_ARG     # no context


def test_deep_grammar_needs_no_recursion():
    # rule i = (rule i - 1, 'a'): a chain as deep as there are rules
    depth = 200000
    rules = [(97, 97)] + [(256 + i, 97) for i in range(depth - 1)]
    s = M.encode(rules, [256 + depth - 1], "gamma")
    assert host_decode(s, "gamma") == (0, b"a" * (depth + 1))


HEADERS = [("repair", "bit", 0)]                                    # the bare name means coder=bit
HEADERS += [(h % c, c, mr) for c in M.CODERS for h, mr in (("repair(coder=%s)", 0), ("repair(coder=%s,max_rules=7)", 7), ("repair(%s, 2)", 2))]


@pytest.mark.parametrize("header,coder,mr", HEADERS)
def test_tdc_d_decodes_model_files(tmp_path, header, coder, mr):
    data = T.gen_english(3000, 21).tobytes() + b"\x00\xff" + b"a" * 300 + b"abc" * 50
    f = tmp_path / "p.tdc"
    f.write_bytes(header.encode() + b"%" + M.compress(data, coder, mr))
    out = tmp_path / "p.out"
    r = subprocess.run([TDC, "-d", "-o", str(out), str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == data


DAMAGED = {
    "self-reference": ([(97, 98), (257, 97)], [257]),
    "forward reference": ([(257, 97), (97, 98)], [256]),
    "start symbol out of range": ([(97, 98)], [256, 257]),
    "saturating lengths": (DOUBLING, [256 + 39, 256 + 39]),
}


@pytest.mark.parametrize("what", list(DAMAGED) + ["cut-off field"])
@pytest.mark.parametrize("coder", ["bit", "gamma"])
def test_tdc_d_refuses_damaged_streams(tmp_path, what, coder):
    if what == "cut-off field":
        stream = terminate(M.encode_bits([(97, 98)], [256, 99, 256], coder)[:-1])
    else:
        stream = M.encode(*DAMAGED[what], coder)
    f = tmp_path / "bad.tdc"
    f.write_bytes(b"repair(coder=%s)%%" % coder.encode() + stream)
    r = subprocess.run([TDC, "-d", "-o", str(tmp_path / "bad.out"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and "corrupt stream" in r.stderr, (what, r.stderr)


@pytest.mark.parametrize("algo,word", [("repair(coder=huff)", "No implementation found"), ("repair(coder=sle)", "No implementation found"),
                                       ("repair(coder=arithmetic)", "No implementation found"), ("repair(max_rules=-1)", "max_rules")])
def test_refused_spellings(tmp_path, algo, word):
    f = tmp_path / "in.txt"
    f.write_bytes(b"abc")
    r = subprocess.run([TDC, "-a", algo, "-o", str(tmp_path / "o.tdc"), str(f)], capture_output=True, text=True)
    assert r.returncode == 1 and word in r.stderr
    assert not (tmp_path / "o.tdc").exists()


def test_python_facade_refusals_and_host_loop():
    for coder in (None, "huff", "sle", "arithmetic"):
        with pytest.raises(RuntimeError, match="No implementation found"):
            T.RePairCompressor(None, coder=coder)
    with pytest.raises(RuntimeError, match="max_rules"):
        T.RePairCompressor(None, max_rules=-1)
    data = b"tobeornottobeortobeornot" * 40
    for coder in M.CODERS:
        z = T.RePairCompressor(None, coder=coder, max_rules=9)
        assert z.decompress(M.compress(data, coder, 9)) == data
    assert T.RePairCompressor(None).coder == T.CODER_BIT            # the reference's default


def test_registry_lists_repair():
    r = subprocess.run([TDC, "-l"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "repair(coder=bit | ascii | gamma | delta, max_rules=0)" in r.stdout
