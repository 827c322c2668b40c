"""GPU tests of the device decoder of repair streams (tdc_gpu_repair_decompress{,_into,_stats}; repair_decode.hip): bit, gamma and delta
streams of the device compressor back to their texts with small and with default segments, hand-built grammars around rule counts 2^k
under bit, the smallest streams, deep and far-expanding grammars, the refusals, damaged streams against the host loop's verdict
(tdc_repair_decode), the path option dec_parse picks, the facade and the `tdc` round trip."""
import functools
import os
import subprocess

import numpy as np
import pytest

import tudocomp_amd as T
from tests import repair_damage as D
from tests.models import repair as M
from tests.models.lzss_coders import payload_bits

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_TOO_LARGE, ERR_OOM = -2, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDC = os.path.join(ROOT, "tudocomp_amd", "bin", "tdc")
CID = {"ascii": T.CODER_ASCII, "bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
CODERS = ("bit", "gamma", "delta")
N = 70001
DOUBLING = [(97, 97)] + [(M.SIGMA + i - 1, M.SIGMA + i - 1) for i in range(1, 40)]


@pytest.fixture(scope="module")
def seg_ctx():
    """every stream on the device, in segments of 4096 bit positions"""
    with T.Context(0, options={"dec_parse": 2, "dec_seg": 4096}) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def dev_ctx():
    """every stream on the device, default segments"""
    with T.Context(0, options={"dec_parse": 2}) as ctx:
        yield ctx


@pytest.fixture(params=["seg", "dev"])
def ctx(request, seg_ctx, dev_ctx):
    return seg_ctx if request.param == "seg" else dev_ctx


@functools.lru_cache(maxsize=None)
def text(kind, n=N):
    return (T.gen_english(n, 42) if kind == "english" else T.gen_dna(n, 42)).tobytes()


def device(c, stream, coder):
    """(status, text, stats) of tdc_gpu_repair_decompress_stats"""
    try:
        out, st = c.repair_decompress_stats(stream, CID[coder])
        return 0, out, st
    except T.TdcGpuError as e:
        return e.status, None, None


def verdict(f):
    try:
        return 0, f()
    except T.TdcGpuError as e:
        return e.status, None


def host(stream, coder):
    return verdict(lambda: T.repair_decode(stream, CID[coder]))


def expand(rules, start):
    memo = []
    for l, r in rules:
        memo.append((bytes([l]) if l < M.SIGMA else memo[l - M.SIGMA]) + (bytes([r]) if r < M.SIGMA else memo[r - M.SIGMA]))
    return b"".join(bytes([x]) if x < M.SIGMA else memo[x - M.SIGMA] for x in start)


@pytest.mark.parametrize("max_rules", [0, 1, 64, 512])
@pytest.mark.parametrize("kind", ["english", "dna"])
def test_round_trips(seg_ctx, dev_ctx, kind, max_rules):
    data = text(kind)
    for coder in CODERS:
        stream, cst = dev_ctx.repair_compress(data, max_rules, CID[coder])
        for c in (seg_ctx, dev_ctx):
            status, out, st = device(c, stream, coder)
            assert status == 0 and st["device_parse"] == 1
            assert out == data, (kind, coder, max_rules)
            assert st["rules"] == cst["rules"] and st["n"] == len(data)
            assert st["len_rounds"] >= 1 and st["levels"] >= 1 and st["small_levels"] >= 1
            assert st["factors"] > 0 and st["flatten_rounds"] >= 1
            buf = np.full(len(data), 0xA5, dtype=np.uint8)
            n, st2 = c.repair_decompress_stats_into(stream, buf, CID[coder])
            assert n == len(data) and buf.tobytes() == data and st2["factors"] == st["factors"] and st2["device_parse"] == 1
            buf[:] = 0xA5
            assert c.repair_decompress_into(stream, buf, CID[coder]) == len(data) and buf.tobytes() == data
            short = np.full(len(data) - 1, 0xA5, dtype=np.uint8)
            with pytest.raises(T.TdcGpuError) as e:
                c.repair_decompress_stats_into(stream, short, CID[coder])
            assert e.value.status == ERR_OOM and e.value.required == len(data) and (short == 0xA5).all()
        assert seg_ctx.repair_decompress(stream, CID[coder]) == data


def pow2_grammar(nrules):
    """rule i is two bytes or an earlier rule and a byte (expansions stay short); the start sequence names every rule, the last one first"""
    rules = [(97 + i % 5, 98 + i % 7) if i < 2 or i % 3 == 0 else (M.SIGMA + (i * 7919) % i, 99 + i % 11) for i in range(nrules)]
    start = [M.SIGMA + nrules - 1, 33] + [M.SIGMA + i for i in range(nrules)] + [34]
    return rules, start


@pytest.mark.parametrize("k", range(1, 14))
def test_power_of_two_rule_counts_under_bit(dev_ctx, k):
    for nrules in ((1 << k) - 1, 1 << k, (1 << k) + 1):
        rules, start = pow2_grammar(nrules)
        want = expand(rules, start)
        assert len(want) < 1 << 20
        status, out, st = device(dev_ctx, M.encode(rules, start, "bit"), "bit")
        assert status == 0 and st["device_parse"] == 1 and st["rules"] == nrules
        assert out == want, nrules


@pytest.mark.parametrize("coder", CODERS)
def test_smallest_streams(ctx, coder):
    def check(rules, start, want):
        s = M.encode(rules, start, coder)
        assert host(s, coder) == (0, want)
        status, out, st = device(ctx, s, coder)
        assert (status, out) == (0, want) and st["device_parse"] == 1 and st["rules"] == len(rules)
        return st
    # no byte at all: the count field is cut off, for the host loop and for the device
    assert verdict(lambda: ctx.repair_decompress(b"", CID[coder])) == host(b"", coder) == (ERR_ARG, None)
    check([], [], b"")                                            # the empty grammar: the count field and the terminator
    assert check([], [113], b"q")["factors"] == 0
    assert check([], list(b"literals only, no rules \x00\xff"), b"literals only, no rules \x00\xff")["factors"] == 0
    three = [(97, 98), (M.SIGMA, 99), (M.SIGMA + 1, M.SIGMA)]
    assert check(three, [M.SIGMA + 2], b"abcab")["factors"] == 1  # the second ab
    check(three, [], b"")
    st = check(three, [120, 121], b"xy")                          # rules none of which the start sequence uses
    assert st["factors"] == 0
    run = b"a" * 5000
    st = check(*M.grammar(run), run)
    assert st["factors"] >= 1 and st["flatten_rounds"] >= 1


def chain(n):
    return [(97, 98)] + [(M.SIGMA + i - 1, 98) for i in range(1, n)]


@pytest.mark.parametrize("coder", CODERS)
def test_depth(dev_ctx, coder):
    want = b"a" + b"b" * 300 + b"c"
    s = M.encode(chain(300), [M.SIGMA + 299, 99], coder)
    status, out, st = device(dev_ctx, s, coder)
    assert (status, out) == (0, want) and st["device_parse"] == 1
    assert 2 <= st["len_rounds"] <= 301 and 2 <= st["levels"] <= 301
    with T.Context(0, options={"dec_parse": 2, "repair_dec_rounds": 16}) as capped:
        status, out, st = device(capped, s, coder)
        assert (status, out) == (0, want) and st["device_parse"] == 0          # deeper than the cap: the host loop, and the call says so
        status, out, st = device(capped, M.encode(chain(10), [M.SIGMA + 9], coder), coder)
        assert (status, out) == (0, b"a" + b"b" * 10) and st["device_parse"] == 1


def test_expansion_through_a_larger_arena():
    """26 doubling rules in a stream of some dozen bytes: the text pass does not fit the arena the parse took"""
    n = 1 << 26
    with T.Context(0, options={"dec_parse": 2}) as fresh:         # a fresh context: its arena starts empty
        status, out, st = device(fresh, M.encode(DOUBLING[:26], [M.SIGMA + 25], "gamma"), "gamma")
        assert status == 0 and st["device_parse"] == 1 and st["rules"] == 26 and st["n"] == n
        assert len(out) == n and out == b"a" * n
        assert st["factors"] == 25                                # the second half of every rule but the first, which is two bytes
        assert device(fresh, M.encode([], [113], "gamma"), "gamma")[:2] == (0, b"q")


@pytest.mark.parametrize("coder", CODERS)
def test_expansion_limits(dev_ctx, coder):
    big = M.encode(DOUBLING, [M.SIGMA + 39], coder)               # 2^40 bytes: refused before any text is made
    assert device(dev_ctx, big, coder)[0] == ERR_TOO_LARGE and host(big, coder)[0] == ERR_TOO_LARGE
    buf = np.zeros(16, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        dev_ctx.repair_decompress_stats_into(big, buf, CID[coder])
    assert e.value.status == ERR_TOO_LARGE
    status, out, st = device(dev_ctx, M.encode(DOUBLING, [97], coder), coder)      # unused rules whose lengths saturate
    assert (status, out) == (0, b"a") and st["device_parse"] == 1


def test_refusals_by_name(dev_ctx):
    def refused(s, coder):
        assert host(s, coder)[0] == ERR_ARG
        assert verdict(lambda: dev_ctx.repair_decompress(s, CID[coder]))[0] == ERR_ARG
        assert device(dev_ctx, s, coder)[0] == ERR_ARG
    for i in (4, 8192):                                           # rule i naming itself, at a power of two: bits_for(i) bits hold i
        rules = [(97, 98)] * i + [(M.SIGMA + i, 99)]
        refused(M.encode(rules, [M.SIGMA + i], "bit"), "bit")
    refused(M.encode([(M.SIGMA + 1, 97), (98, 99)], [M.SIGMA], "gamma"), "gamma")          # a forward reference
    for coder in CODERS:
        refused(M.encode([(97, 98), (M.SIGMA, 99)], [M.SIGMA + 1, M.SIGMA + 2], coder), coder)     # a start symbol equal to `rules`
        good = M.encode([(97, 98), (M.SIGMA, 99)], [M.SIGMA + 1, 100], coder)
        assert device(dev_ctx, good, coder)[:2] == (0, b"abcd")
        refused(D.cut(good, payload_bits(good) - 1), coder)      # a cut-off last field
    bits = M.encode_bits([(97, 98)], [M.SIGMA], "bit")
    nbytes = len(M.terminate(bits))
    assert host(M.terminate(format(2 * nbytes, "032b") + bits[32:]), "bit")[0] == ERR_ARG   # (2 * len rules pass the count check and run into the end)
    refused(M.terminate(format(2 * nbytes + 1, "032b") + bits[32:]), "bit")                 # a count above 2 * len
    assert device(dev_ctx, M.encode([(97, 98)], [M.SIGMA], "bit"), "bit")[:2] == (0, b"ab")  # the context is usable afterwards


@pytest.mark.parametrize("coder", CODERS)
def test_damaged_streams_get_the_host_loops_verdict(ctx, coder):
    for name, s in D.damaged_streams(coder):
        want = host(s, coder)
        got = verdict(lambda: ctx.repair_decompress(s, CID[coder]))
        assert got == want, (name, got[0], want[0])
    for name, s, data in D.good_streams(coder):                   # ... and the good streams afterwards, on the device
        assert device(ctx, s, coder)[:2] == (0, data)


def test_dec_parse_picks_the_path(gpu_ctx):
    small = text("english")
    data = text("english", 2 << 20)
    for coder in CODERS:
        s, _ = gpu_ctx.repair_compress(small, 64, CID[coder])
        out, st = gpu_ctx.repair_decompress_stats(s, CID[coder])  # the default: small streams stay on the host
        assert out == small and st["device_parse"] == 0 and st["rules"] == 0
        stream, cst = gpu_ctx.repair_compress(data, 64, CID[coder])
        assert len(stream) >= 1 << 20
        out, st = gpu_ctx.repair_decompress_stats(stream, CID[coder])
        assert out == data and st["device_parse"] == 1 and st["rules"] == cst["rules"] == 64
    with T.Context(0, options={"dec_parse": 0}) as off:
        out, st = off.repair_decompress_stats(stream, CID["delta"])
        assert out == data and st["device_parse"] == 0
    s, _ = gpu_ctx.repair_compress(data, 64, T.CODER_ASCII)       # ascii keeps the host loop whatever the size
    out, st = gpu_ctx.repair_decompress_stats(s, T.CODER_ASCII)
    assert len(s) >= 1 << 20 and out == data and st["device_parse"] == 0


def test_facade_and_command_line(dev_ctx, tmp_path):
    data = text("english", 30000) + b"\x00\xff" + b"a" * 300
    for coder in CODERS + ("ascii",):
        z = T.RePairCompressor(dev_ctx, coder, max_rules=200, dec="gpu")
        s = z.compress(data)
        assert z.decompress(s) == data
        assert T.RePairCompressor(None, coder).decompress(s) == data
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tudocomp_amd", "host")])
    src = tmp_path / "in.txt"
    src.write_bytes(data)
    # (the file is small: every stream on the device, and the decoder's log says that it ran)
    env = dict(os.environ, TDC_GPU_DEBUG_KNOBS="1", TDC_GPU_DEC_PARSE="2", TDC_GPU_DEC_LOG="1")
    payloads = []
    for algo in ("repair(coder=bit,dec=gpu)", "repair(coder=bit)", "repair(coder=ascii,dec=gpu)"):
        packed, back = tmp_path / "p.tdc", tmp_path / "p.out"
        r = subprocess.run([TDC, "-a", algo, "-f", "-o", str(packed), str(src)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        blob = packed.read_bytes()
        assert blob.startswith(algo.encode() + b"%")              # the header is written as given
        payloads.append(blob[len(algo) + 1:])
        r = subprocess.run([TDC, "-d", "-f", "-o", str(back), str(packed)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        assert back.read_bytes() == data
        assert ("repair decode:" in r.stderr) == (algo == "repair(coder=bit,dec=gpu)")      # ascii with dec=gpu: the host loop
    assert payloads[0] == payloads[1]
