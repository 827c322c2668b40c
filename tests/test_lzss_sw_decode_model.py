"""CPU tests of the executable model of the device decoder of lzss streams (tests/models/lzss_sw_decode.py) against the sequential model
of the host loop (tests/models/lzss_sw.py decode): good streams of all three coders at every segment size, hand-built bit token lists
around text position 2^k, the refusals, text_length, and the damaged streams the GPU test feeds to the device (held against tdc_lzss_sw_decode too)."""
import pytest

import tudocomp_amd as T

from tests import lzss_sw_damage as D
from tests.models import lzss_sw as M
from tests.models import lzss_sw_decode as MD
from tests.models.lzss_coders import terminate

CID = {"bit": T.CODER_BIT, "gamma": T.CODER_GAMMA, "delta": T.CODER_DELTA}
SEGS = (64, 65, 100, 257, 1 << 30)


def verdict(f, *a, **kw):
    try:
        return 0, f(*a, **kw)
    except MD.Malformed:
        return -2, None
    except MD.TooLarge:
        return -4, None


@pytest.mark.parametrize("coder", MD.CODERS)
def test_model_equals_the_host_loop_on_sweep_streams(coder):
    for i, (data, w, t) in enumerate(M.sweep(20261020, 420)):
        s = M.encode(M.parse(data, w, t), coder, w)
        want = verdict(M.decode, s, coder, w)
        assert want[0] == 0 or (coder == "bit" and M.truncates(data, w, t))      # (a truncated length may make the stream malformed)
        seg = SEGS[i % len(SEGS)]
        for pad in (0, 4096):
            st = {}
            assert verdict(MD.decode, s, coder, w, seg=seg, pad=pad, stats=st) == want, (data, w, t, coder, seg, pad)
            if want[0] == 0 and s != terminate(""):
                assert st["segments"] >= 1 and st["evaluated"] >= 1
        if want[0]:
            assert verdict(MD.text_length, s, coder, w)[0] == want[0]
            continue
        assert MD.text_length(s, coder, w) == len(want[1])
        if not (coder == "bit" and M.truncates(data, w, t)):
            assert MD.factor_tokens(s, coder, w) == sum(1 for tok in M.parse(data, w, t) if tok[1] is not None)
        assert not MD.over_cap(s, coder, w)
        if not (coder == "bit" and M.truncates(data, w, t)):
            assert want[1] == data


@pytest.mark.parametrize("k", range(3, 13))
@pytest.mark.parametrize("case", MD.BOUNDARY_CASES)
def test_bit_tokens_around_a_power_of_two(case, k):
    toks = MD.boundary_tokens(case, [k])
    text = MD.text_of(toks)
    assert len(text) > (1 << k)
    s = M.encode(toks, "bit", 16)
    assert M.decode(s, "bit", 16) == text
    for seg, pad in ((1 << 30, 4096), (1 << 30, 0), (64, 0), (1000, 7)):
        st = {}
        assert MD.decode(s, "bit", 16, seg=seg, pad=pad, stats=st) == text, (case, k, seg, pad)
        assert st["segments"] >= k                                   # one stretch per width at least
    assert MD.text_length(s, "bit", 16) == len(text)


def test_bit_tokens_around_several_powers_of_two():
    for case in MD.BOUNDARY_CASES:
        toks = MD.boundary_tokens(case, range(3, 11), n=1500)
        text = MD.text_of(toks)
        s = M.encode(toks, "bit", 4096)
        assert M.decode(s, "bit", 4096) == text == MD.decode(s, "bit", 4096, seg=512)


@pytest.mark.parametrize("coder", MD.CODERS)
def test_refusals(coder):
    enc = lambda toks, w=16: M.encode(toks, coder, w)
    dec = lambda s, **kw: verdict(MD.decode, s, coder, 16, **kw)
    for seg in (64, 1 << 30):
        assert dec(enc([(0, None, 97), (1, 1, 2)]), seg=seg)[0] == -2                   # distance 0
        if coder != "bit":                                                              # (bit: bits_for(1) = 1 bit holds 0 or 1)
            assert dec(enc([(0, None, 97), (1, -1, 2)]), seg=seg)[0] == -2              # distance 2 above a text of 1
        assert dec(enc([(0, 0, 3)]), seg=seg)[0] == -2                                  # a factor in front of any text
        bits = M.encode_bits([(0, None, 97), (1, 0, 5), (6, None, 98)], coder, 16)
        for cut in (1, 3, 7):                                                           # the last token cut off
            assert dec(terminate(bits[:-cut]), seg=seg)[0] == -2
        assert dec(enc([(0, None, 97), (1, 0, 0), (1, None, 98)]), seg=seg) == (0, b"ab")   # length 0 decodes to nothing
    assert dec(b"") == (0, b"") and dec(terminate("")) == (0, b"")
    if coder != "bit":
        big = enc([(0, None, 97)] + [(1 + (i << 31), (i << 31), 1 << 31) for i in range(3)])
        assert dec(big)[0] == -4 and verdict(MD.text_length, big, coder, 16)[0] == -4   # 1 + 3 * 2^31 bytes: judged from the scan's total
        assert not MD.over_cap(big, coder)


def test_fields_above_the_device_caps():
    """gamma / delta fields the host loop reads and the device refuses: the one licensed difference"""
    lit9 = terminate("0" + "0" * 9 + "1" + "1" + "0" * 8)                               # a literal code of 9 value bits: the byte 0
    assert verdict(M.decode, lit9, "gamma", 16) == (0, b"\x00")
    assert verdict(MD.decode, lit9, "gamma", 16)[0] == -2 and MD.over_cap(lit9, "gamma")
    len33 = terminate("0" + "01" + "1" + "1" + "01" + "1" + "0" * 33 + "1" + "0" * 32 + "1")    # the byte 1, then (dist 1, len 1 in 33 bits)
    assert verdict(M.decode, len33, "gamma", 16) == (0, b"\x01\x01")
    assert verdict(MD.decode, len33, "gamma", 16)[0] == -2 and MD.over_cap(len33, "gamma")
    wide = terminate("0" + "00001" + "1001" + "0" * 8 + "1")                            # delta: width 9 for a literal
    assert verdict(M.decode, wide, "delta", 16) == (0, b"\x01")
    assert verdict(MD.decode, wide, "delta", 16)[0] == -2 and MD.over_cap(wide, "delta")
    assert verdict(MD.decode, terminate("1" + "0" * 70 + "1"), "gamma", 16)[0] == -2    # both refuse: a unary prefix above 64
    assert not MD.over_cap(terminate("1" + "0" * 70 + "1"), "gamma")


@pytest.mark.parametrize("coder", MD.CODERS)
def test_damaged_streams(coder):
    streams = D.damaged_streams(coder)
    assert streams[-1][0] == "good" and verdict(MD.decode, streams[-1][1], coder, D.WINDOW) == (0, D.TEXT)
    licensed = checked = 0
    verdicts = set()
    for name, s in streams:
        host = verdict(M.decode, s, coder, D.WINDOW)
        try:                                                            # the host loop itself, tdc_lzss_sw_decode: the same verdict
            real = 0, T.lzss_sw_decode(s, CID[coder], D.WINDOW)
        except T.TdcGpuError as e:
            real = e.status, None
        assert real == host, name
        n = verdict(MD.text_length, s, coder, D.WINDOW)
        assert n[0] == host[0] and (host[0] or n[1] == len(host[1])), name
        assert host[0] != 0 or n[1] <= D.TEXT_LIMIT, name               # nothing that announces a large text reaches a decoder
        verdicts.add(host[0])
        if MD.over_cap(s, coder, D.WINDOW):
            licensed += 1
            assert coder != "bit"
            continue
        checked += 1
        for seg in (4096, 1 << 30) if checked % 4 == 0 or name == "good" else (4096,):
            assert verdict(MD.decode, s, coder, D.WINDOW, seg=seg) == host, (name, seg)
    assert {0, -2} <= verdicts
    assert 2 * licensed <= len(streams)                                  # at least half are held to the host loop's verdict
