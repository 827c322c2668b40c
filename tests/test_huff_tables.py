"""CPU tests of tests/huff_tables.py: the crafted encode(huff) streams are what they claim to be.  The host decoder (the specification)
and the parallel formulation of tests/models/bytestage_decode.py return the symbols put in; the border sweep reaches every entry offset,
the chunk and group borders and the walk behind bit 64 -- conditions on the INPUTS of tests/test_gpu_huff_tables.py, proved here so that
the GPU tests cannot pass vacuously; the refusal streams are refused."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import huff_tables as H
from tests import prim_inputs as P
from tests.models import bytestage_decode as D

TABLES = {t.name: t for t in H.tables()}
SWEEPABLE = [n for n, t in TABLES.items() if len(t.deepest) >= 2]
assert len(SWEEPABLE) == len(TABLES) - 1 and "chain(129)-sigma100" not in SWEEPABLE      # (its deepest codes are the ones sigma cuts off)
# The model computes next(x) at every bit in plain Python: about 6 us a bit and more inside deep codes.  Its sequences hold 3000 codes
# up to 65 bits and 1000 above (chain(255): 128 000 bits, 63 tiles of 2048, 500 of 256).  A border sweep is 2^20 bits and more: 4 to 7 s
# per (tile, group) up to 33 bits, and more the deeper the table.  So the model walks the sweeps of the chains up to 33 bits (five tables)
# at (2048, 512), where tile 512 heads the second group, and those of 12 and 13 bits at (256, 4) as well.  The sweeps of the thirteen
# deeper tables go through the host decoder alone (test_border_sweep_reaches_what_it_is_for); the model meets their entry offsets in the
# uniform sequences, not one by one.
MODEL_CODES = lambda t: 3000 if t.longest <= 65 else 1000
MODEL_SWEEPS = {"chain(12)": ((2048, 512), (256, 4)), "chain(13)": ((2048, 512), (256, 4)), "chain(31)": ((2048, 512),),
                "chain(32)": ((2048, 512),), "chain(33)": ((2048, 512),)}


def test_the_tables_are_the_ones_asked_for():
    assert P.DX_G == H.DX_G
    for L in H.CHAIN_DEPTHS:
        t = TABLES["chain(%d)" % L]
        assert t.longest == L and t.sigma == L + 1 and t.usable.all()
        assert [format(int(v), "0%db" % l) for l, v in zip(t.length, t.value)] == ["0" * (l - 1) + "1" for l in range(1, L)] + ["0" * L, "0" * (L - 1) + "1"]
    assert TABLES["chain(255)"].sigma == 256
    for (L, D), reach in zip(H.BUSHY_SHAPES, (32, 128, 16)):
        t = TABLES["bushy(%d,%d)" % (L, D)]
        d = D.bit_length() - 1
        assert t.longest == L and t.sigma == L - d + D and int(t.numl[-1]) == D and len(t.deepest) == reach
        assert (t.numl[:L - d] == 1).all() and not t.numl[L - d:-1].any()
        assert t.usable[:L - d].all()                                           # every single code above the block can be reached
    t = TABLES["bushy(70,20)-open"]
    assert t.numl[0] == 0 and t.first[0] == 1 and len(t.deepest) == 16            # "1" stops the decoder at length 1, where no code is
    t = TABLES["chain(129)-sigma100"]
    assert t.sigma == 100 < int(t.numl.sum()) and len(t.symbols) == 100 and int(t.length[t.symbols].max()) == 100
    # the literal bushy(70, 20) of one code at each length 1 .. L - ceil(log2 D) collapses: first = 1 at length 66, no code there
    lit = H.Table("literal", [1] * 65 + [0] * 4 + [20])
    assert lit.first[65] == 1 and lit.first[64] == 0 and lit.symbols.tolist() == [0]


def test_stream_layout_by_hand():
    # chain(3): longest 3, numl 1 1 2, sigma 4, order abcd; codes 1, 01, 000, 001.  "1" + 03 01 01 02 04 + abcd, then 1 01 000 001 1
    s, hb, total, starts = H.stream([1, 1, 2], b"abcd", [0, 1, 2, 3, 0])
    bits = "1" + "".join(format(b, "08b") for b in bytes([3, 1, 1, 2, 4]) + b"abcd") + "1" + "01" + "000" + "001" + "1"
    assert hb == 73 and total == 83 == len(bits) and starts.tolist() == [73, 74, 76, 79, 82]
    want = bits + "0" * (88 - 3 - len(bits)) + "011"                              # 83 % 8 = 3 < 6: the terminator shares the last byte
    assert s == int(want, 2).to_bytes(11, "big") and T.huff_decode_literals(s) == b"abcda"
    forms = set()
    for k in range(8):                                                            # every total % 8: own byte from 6 on, a zero byte at 0
        s, hb, total, _ = H.stream([1, 1, 2], b"abcd", [0] * k)
        u = total % 8
        forms.add(u)
        assert len(s) == total // 8 + (1 if u < 6 else 2) and s[-1] & 7 == u and D.huff_total_bits(s) == total
        assert (s[-1] == 0) == (u == 0) and T.huff_decode_literals(s) == b"a" * k
    assert forms == set(range(8))
    # values of 128 and more take two groups: low seven bits first
    assert H.header_bytes([0] * 200, b"", 0)[:2].tolist() == [0x80 | 72, 1] and H._groups(256) == [0x80, 2] and H._groups(127) == [127]


@pytest.mark.parametrize("name", list(TABLES))
def test_host_decoder_and_model_return_the_symbols(name):
    t = TABLES[name]
    rng = np.random.default_rng(t.longest)
    mean = float(t.length[t.symbols].mean())
    cases = [("uniform", H.uniform(t, int(3000 * mean), rng)), ("geometric", H.geometric(t, 3000, rng)),
             ("ends with a deepest code", H.ending_with_deepest(t, int(500 * mean), rng) if len(t.deepest) else t.symbols[-1:])]
    for kind, idx in cases:
        s, hb, total, starts = H.table_stream(t, idx)
        assert len(idx) >= 1 and total - hb == int(t.length[idx].sum()) and starts[0] == hb
        assert T.huff_decode_literals(s) == t.bytes_of(idx), kind
    assert len(cases[0][1]) >= 2500 and set(cases[0][1].tolist()) == set(t.symbols.tolist())     # uniform: every usable symbol occurs
    assert 1.9 < t.length[cases[1][1]].mean() < 3.1                                    # geometric: about two bits a code (three without "1")
    n = MODEL_CODES(t)
    for kind, idx in (("uniform", H.uniform(t, int(n * mean), rng)), ("geometric", H.geometric(t, n, rng))):
        assert len(idx) >= 0.85 * n, kind
        s = H.table_stream(t, idx)[0]
        for tile, group in ((max(256, t.longest), 4), (2048, 512)):
            assert D.huff_decode(s, tile, group) == t.bytes_of(idx), (kind, tile, group)


@pytest.mark.parametrize("name", SWEEPABLE)
def test_border_sweep_reaches_what_it_is_for(name):
    t = TABLES[name]
    L = t.longest
    borders = max(2 * L, 520)
    idx = H.border_sweep(t, borders)
    s, hb, total, starts = H.table_stream(t, idx)
    assert T.huff_decode_literals(s) == t.bytes_of(idx)
    assert 70 << 10 <= len(s) <= 140 << 10
    ln = t.length[idx]
    off = H.entry_offsets(starts, hb, total)
    assert len(off) == borders + 1 and off[0] == 0 and off[1:].tolist() == [(k - 1) % L for k in range(1, borders + 1)]
    assert set(off.tolist()) == set(range(L))                                       # every entry state of the tile scheme
    deep = ln == L
    tiles = H.straddles(starts, ln, H.HD_T, hb)
    assert int((deep & tiles).sum()) == int((off[1:] > 0).sum()) and not (tiles & ~deep).any()
    assert (deep & H.straddles(starts, ln, H.HD_CH, hb)).sum() >= 50                # the slack words of the exit pass's stream image
    group = deep & H.straddles(starts, ln, H.HD_T * H.DX_G, hb)
    assert group.sum() == 1 and (starts[group] - hb + L) // H.HD_T == H.DX_G        # ... and the one in front of tile 512
    # the two deepest codes alternate: the bit that tells them apart is the last one, behind the border
    assert set(idx[deep][0::2].tolist()) == {int(t.deepest[0])} and set(idx[deep][1::2].tolist()) == {int(t.deepest[1])}
    assert int(t.value[t.deepest[0]]) == 0 and int(t.value[t.deepest[1]]) == 1
    if L >= 65:                                                                     # the walk re-peeks at length 64 (128, 192)
        assert (ln[deep & tiles] > 64).all() and (deep & tiles).sum() >= 500


@pytest.mark.parametrize("name,tile,group", [(n, tl, g) for n, cfgs in MODEL_SWEEPS.items() for tl, g in cfgs])
def test_model_walks_the_border_sweep(name, tile, group):
    t = TABLES[name]
    idx = H.border_sweep(t, max(2 * t.longest, 520))
    assert D.huff_decode(H.table_stream(t, idx)[0], tile, group) == t.bytes_of(idx)


def test_refusal_streams_are_refused_for_the_code_put_in():
    cases = H.refusal_streams(np.random.default_rng(5))
    assert len(cases) == 8
    for name, bad, good in cases:
        with pytest.raises(T.TdcGpuError) as e:
            T.huff_decode_literals(bad)
        assert e.value.status == -2, name
        assert len(T.huff_decode_literals(good)) > 1000, name
        if "first" in name:                                                         # (the model walks every bit: the short case only)
            short = bad[:D.huff_header(bad, D.huff_total_bits(bad))[6] // 8 + 40] + b"\x00"
            with pytest.raises(D.Refused):
                D.huff_decode(short, 256, 4)
