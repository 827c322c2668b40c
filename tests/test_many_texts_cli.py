"""CPU tests of tests/many_texts.py (no GPU): the batch sizes against the grid caps as the sources state them -- a changed cap fails
here, so tests/test_gpu_many_texts.py cannot silently go back to one text per workgroup --, the named sequences at their places, the
natures that repair's round kernel meets on consecutive trips, the pool's truth through the host decoders (once per pool entry), and the
numpy helpers against plain Python."""
import os
import re

import numpy as np
import pytest

import tudocomp_amd as T
from tests import lz_batches as LB
from tests import lzss_sw_batches as SB
from tests import many_texts as MT
from tests import repair_batches as RB
from tests.models import lzss_sw_decode as SMD

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tudocomp_amd", "csrc")
ALGOS = ("lzw-bit", "lzw-gamma", "lz78", "lzss-bit", "lzss-gamma", "lzss-delta")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def cap_in(text, function):
    """the N of `(size_t)1 << N` in the first statement after the function's name"""
    at = text.index(function + "(")
    m = re.compile(r"\(size_t\)1 << (\d+)\)").search(text, at)
    assert m and m.start() - at < 1200 and text.count(";", at, m.start()) <= 3, function
    return 1 << int(m.group(1))


def test_the_caps_are_what_the_sources_state():
    rb = source("repair_batch.hip")
    m = re.findall(r"constexpr unsigned RB_MAX_GRID = (\d+);", rb)
    assert len(m) == 1 and int(m[0]) == MT.RB_GRID
    assert "std::min<unsigned>(P.accepted, RB_MAX_GRID)" in rb
    caps = [cap_in(source("lz_batch.hip"), "unsigned lzb_text_grid"), cap_in(source("lz_batch_decode.hip"), "unsigned lzb_walk_grid"),
            cap_in(source("lzss_sw_batch.hip"), "unsigned swb_decode_grid"), cap_in(rb, "void rb_encode_as")]
    assert caps == [MT.CAP16] * 4
    # every kernel the batches are for walks the texts by its grid
    for name, loops in (("repair_batch.hip", ("j = blockIdx.x; j < P.accepted; j += gridDim.x", "k = blockIdx.x; k < E.count; k += gridDim.x")),
                        ("lz_batch.hip", ("k = blockIdx.x; k < P.count; k += gridDim.x", "k = blockIdx.x; k < count; k += gridDim.x")),
                        ("lz_batch_decode.hip", ("sidx = blockIdx.x; sidx < count; sidx += gridDim.x",)),
                        ("lzss_sw_batch.hip", ("sidx = blockIdx.x; sidx < count; sidx += gridDim.x",))):
        for loop in loops:
            assert loop in source(name), (name, loop)


def test_the_counts_reach_later_trips():
    assert MT.TRIPS3 > 2 * MT.CAP16 and MT.TRIPS3 > 2 * MT.RB_GRID and len(MT.trips3()) == MT.TRIPS3
    assert MT.BORDERS16 == (MT.CAP16, MT.CAP16 + 1, 2 * MT.CAP16 + 1)
    assert MT.REPAIR_BORDERS[:3] == (MT.RB_GRID, MT.RB_GRID + 1, 2 * MT.RB_GRID + 1) and MT.REPAIR_BORDERS[3] > 3 * MT.RB_GRID
    for count in MT.BORDERS16:
        assert len(MT.border(count)) == count
    for count in MT.REPAIR_BORDERS:
        assert len(MT.repair_border(count)) == count
    # workgroups 0 .. 4098 take three texts, all others two
    trips = np.bincount(np.arange(MT.TRIPS3) % MT.CAP16, minlength=MT.CAP16)
    assert (trips[:4099] == 3).all() and (trips[4099:] == 2).all()


def test_the_pool():
    pool = MT.pool()
    classes = {c for _, c, _ in pool}
    assert len(pool) <= 125 and max(len(x) for _, _, x in pool) <= MT.TEXT_MOST
    assert classes == {"empty", "tiny", "bulk", "long", "a5000", "tietext", "distinct64", "runs", "refused"} | set(MT.NATURES)
    by = {name: x for name, _, x in pool}
    assert by["empty"] == b"" and {len(x) for _, c, x in pool if c == "tiny"} == {1, 2, 3}
    assert all(3 <= len(x) <= 40 and set(x) <= set(b"abcd") for _, c, x in pool if c == "bulk")
    assert all(300 <= len(x) <= 700 for _, c, x in pool if c == "long")
    assert by["a5000"] == b"a" * 5000 and by["tie"] == RB.tie_text()
    assert len(set(by["distinct64"])) == 64 and len(RB.host(by["distinct64"])[0]) == 0     # no repeated pair: no rule
    assert set(by["zeros300"]) == {0} and set(by["ff300"]) == {255}
    # what lz78 refuses alone, and only that: the left-over phrase ends on a byte >= 0x80
    status = MT.lz78_statuses()
    refused = {name for (name, _, _), s in zip(pool, status.tolist()) if s}
    assert refused == {name for name, c, _ in pool if c == "refused"} and (status[status != 0] == MT.ERR_UNSUPPORTED).all()
    assert all(by[name][-1] >= 0x80 for name in refused) and len(by["refused_long"]) > 300
    # the depth turns above 64 of lz78 and lzw, and the chunked mark of repair, come from a^5000
    assert LB.lzw_lengths(LB.lzw_codes(by["a5000"])).max() > 64 and len(LB.lz78_pairs(by["a5000"])[0]) > 64
    assert 5000 > 2 * RB.CHUNK


def test_every_named_sequence_is_at_its_places():
    index, names = MT.trips3(), MT.names()
    seen = set()
    for name, seq, places in MT.SEQUENCES:
        for k in places:
            assert k < 4099 and not {k, k + MT.CAP16, k + 2 * MT.CAP16} & seen
            seen |= {k, k + MT.CAP16, k + 2 * MT.CAP16}
            assert [index[k + trip * MT.CAP16] for trip in range(3)] == [names[x] for x in seq], name
    cls = {name: c for name, c, _ in MT.pool()}
    length = {name: len(x) for name, _, x in MT.pool()}
    want = {"long_empty_long": lambda a, b, c: length[a] >= 700 and length[b] == 0 and length[c] >= 700,
            "empty_long_tiny": lambda a, b, c: length[a] == 0 and length[b] >= 300 and length[c] == 1,
            "refused_accepted_refused": lambda a, b, c: [cls[x] == "refused" for x in (a, b, c)] == [True, False, True],
            "accepted_refused_accepted": lambda a, b, c: [cls[x] == "refused" for x in (a, b, c)] == [False, True, False],
            "run_nopair_tie": lambda a, b, c: (cls[a], cls[b], cls[c]) == ("a5000", "distinct64", "tietext"),
            "ff_one_00": lambda a, b, c: (a, length[b], c) == ("ff300", 1, "zeros300"),
            "refused_refused_accepted": lambda a, b, c: [cls[x] == "refused" for x in (a, b, c)] == [True, True, False]}
    assert set(want) == {name for name, _, _ in MT.SEQUENCES}
    for name, seq, _ in MT.SEQUENCES:
        assert want[name](*seq), name
    # the batch: every class in it, short texts by far the most, below 8 MB
    lens = np.array([len(x) for x in MT.texts()])[index]
    assert lens.sum() < 8 << 20 and set(index.tolist()) == set(range(len(MT.pool())))
    assert (lens <= 40).mean() > 0.9
    for count in MT.BORDERS16:
        b = MT.border(count)
        assert {MT.pool()[j][1] for j in set(b.tolist())} <= set(MT.SHORT) and len(MT.texts()[b[-1]]) > 0


@pytest.mark.parametrize("algo", ALGOS)
def test_the_damaged_streams_are_at_their_places(algo):
    streams, status, texts, index = MT.decode_batch(algo)
    count = len(MT.pool())
    assert len(status) == len(streams.len) == len(texts.len) > count and (status[:count] == 0).all()
    assert (status[count:] != 0).any() and (status[count:] == 0).any() and set(status.tolist()) <= {0, MT.ERR_ARG, MT.ERR_TOO_LARGE}
    assert (texts.len[status != 0] == 0).all()
    used = set()
    for name, pattern, places in MT.DAMAGE_PLACES:
        for k in places:
            at = [k + trip * MT.CAP16 for trip in range(3)]
            assert k < 4099 and [int(index[p]) < count for p in at] == [bool(v) for v in pattern], name
            assert all(len(streams[index[p]]) > (100 if index[p] < count else 0) for p in at)
            used |= {int(index[p]) for p in at if index[p] >= count}
    assert used == set(range(count, len(status)))                       # every damaged stream is somewhere
    taken = {k + trip * MT.CAP16 for _, _, places in MT.SEQUENCES for k in places for trip in range(3)}
    changed = set(np.flatnonzero(index != MT.trips3()).tolist())
    assert not changed & taken and len(changed) >= 12
    assert int(streams.len[index].sum()) < 16 << 20 and int(texts.len[index].sum()) < 16 << 20


def test_repair_meets_different_natures_on_consecutive_trips():
    nature = np.array([MT.NATURES.index(c) if c in MT.NATURES else -1 for _, c, _ in MT.pool()])
    lens = np.array([len(x) for x in MT.texts()])
    for count in MT.REPAIR_BORDERS:
        index = MT.repair_border(count)
        assert (nature[index] >= 0).all()
        for n in set(lens[index].tolist()):                              # several natures at every length
            assert len(set(nature[index[lens[index] == n]].tolist())) == len(MT.NATURES), (count, n)
        order = MT.round_order(index)
        assert (np.diff(lens[index[order]]) <= 0).all() and sorted(order.tolist()) == list(range(count))
        same_len = np.flatnonzero(np.diff(lens[index[order]]) == 0)
        assert (order[same_len] < order[same_len + 1]).all()             # stable
        if count > MT.RB_GRID + 1:
            nat = nature[index[order]]
            differ = nat[:count - MT.RB_GRID] != nat[MT.RB_GRID:]        # sorted place j and j + 2048: one workgroup's consecutive trips
            groups = len(set((np.flatnonzero(differ) % MT.RB_GRID).tolist()))
            assert groups >= 1000, (count, groups)
    index = MT.repair_border(MT.REPAIR_BORDERS[3])
    nat = nature[index[MT.round_order(index)]]
    three = sum(1 for j in range(MT.RB_GRID) if len({nat[j], nat[j + MT.RB_GRID], nat[j + 2 * MT.RB_GRID]}) >= 2)
    assert three >= 1000
    # trips3: the workgroups of the round kernel take 66 or 67 texts each
    nat = np.array([c for _, c, _ in MT.pool()])[MT.trips3()[MT.round_order(MT.trips3())]]
    differ = nat[:-MT.RB_GRID] != nat[MT.RB_GRID:]
    assert len(set((np.flatnonzero(differ) % MT.RB_GRID).tolist())) >= 1000


def test_the_pools_truth_decodes_back():
    texts = MT.texts()
    for coder in ("bit", "gamma"):
        s = MT.lzw_streams(coder)
        assert all(T.lzw_decode(s[j].tobytes(), LB.LZW_CODERS[coder]) == x for j, x in enumerate(texts)), coder
    s, status = MT.lz78_streams(), MT.lz78_statuses()
    for j, x in enumerate(texts):
        assert (len(s[j]) == 0) if status[j] else (LB.lz78_decode(s[j].tobytes()) == x), j
    for coder in MT.LZSS_CODERS:
        status, s = MT.lzss_truth(coder)
        assert (status == 0).all()                                       # window 16: no length that five bits do not hold
        assert all(SMD.decode(s[j].tobytes(), coder, MT.WINDOW) == x for j, x in enumerate(texts)), coder
        assert all(T.lzss_sw_decode(s[j].tobytes(), SB.CODER_ID[coder], MT.WINDOW) == x for j, x in enumerate(texts)), coder
    for max_rules in (0, 1):
        for coder in MT.REPAIR_CODERS:
            s = MT.repair_streams(coder, max_rules)
            assert all(T.repair_decode(s[j].tobytes(), RB.CID[coder]) == x for j, x in enumerate(texts)), (coder, max_rules)
        assert MT.repair_rules(max_rules).len.max() == (1 if max_rules else MT.repair_rules(0).len.max()) > 0
    assert (MT.repair_rules(0).len == 0).sum() > 10 and MT.repair_rules(0).len.max() > 100
    # the items of the parses: as many as the streams hold
    assert MT.lzw_items().len.sum() > 0 and (MT.lz78_ids().len == MT.lz78_chars().len).all()


def test_take_and_differing_against_plain_python():
    rng = np.random.default_rng(1)
    seqs = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 20, 30)] + [b""]
    r = MT.Ragged(seqs)
    index = rng.integers(0, len(seqs), 500)
    for align in (1, 8):
        flat, off, lens = MT.take(r, index, align)
        assert (off % align == 0).all() and lens.tolist() == [len(seqs[j]) for j in index]
        assert [flat[o:o + n].tobytes() for o, n in zip(off[:-1].tolist(), lens.tolist())] == [seqs[j] for j in index]
        assert len(MT.differing(flat, off[:-1], lens, r, index)) == 0
        longest = int(np.argmax(lens))
        bad = flat.copy()
        bad[off[longest] + lens[longest] - 1] ^= 1                        # one bit of one text
        assert MT.differing(bad, off[:-1], lens, r, index).tolist() == [longest]
        shorter = lens.copy()
        shorter[longest] -= 1                                            # one length
        assert MT.differing(flat, off[:-1], shorter, r, index).tolist() == [longest]
    got = [seqs[j] for j in index]
    flat, starts, lens = MT.flatten(got, np.uint8)
    assert len(MT.differing(flat, starts, lens, r, index)) == 0
    words = MT.Ragged([np.arange(n, dtype=np.uint64) << 40 for n in range(9)], np.uint64)
    idx = np.array([8, 0, 3, 3])
    flat, starts, lens = MT.flatten([words[j].copy() for j in idx], np.uint64)
    assert len(MT.differing(flat, starts, lens, words, idx)) == 0 and flat.dtype == np.uint64
