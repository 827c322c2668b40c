"""GPU tests of repair over a batch of texts, one workgroup per grammar (tdc_gpu_repair_compress_batch, tdc_gpu_repair_grammar_batch;
repair_batch.hip).  Truth comes from code that is not under test (tests/repair_batches.py): the host loop tdc_repair_grammar for the
grammars -- rules and start sequence, exactly --, the model's coders on those grammars for the streams, tests/golden/repair_kats.json
for the hand-derived cases.  Every accepted stream goes back through tdc_repair_decode.  The batches are named for what they reach."""
import numpy as np
import pytest

import tudocomp_amd as T
from tests import repair_batches as B
from tests.models import repair_batch as RB

pytestmark = pytest.mark.gpu

CODERS = ("bit", "ascii", "gamma", "delta")


def run(ctx, texts, coder, max_rules=0):
    """(streams, statuses, stats) through the caller-owned entry point; what holds for every call is asserted here"""
    lengths = [len(x) for x in texts]
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    cap = T.repair_batch_bound(lengths, B.CID[coder])
    out = np.full(cap + 8, 0xA5, dtype=np.uint8)
    out_off, out_len, status, st = ctx.repair_compress_batch_into(data, off, out, max_rules, B.CID[coder])
    assert out_off[0] == 0 and (out_off % 8 == 0).all() and (np.diff(out_off.astype(np.int64)) >= out_len.astype(np.int64)).all()
    assert int(out_off[-1]) <= cap and (out[int(out_off[-1]):] == 0xA5).all()              # the bound is at least what was used
    assert st["n"] == sum(lengths) and st["out_len"] == int(out_off[-1])
    assert ((status == 0) | (out_len == 0)).all()
    return [out[int(o):int(o) + int(l)].tobytes() for o, l in zip(out_off[:-1], out_len)], status.tolist(), st


def check_grammars(ctx, texts, max_rules=0):
    rules, start, status = ctx.repair_grammar_batch(texts, max_rules)
    assert status == [0] * len(texts)
    bad = [k for k, x in enumerate(texts)
           if not (np.array_equal(rules[k], B.host(x, max_rules)[0]) and np.array_equal(start[k], B.host(x, max_rules)[1]))]
    assert not bad, ("grammar", bad[:5], len(bad), max_rules)


def check(ctx, texts, coders=CODERS, max_rules=0):
    """the grammars, the streams under the coders, the statuses, the counters and the way back; returns the last call's stats"""
    texts = list(texts)
    count = len(texts)
    check_grammars(ctx, texts, max_rules)
    st = None
    for coder in coders:
        got, status, st = run(ctx, texts, coder, max_rules)
        assert status == [0] * count
        bad = [k for k in range(count) if got[k] != B.stream(texts[k], coder, max_rules)]
        assert not bad, (coder, bad[:5], len(bad))
        assert st["rules"] == sum(len(B.host(x, max_rules)[0]) for x in texts)
        assert st["replaced"] == sum(len(x) - len(B.host(x, max_rules)[1]) for x in texts)
        assert all(T.repair_decode(got[k], B.CID[coder]) == texts[k] for k in range(count))
    return st


def test_known_answers_and_hand_derived_grammars(gpu_ctx):
    kats = B.kat_cases()
    rules, start, _ = gpu_ctx.repair_grammar_batch([x for x, _, _ in kats])
    for k, (x, want_rules, want_start) in enumerate(kats):
        assert B.as_model(rules[k], start[k]) == ([tuple(r) for r in want_rules], list(want_start)), x
    for coder in CODERS:                                                                    # each between two neighbours
        got, _, _ = gpu_ctx.repair_compress_batch([y for x, _, _ in kats for y in (b"zz", x, b"")], 0, B.CID[coder])
        assert got[1::3] == [B.stream(x, coder) for x, _, _ in kats]
    st = check(gpu_ctx, B.batch("known"))
    assert st["tie_rounds"] > 0


@pytest.mark.parametrize("name", ("no_pair_across", "a_next_to_a", "split_runs", "same_at_three_places"))
def test_borders(gpu_ctx, name):
    texts = B.batch(name)
    st = check(gpu_ctx, texts)
    if name == "no_pair_across":
        assert st["rules"] == 0 and st["replaced"] == 0                                    # 49 repeats in the concatenation, none in a text
    if name == "same_at_three_places":
        for coder in CODERS:
            got, _, _ = run(gpu_ctx, list(texts), coder)
            assert got[0] == got[3] == got[6] and len(got[0]) > 100                         # three neighbourhoods, one stream


@pytest.mark.parametrize("name", ("smallest", "count0", "count1", "only_empties"))
def test_smallest_and_empty(gpu_ctx, name):
    texts = B.batch(name)
    check(gpu_ctx, texts)
    for coder in CODERS:
        got, _, st = run(gpu_ctx, list(texts), coder)
        single = {x: gpu_ctx.repair_compress(x, 0, B.CID[coder])[0] for x in set(texts)}    # the single call, once per distinct text
        assert got == [single[x] for x in texts]                                            # every stream, none left out
        if name == "count0":
            assert got == [] and st["out_len"] == 0
        if name == "only_empties":
            assert len(got) == 5 and len(got[0]) > 0


@pytest.mark.parametrize("name", ("forks", "long_among_short", "random300"))
def test_forks_in_the_kernel(gpu_ctx, name):
    st = check(gpu_ctx, B.batch(name), coders=("bit", "gamma") if name == "long_among_short" else CODERS)
    assert st["len_rounds"] >= 1
    print("%s: %d texts, %d rules, %d tie rounds, %d rebuilds, %d launches, %.2f ms grammars, %.2f ms pack" % (
        name, len(B.batch(name)), st["rules"], st["tie_rounds"], st["rebuilds"], st["len_rounds"], st["ms_factorize"], st["ms_encode"]))


@pytest.mark.parametrize("max_rules", (1, 64, 512))
def test_max_rules(gpu_ctx, max_rules):
    texts = B.batch("capped")
    st = check(gpu_ctx, texts, coders=("bit", "delta"), max_rules=max_rules)
    counts = [len(B.host(x, max_rules)[0]) for x in texts]
    assert max(counts) == max_rules and 0 in counts and st["rules"] == sum(counts)


@pytest.mark.parametrize("rounds", (1, 3))
def test_slices(rounds):
    """a launch performs at most repair_batch_rounds rounds per text and leaves the state: the same grammars, more launches"""
    texts = list(B.batch("random300")[::6]) + [B.tie_text(), b"a" * 5000, b""]
    with T.Context(0) as ctx:
        ctx.set_option("repair_batch_rounds", rounds)
        check_grammars(ctx, texts)
        got, status, st = run(ctx, texts, "bit")
        assert got == [B.stream(x, "bit") for x in texts]
        most = max(len(B.host(x)[0]) for x in texts)
        if rounds == 1:
            assert st["len_rounds"] >= most                                                 # one rule per launch
        assert most // rounds <= st["len_rounds"] <= most // rounds + 2
        check_grammars(ctx, texts, 64)


def test_small_tables_are_rebuilt_in_the_kernel(gpu_ctx):
    """`rebuilds` counts the halvings of a shrinking text's table too, which the default table also does.  What repair_batch_table = 1
    adds are the rebuilds a table that could fill asks for: more rebuilds than the default on the same texts, and on a few texts
    exactly the model's count, whose fill condition is asserted to have fired."""
    texts = list(B.batch("random300")[::5]) + list(B.batch("forks")[::4]) + [B.tie_text()]
    few = list(B.batch("random300")[2::40]) + [B.tie_text()]
    model = {}
    for table in (0, 1):
        model[table] = RB.BatchStats()
        assert RB.batch_grammars(few, table=table, stats=model[table]) == [B.as_model(*B.host(x)) for x in few]
    assert model[0].fills == 0 and model[1].fills > 0 and model[1].rebuilds > model[0].rebuilds
    _, _, st0 = run(gpu_ctx, texts, "gamma")
    _, _, few0 = run(gpu_ctx, few, "gamma")
    with T.Context(0) as ctx:
        ctx.set_option("repair_batch_table", 1)
        check_grammars(ctx, texts)
        got, _, st = run(ctx, texts, "gamma")
        assert st["rebuilds"] > st0["rebuilds"] > 0 and st["tie_rounds"] > 0
        assert got == [B.stream(x, "gamma") for x in texts]
        _, _, few1 = run(ctx, few, "gamma")
    assert (few0["rebuilds"], few1["rebuilds"]) == (model[0].rebuilds, model[1].rebuilds)


def test_nothing_depends_on_what_the_arena_held(gpu_ctx):
    texts = list(B.batch("random300"))
    want = [B.stream(x, "bit") for x in texts]
    for fill in (0x00, 0x01, 0xFF):
        gpu_ctx.prim_arena_fill(fill)
        got, _, _ = run(gpu_ctx, texts, "bit")
        assert got == want, fill
    gpu_ctx.lzw_compress_batch(texts[:50], T.CODER_BIT)                                     # another entry point has used the arena
    gpu_ctx.repair_compress(B.english(30000, 9), 0, T.CODER_BIT)
    got, _, _ = run(gpu_ctx, texts, "bit")
    assert got == want


def test_placement_and_the_short_buffer(gpu_ctx):
    texts = list(B.batch("smallest"))
    lengths = [len(x) for x in texts]
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    data = np.frombuffer(b"".join(texts), dtype=np.uint8)
    _, _, st = run(gpu_ctx, texts, "delta")
    used = st["out_len"]
    assert used % 8 == 0 and used <= T.repair_batch_bound(lengths, T.CODER_DELTA)
    out = np.full(used - 1, 0x5A, dtype=np.uint8)
    with pytest.raises(T.TdcGpuError) as e:
        gpu_ctx.repair_compress_batch_into(data, off, out, 0, T.CODER_DELTA)
    assert e.value.status == B.ERR_OOM and e.value.required == used
    assert (out == 0x5A).all()                                                              # nothing was written
    out = np.full(used, 0x5A, dtype=np.uint8)
    out_off, out_len, status, _ = gpu_ctx.repair_compress_batch_into(data, off, out, 0, T.CODER_DELTA)
    assert int(out_off[-1]) == used and status.tolist() == [0] * len(texts)


def test_a_text_beyond_the_cap_is_refused_alone(gpu_ctx):
    a, c = b"abcdcdab", B.english(2000, 24)
    texts = [a, bytes(B.TEXT_CAP + 1), c]
    rules, start, status = gpu_ctx.repair_grammar_batch(texts)
    assert status == [0, B.ERR_TOO_LARGE, 0] and len(rules[1]) == 0 and len(start[1]) == 0
    assert np.array_equal(rules[0], B.host(a)[0]) and np.array_equal(start[2], B.host(c)[1])
    for coder in ("bit", "gamma"):
        got, status, st = run(gpu_ctx, texts, coder)
        assert status == [0, B.ERR_TOO_LARGE, 0] and got[1] == b""
        assert [got[0], got[2]] == [B.stream(a, coder), B.stream(c, coder)]
        assert st["rules"] == len(B.host(a)[0]) + len(B.host(c)[0])


def test_round_trip_on_the_device_and_the_facade(gpu_ctx):
    texts = list(B.batch("random300"))
    for coder in ("bit", "gamma", "delta"):
        got, _, _ = run(gpu_ctx, texts, coder)
        for k in range(0, 300, 15):                                                         # a sample of 20 through the device decoder
            assert gpu_ctx.repair_decompress(got[k], B.CID[coder]) == texts[k]
    comp = T.RePairCompressor(gpu_ctx, coder="gamma", max_rules=64)
    streams, status = comp.compress_batch(texts[:40])
    want, want_status, _ = gpu_ctx.repair_compress_batch(texts[:40], 64, T.CODER_GAMMA)
    assert streams == want and status == want_status == [0] * 40
    assert streams == [B.stream(x, "gamma", 64) for x in texts[:40]] and comp.last_stats["rules"] > 0
    assert streams[3] == comp.compress(texts[3])
