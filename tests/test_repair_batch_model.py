"""The model of the batch kernel (tests/models/repair_batch.py: the tie by smallest last occurrence, the in-place rebuild at both table
sizes, rounds in slices with the state carried, the chunked scans) against grammar() of tests/models/repair.py, the reference's two loops
restated, on the batches of tests/repair_batches.py.  Texts too long for the literal loops in Python are held against the host loop
tdc_repair_grammar, which tests/test_repair_cli.py holds against grammar().  No GPU."""
import functools

import pytest

from tests import repair_batches as B
from tests.models import repair as M
from tests.models import repair_batch as RB

LITERAL_MAX = 2100            # grammar() walks linked lists in Python: O(rules * n)


@functools.lru_cache(maxsize=None)
def want(x, max_rules=0):
    if len(x) <= LITERAL_MAX:
        r, s = M.grammar(x, max_rules)
    else:
        r, s = B.as_model(*B.host(x, max_rules))
    return tuple(r), tuple(s)


def run(texts, **kw):
    st = RB.BatchStats()
    got = RB.batch_grammars(texts, stats=st, **kw)
    for x, g in zip(texts, got):
        r, s = want(x, kw.get("max_rules", 0))
        assert g == (list(r), list(s)), (len(x), x[:24], kw)
    return st


SMALL = ("count0", "count1", "only_empties", "no_pair_across", "a_next_to_a", "split_runs", "same_at_three_places", "smallest")


@pytest.mark.parametrize("name", SMALL)
def test_small_batches_with_invariants(name):
    st = run(B.batch(name), check=True)
    assert st.peak <= 0.5
    if name == "no_pair_across":
        assert st.rules == 0
    run(B.batch(name), rounds=1, table=1, check=True)


def test_known_answers():
    for x, rules, start in B.kat_cases():
        assert RB.batch_grammars([x]) == [([tuple(r) for r in rules], list(start))]
    texts = [x for x in B.batch("known") if len(x) <= 4200]
    st = run(texts)
    assert st.tie_rounds > 0
    st = run([b"a" * 65537, b"b" + b"a" * 65536], rounds=3)          # runs over 33 chunks, from an even and an odd position
    assert st.tie_rounds == 0 and st.launches >= 6


def test_forks():
    texts = B.batch("forks")[::3]
    st = run(texts)
    assert st.rebuilds > 0                                           # the table is halved as the sequence shrinks
    run(B.batch("forks")[-3:], table=1, rounds=7)


def test_ties_are_decided_by_the_last_occurrence():
    st = run([B.tie_text(), B.tie_text()[::-1], B.tie_text() + B.tie_text()[::-1]], check=True)
    assert st.tie_rounds > 100
    for mr in (1, 2, 7):
        run([B.tie_text()], max_rules=mr)


@pytest.mark.parametrize("rounds,table", [(1, 0), (3, 0), (256, 0), (256, 1), (3, 1)])
def test_slices_and_table_sizes(rounds, table):
    texts = B.batch("random300")[::30]
    st = run(texts, rounds=rounds, table=table)
    most = max(len(want(x)[0]) for x in texts)
    if rounds == 1:
        assert st.launches >= most                                   # one rule per launch, and the launch that finds nothing left
    assert st.launches <= most // rounds + 2
    assert st.rebuilds > 0 and st.peak <= 0.5
    assert (st.fills > 0) == (table == 1)                            # only the small table asks for a rebuild because it could fill


@pytest.mark.parametrize("max_rules", [1, 64, 512])
def test_max_rules(max_rules):
    texts = B.batch("random300")[5::40] + (b"", b"a", b"abab")
    st = run(texts, max_rules=max_rules)
    counts = [len(want(x, max_rules)[0]) for x in texts]
    assert max(counts) <= max_rules and min(counts) < max_rules      # texts that need fewer rules than the cap are among them
    assert st.rules == sum(counts)


def test_the_table_of_a_text():
    assert [RB.table_slots(n, 4) for n in (0, 1, 2, 3, 255, 256, 257, 1 << 24, (1 << 24) + 1)] == [0, 0, 8, 16, 1024, 1024, 2048, 1 << 26, 0]
    assert [RB.table_slots(n, 2) for n in (2, 4, 5, 256, 257)] == [8, 8, 16, 512, 1024]
    assert RB.batch_grammars([b"ab", b"x" * ((1 << 24) + 1), b"abab"])[1] is None
