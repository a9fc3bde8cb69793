"""The record corpus of tests/record_corpus.py, checked on the CPU: every class is there, the oracle
gives every class the verdict the GPU tests rely on, and no list built from it can make a wrong
validator reach outside an allocation (tests/test_gpu_record_validation.py runs these lists)."""
import collections

import numpy as np
import pytest

from oracle import oracle
from tests import merge_model as mm
from tests import record_corpus as rc


@pytest.fixture(scope="module")
def corpus():
    return rc.corpus()


def test_every_class_is_present(corpus):
    have = collections.Counter(e.cls for e in corpus)
    for cls in rc.ACCEPTED_CLASSES + rc.REFUSED_CLASSES:
        assert have[cls] >= 1, cls
    assert set(have) == set(rc.ACCEPTED_CLASSES + rc.REFUSED_CLASSES)
    by_base = {e.base for e in corpus if e.cls == rc.BASE}
    assert by_base >= {f"runs{k}" for k in rc.RUN_COUNTS} | {"whole", "long_odd_a"}
    # the step boundaries of both wave forms: a bad run 16 and a bad run 64 in every class that
    # names a run, each in a record that goes on after that run
    for cls in (rc.LEN0, rc.SWAPPED, rc.OVERLAP1, rc.ABUTTING, rc.REACH_FFFF):
        notes = {(e.note, e.base) for e in corpus if e.cls == cls}
        assert ("r16", "runs129") in notes and ("r64", "runs129") in notes, cls
        assert ("r16", "runs17") in notes and ("r64", "runs65") in notes, cls


def test_verdicts_per_class(corpus):
    for e in corpus:
        rcode, page = rc.verdict_and_page(e.rec, e.init)
        assert rcode == e.verdict and np.array_equal(page, e.page)
        if e.cls in rc.REFUSED_CLASSES:
            assert e.verdict == -22, e.name
            assert np.array_equal(e.page, e.init), e.name
        else:
            assert e.verdict == 0, e.name
        assert len(e.rec) % 4 == 0 and e.init.all()


def test_base_records_reproduce_current(corpus):
    B = rc.bases()
    n = 0
    for e in corpus:
        if e.cls != rc.BASE:
            continue
        twin, cur, rec = B[e.base]
        assert e.accepted and np.array_equal(e.page, cur) and (twin != cur).any()
        n += 1
    assert n == len(B) >= len(rc.RUN_COUNTS) + 2
    assert {int(rc.words(B[f"runs{k}"][2])[0]) for k in rc.RUN_COUNTS} == set(rc.RUN_COUNTS)


def test_accepted_mutants_change_what_is_written(corpus):
    """An accepted mutant is not its base under another name: its page differs from the base's
    current page (a payload shifted by a byte, a run moved), so a kernel that got it wrong shows."""
    B = rc.bases()
    for e in corpus:
        if e.cls in (rc.ABUTTING, rc.LEN1_SAME):
            assert not np.array_equal(e.page, B[e.base][1]), e.name


def test_counts(corpus):
    assert sum(e.accepted for e in corpus) >= 40
    assert sum(not e.accepted for e in corpus) >= 80
    assert len(corpus) <= 4096


def test_merge_model_agrees_with_the_oracle(corpus):
    """tests/merge_model.py's parse_record and or_apply give every corpus record the same verdict,
    and the same bytes where they accept."""
    for e in corpus:
        cov, val = mm.parse_record(e.rec)
        assert isinstance(cov, str) == (not e.accepted), e.name
        if e.accepted:
            want = e.init.copy()
            want[cov] = val[cov]
            assert np.array_equal(want, e.page), e.name


def _lists():
    rng = np.random.default_rng(1)
    sub = rc.wire_subset(rc.ordered())
    return {
        "tiny": rc.tiny_list(),
        "short": rc.short_list(),
        "long": rc.long_list(),
        "wire_short": rc.with_tail(sub, rng),
        "wire_accepted": rc.with_tail([e for e in sub if e.accepted], rng),
        "wire_long": rc.with_tail(rc.long_items(sub, rng, fronts=(0,))[0], rng),
    }


@pytest.fixture(scope="module")
def lists():
    return _lists()


def test_lists_cannot_reach_outside_an_allocation(lists):
    for name, lst in lists.items():
        rc.check_safety(lst)
        if name.startswith("wire"):
            assert len(lst.data) == lst.total  # nothing but the stream: what a frame carries
        # a REPLICA of n_pages pages holds the farthest store a header can name
        last = max(p for _, p, _ in lst.slots)
        assert (last * rc.PAGE + 0xFFFF + 0xFFFF) <= lst.n_pages * rc.PAGE
    assert lists["tiny"].n <= 4096 < lists["short"].n <= 16384 < lists["long"].n
    assert lists["wire_short"].n <= 4096 and lists["wire_long"].n > 16384
    assert lists["long"].n % 64 and lists["long"].n_pages * rc.PAGE < 200 << 20


def test_wire_subset_keeps_every_class(corpus):
    sub = rc.wire_subset(corpus)
    assert {e.cls for e in sub} == {e.cls for e in corpus}
    assert sum(not e.accepted for e in sub) >= 80 and sum(e.accepted for e in sub) >= 40


def test_check_safety_notices_a_violation():
    e = next(e for e in rc.corpus() if e.cls == rc.REACH_FFFF)
    lst = rc.RecordList([e])
    rc.check_safety(lst)
    with pytest.raises(AssertionError):
        rc.check_safety(lst, alloc=lst.total)      # the padding is what makes it safe
    lst.ids[0] = lst.n_pages                       # a page id outside the arena
    with pytest.raises(AssertionError):
        rc.check_safety(lst)


@pytest.mark.parametrize("win", [2048, 4096, 8192])
def test_long_list_places_refused_records_at_window_edges(lists, win):
    """In the long list, for every window size of the long-list kernels: the corpus copies start at
    lanes 0, 1 and 63 of a 64-record task, and some refused record is the first of a staged window,
    some the last, and some directly follows (in its task) a valid record that alone exceeds the
    window: each of the three in every copy."""
    lst = lists["long"]
    assert [s % 64 for s in lst.starts] == list(rc.LONG_FRONTS)
    n_c = len(rc.ordered())
    refused = {i for i, _, e in lst.slots if not e.accepted}
    valid_big = {i for i, _, e in lst.slots if e.accepted and len(e.rec) > win}
    w = rc.windows(lst.rec_off, 64, win)
    assert sum(b - a for a, b, _ in w) == lst.n

    def copy_of(i):
        return max(k for k, s in enumerate(lst.starts) if s <= i) if i < lst.starts[-1] + n_c else None

    first = {copy_of(a) for a, b, staged in w if staged and b - a > 1 and a in refused}
    last = {copy_of(b - 1) for a, b, staged in w if staged and b - a > 1 and b - 1 in refused}
    after = {copy_of(a) for a, b, staged in w
             if not staged and a in valid_big and a + 1 in refused and (a + 1) % 64}
    assert first == last == after == {0, 1, 2}
    # and every corpus record sits at three different lanes
    lanes = collections.defaultdict(set)
    for i, _, e in lst.slots:
        lanes[id(e)].add(i % 64)
    assert all(len(v) == 3 for v in lanes.values())
    assert {0, 63} <= {i % 64 for i in refused}


def test_short_lists_stage_four_records_per_task(lists):
    """The short form (4 records per task, 12 KiB window): the oversized records go alone, and a
    refused record is met in every one of a task's four rows."""
    for name in ("tiny", "short"):
        lst = lists[name]
        w = rc.windows(lst.rec_off, 4, 12288)
        alone = {a for a, b, staged in w if not staged}
        over = {i for i, _, e in lst.slots if len(e.rec) > 12288}
        assert alone == over and len(over) == 4
        assert {i % 4 for i, _, e in lst.slots if not e.accepted} == {0, 1, 2, 3}


def test_arena_expectation_is_the_oracles(lists):
    """RecordList.arena: corpus pages start as their record's initial page and end as the oracle's
    page; applying the list record by record with the oracle gives the same arena."""
    lst = lists["tiny"]
    init, want = lst.arena(5)
    assert init.all()
    got = init.copy()
    for i, page, e in lst.slots:
        one = lst.data[int(lst.rec_off[i]):int(lst.rec_off[i + 1])]
        rcode = oracle.apply(got, np.array([0, len(one)], np.uint64), one, ids=np.array([page], np.uint32))
        assert rcode == e.verdict
    assert np.array_equal(got, want)
    touched = np.flatnonzero((init != want).any(axis=1))
    assert set(touched) == {p for _, p, e in lst.slots if e.accepted}
