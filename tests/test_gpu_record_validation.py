"""Every record validator of the library against the oracle on malformed streams (docs/SPEC.md §4):
record_runs_check<64> (apply_tiny_kernel, the merge kernels), record_runs_check<16> (apply_kernel,
and the from-global path of every kernel) and the lane-serial walk of flat_window
(apply_flat_kernel), reached through gdsm_apply, gdsm_apply_async, gdsm_wire_apply and gdsm_merge.

The records are the corpus of tests/record_corpus.py; what each call must leave behind is the
oracle's answer per record. After every call: -EINVAL exactly when the list holds a refused
record, every accepted record's page equal to the oracle's, every refused record's page and every
other page of the arena (the 32 guard pages after each corpus page included) unchanged, and the
context still usable. The lists are built so that a wrongly accepted record shows as a wrong byte
in that comparison (tests/test_record_corpus.py checks their layout on the CPU)."""
import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import _lib
from gallocy_amd.gdsm import GdsmError, Runs
from oracle import oracle, wire
from tests import record_corpus as rc
from tests.test_gpu_merge import run_merge

pytestmark = pytest.mark.gpu

SMALL = rc.build([64], [8], np.arange(1, 9, dtype=np.uint8))


class Case:
    """A list, its arena before and after (the oracle's), and a REPLICA-only context for it."""

    def __init__(self, lst, seed):
        self.lst = lst
        self.init, self.want = lst.arena(seed)
        self.ctx = ga.Context(lst.n_pages, arenas=("replica",))

    def close(self):
        self.ctx.close()


def _case(lst, seed):
    c = Case(lst, seed)
    try:
        yield c
    finally:
        c.close()


@pytest.fixture(scope="module")
def tiny():
    yield from _case(rc.tiny_list(), 101)


@pytest.fixture(scope="module")
def short():
    yield from _case(rc.short_list(), 102)


@pytest.fixture(scope="module")
def long():
    yield from _case(rc.long_list(), 103)


def _upload(ctx, lst):
    """The list on the device: the data allocation is the padded stream, zero bytes behind it."""
    rc.check_safety(lst, alloc=len(lst.data))
    runs = Runs(ctx, lst.n, max(16, len(lst.data)))
    ro = np.ascontiguousarray(lst.rec_off, np.uint64)
    L = ga.gdsm.lib()
    ga.gdsm.check(L.gdsm_memcpy_h2d(ctx.handle, runs.s.rec_off, ro.ctypes.data, ro.nbytes), "h2d")
    if len(lst.data):
        ga.gdsm.check(L.gdsm_memcpy_h2d(ctx.handle, runs.s.data, lst.data.ctypes.data, lst.data.nbytes), "h2d")
    return runs, ctx.ids(lst.ids)


def _describe(lst, pages):
    by_page = {p: e for _, p, e in lst.slots}
    out = []
    for p in pages[:12]:
        p = int(p)
        if p in by_page:
            out.append(f"page {p}: {by_page[p].name} ({'accepted' if by_page[p].accepted else 'refused'})")
        else:
            near = max((q for q in by_page if q < p), default=None)
            out.append(f"page {p}: not a corpus page" +
                       (f", {p - near} after {by_page[near].name}" if near is not None else ""))
    return "; ".join(out)


def _compare(got, want, lst):
    """The whole arena against the oracle's: accepted pages, refused pages, guard pages, fillers."""
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero((got != want).any(axis=1))
    pytest.fail(f"{len(bad)} pages differ from the oracle: {_describe(lst, bad)}")


def _still_works(case):
    """One small valid apply on the arena's last page, which no list targets."""
    ctx, page = case.ctx, case.lst.n_pages - 1
    before = ctx.download("replica", page, 1)
    want = before.copy()
    ro = np.array([0, len(SMALL)], np.uint64)
    assert oracle.apply(want, ro, SMALL) == 0
    runs = Runs.from_host(ctx, ga.HostRuns(ro, SMALL))
    ids = ctx.ids(np.array([page], np.uint32))
    ctx.apply(runs, "replica", ids)
    ctx.sync()
    assert np.array_equal(ctx.download("replica", page, 1), want)
    ctx.upload("replica", before, page)
    runs.free()
    ids.free()


def _sync(ctx, refused):
    if refused:
        with pytest.raises(GdsmError) as e:
            ctx.sync()
        assert e.value.errno == 22
    else:
        ctx.sync()


def _run_apply(case, variant=0, use_async=False):
    ctx, lst, want = case.ctx, case.lst, case.want
    L = _lib.load()
    ctx.upload("replica", case.init)
    runs, ids = _upload(ctx, lst)
    assert L.gdsm_tune(b"apply_variant", variant) == 0
    try:
        (ctx.apply_async if use_async else ctx.apply)(runs, "replica", ids)
        _sync(ctx, lst.refused)
    finally:
        L.gdsm_tune(b"apply_variant", 0)
    _compare(ctx.download("replica"), want, lst)
    _still_works(case)
    runs.free()
    ids.free()


# ---- a. the tiny path: apply_tiny_kernel, record_runs_check<64>, and its oversized branch ----
def test_tiny_list(tiny):
    assert tiny.lst.n <= 4096 and tiny.lst.refused
    _run_apply(tiny)


@pytest.mark.parametrize("variant", [0, 1])
def test_list_of_accepted_records_reports_nothing(variant):
    """No refused record, no -EINVAL: the accepted mutants (abutting runs, a payload shifted by a
    byte) among the canonical records, wave form and row form."""
    case = Case(rc.RecordList([e for e in rc.ordered() if e.accepted]), 104)
    try:
        assert not case.lst.refused and len(case.lst.slots) >= 40
        _run_apply(case, variant=variant)
    finally:
        case.close()


# ---- b. the row form on short lists: apply_kernel<0, kApplyWinShort>, record_runs_check<16> ----
def test_row_form_variant_1(tiny):
    _run_apply(tiny, variant=1)


def test_row_form_default_variant_between_4097_and_16384_records(short):
    assert 4096 < short.lst.n <= 16384 and short.lst.refused
    _run_apply(short)


# ---- c. long lists: every apply_variant above 16384 records ----
@pytest.mark.parametrize("variant", list(range(8)))
def test_long_list(long, variant):
    """Variants 0, 3, 4, 5, 6, 7: apply_flat_kernel (flat_window's header walk; records larger than
    the 4 / 8 / 2 KiB window through the row form from global memory); 1 and 2: apply_kernel with
    an 8 / 4 KiB window. Three copies of the corpus start at lanes 0, 1 and 63 of a task."""
    assert long.lst.n > 16384 and long.lst.refused
    _run_apply(long, variant=variant)


# ---- d. gdsm_apply_async: the same kernels on the second stream ----
def test_apply_async(tiny):
    _run_apply(tiny, use_async=True)


# ---- e. gdsm_wire_apply: records inside a frame with a valid checksum ----
def _wire_case(items, seed):
    lst = rc.with_tail(items, np.random.default_rng(seed))
    rc.check_safety(lst, alloc=lst.total)  # the frame's data ends the device buffer
    text = wire.encode(lst.ids, lst.rec_off, lst.data)
    ids, ro, data = wire.decode(text)
    assert np.array_equal(ids, lst.ids) and np.array_equal(ro, lst.rec_off) and np.array_equal(data, lst.data)
    return Case(lst, seed), text


def _wire_refused(case, text):
    """-EINVAL; refused pages, guard pages and every unlisted page unchanged; a page of a valid
    record applied or untouched (SPEC §7: records before a malformed one may already be applied)."""
    ctx, lst = case.ctx, case.lst
    assert lst.refused
    ctx.upload("replica", case.init)
    with pytest.raises(GdsmError) as e:
        ctx.wire_apply(text)
    assert e.value.errno == 22
    got = ctx.download("replica")
    valid = np.zeros(lst.n_pages, bool)
    valid[[p for _, p, e in lst.slots if e.accepted] + [p for _, p in lst.fillers]] = True
    same_init = (got == case.init).all(axis=1)
    same_want = (got == case.want).all(axis=1)
    bad = np.flatnonzero(~np.where(valid, same_init | same_want, same_init))
    assert len(bad) == 0, _describe(lst, bad)
    _still_works(case)


def test_wire_apply_short_frame():
    case, text = _wire_case(rc.wire_subset(rc.ordered()), 201)
    try:
        assert case.lst.n <= 4096
        _wire_refused(case, text)
    finally:
        case.close()


def test_wire_apply_frame_of_accepted_records():
    case, text = _wire_case([e for e in rc.wire_subset(rc.ordered()) if e.accepted], 202)
    try:
        assert not case.lst.refused and len(case.lst.slots) >= 40
        case.ctx.upload("replica", case.init)
        assert case.ctx.wire_apply(text) == case.lst.n
        _compare(case.ctx.download("replica"), case.want, case.lst)
        _still_works(case)
    finally:
        case.close()


def test_wire_apply_long_frame_reaches_the_flat_kernel():
    rng = np.random.default_rng(203)
    items, _ = rc.long_items(rc.wire_subset(rc.ordered()), rng, fronts=(0,))
    case, text = _wire_case(items, 203)
    try:
        assert case.lst.n > 16384
        _wire_refused(case, text)
    finally:
        case.close()


# ---- f. gdsm_merge: both record_check<64> call sites ----
@pytest.fixture(scope="module")
def mctx():
    with ga.Context(16) as c:
        yield c


@pytest.mark.parametrize("K", [1, 2])
def test_merge_takes_nothing_from_a_refused_record(mctx, K):
    """The corpus as stream 0 (K = 2: small valid records of a second writer on the same pages):
    offsets, data, conflicts, counts and the guard bytes past the out stream against
    tests/merge_model.py; sync reports -EINVAL; a refused record contributes nothing; abutting
    runs come out fused."""
    lst = rc.tiny_list()
    rc.check_safety(lst, alloc=len(lst.data))
    streams = [lst.stream()]
    second = None
    if K == 2:
        rng = np.random.default_rng(301)
        second = [rc.build([int(rng.integers(0, rc.PAGE - 4))], [4], rng.integers(1, 256, 4, dtype=np.uint8))
                  for _ in range(lst.n)]
        ro = np.zeros(lst.n + 1, np.uint64)
        ro[1:] = np.cumsum([len(r) for r in second])
        streams.append((ro, np.concatenate(second)))
    (m_ro, m_data, *_), out = run_merge(mctx, streams, einval=True)
    out.free()
    fused = 0
    for i, _, e in lst.slots:
        got = m_data[int(m_ro[i]):int(m_ro[i + 1])]  # (run_merge: identical to the device's)
        if not e.accepted:
            assert got.tobytes() == (second[i].tobytes() if K == 2 else b""), e.name
        elif K == 1:
            page = e.init.copy()
            assert oracle.apply(page.reshape(1, -1), np.array([0, len(got)], np.uint64), got) == 0
            assert np.array_equal(page, e.page), e.name
            if e.cls == rc.ABUTTING:
                assert int(rc.words(got)[0]) == int(rc.words(e.rec)[0]) - 1, e.name
                fused += 1
            elif e.cls == rc.BASE:
                assert got.tobytes() == e.rec.tobytes(), e.name
    assert K == 2 or fused >= 10
    # the context still merges
    _, out = run_merge(mctx, [(np.array([0, len(SMALL)], np.uint64), SMALL)])
    out.free()
