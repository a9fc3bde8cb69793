"""The long-list diff (more than 32768 pages: the grid form of diff_single_kernel) where the context
picks its own geometry, bit for bit against the oracle: every pair of (density that set the
hint, density being diffed), the first long lengths, fused apply / id lists / re-twin at that
size, the second use of a spill slot in the 16-page geometry, the raw entry point whose workspace
has no spill pool, and caller lists longer than one sweep of the prep kernel. Every case asserts
the geometry it claims through gdsm_debug_last_diff_variant; the inputs are those of
tests/diff_long_cases.py (checked on the CPU by tests/test_diff_long_cases.py).

The automatic table is pinned here: a change of kDense64 / kDense16 (gdsm_pages.hip) changes
DENSE64 / DENSE16 of tests/diff_long_cases.py with it."""
import ctypes as C
import errno

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import _lib
from gallocy_amd.gdsm import GdsmError, HostRuns, Runs
from oracle import oracle
from tests import diff_long_cases as dl

pytestmark = pytest.mark.gpu

GUARD = 0xA5
# bytes per page taught to a context to put its hint inside a band (diff_long_cases.BANDS)
TEACH = {"S": 50, "M": 300, "D": 1500}
VARIANT = {"S": 5, "M": 1, "D": 7}


def last_diff():
    """(variant, form) of this thread's last diff launch."""
    v = _lib.load().gdsm_debug_last_diff_variant()
    return v & 0xFF, v >> 8


def teach(c, n, hint):
    """Leaves `hint` in the context the way a caller does: gdsm_runs_total of a stream of n
    records whose total is (hint - 1) * n bytes (offsets only; nothing reads its data)."""
    ro = np.zeros(n + 1, np.uint64)
    ro[-1] = (hint - 1) * n
    r = Runs.from_host(c, HostRuns(ro, np.zeros(0, np.uint8)), cap=16)
    t = C.c_uint64(0)
    rc = _lib.load().gdsm_runs_total(c.handle, C.byref(r.s), C.byref(t))
    assert rc == (-errno.ENOSPC if ro[-1] > 16 else 0) and t.value == ro[-1]
    assert dl.hint_of(t.value, n) == hint
    r.free()


@pytest.fixture(scope="module")
def cases():
    """cases(cls, n, hot=(), ids=None) -> (twin, current, rec_off, data): the pages of a class and
    their oracle stream (of the list `ids`, a key of cases.lists, when given), computed once."""
    pages, streams, lists = {}, {}, {}

    def get(cls, n, hot=(), ids=None):
        if (cls, n, hot) not in pages:
            pages[cls, n, hot] = dl.pages(cls, n, hot=hot)
        t, c = pages[cls, n, hot]
        if (cls, n, hot, ids) not in streams:
            streams[cls, n, hot, ids] = oracle.diff_pages(t, c, ids=None if ids is None else lists[ids])
        return (t, c) + streams[cls, n, hot, ids]
    get.lists = lists
    yield get
    pages.clear()
    streams.clear()


def check_stream(runs, ro, data, what):
    assert runs.total() == int(ro[-1]), what
    host = runs.to_host()
    dl.assert_stream_equal(host.rec_off, host.data, ro, data, what)


def test_spill_slot_reuse_in_the_16_page_geometry(cases):
    """(d) 82 309 pages = 4 * 16 * 1280 + six workgroups + 5 pages of class X, the pages of the
    first users of spill slots 0-6 and of the tickets that take them again all spilling or late.
    Unknown hint: variant 5; the dense hint that leaves: variant 7, whose workgroups 1280 .. 1286
    wait for a slot, take it over and read back what they spilled into it; then the same with the
    fused apply over a permuted list; then twin() over all pages and a release with re-twin (both
    past their 65 536-page sweep)."""
    n = dl.N_REUSE
    t, cur, ro, data = cases("X", n, dl.HOT_REUSE)
    total = int(ro[-1])
    assert dl.expected_variant(dl.hint_of(total, n)) == 7
    with ga.Context(n) as c:
        c.upload("twin", t)
        c.upload("current", cur)
        runs = Runs(c, n, cap=total + 4096)
        c.diff(out=runs)
        assert last_diff() == (5, dl.FORM_GRID)
        check_stream(runs, ro, data, "unknown hint")
        c.diff(out=runs)
        assert last_diff() == (7, dl.FORM_GRID)
        check_stream(runs, ro, data, "dense hint")
        cases.lists["perm_reuse"] = ids = np.random.default_rng(82).permutation(n).astype(np.uint32)
        _, _, ro_p, data_p = cases("X", n, dl.HOT_REUSE, ids="perm_reuse")
        c.upload("replica", t)
        c.diff(c.ids(ids), out=runs, apply_to="replica")
        assert last_diff() == (7, dl.FORM_GRID)
        check_stream(runs, ro_p, data_p, "dense hint, permuted list, fused apply")
        assert np.array_equal(c.download("replica"), cur)
        c.twin()
        c.sync()
        assert np.array_equal(c.download("twin"), cur)
        c.diff(out=runs)
        assert last_diff() == (7, dl.FORM_GRID)
        assert runs.total() == 0
        # ... and the re-twin of a release past its own 65 536-page sweep
        c.upload("twin", t)
        teach(c, n, TEACH["D"])
        c.release(out=runs)
        assert last_diff() == (7, dl.FORM_GRID)
        check_stream(runs, ro, data, "release with re-twin")
        assert np.array_equal(c.download("twin"), cur)


def test_every_pair_of_hint_and_data(cases):
    """(a) One context of 33 037 pages (516 64-page units + 13 pages, 2064 16-page units + 13: in
    both geometries the last workgroup has one live wave and the last unit is partial) walks 17
    CURRENT uploads: no hint first, then every ordered pair (class whose total set the hint,
    class being diffed) over S, M, D, X. A stale hint must cost time only."""
    n = dl.N_WALK
    t = cases("S", n)[0]
    cap = max(int(cases(k, n)[2][-1]) for k in dl.CLASSES) + 4096
    seen = set()
    with ga.Context(n) as c:
        c.upload("twin", t)
        runs = Runs(c, n, cap=cap)
        prev_cls, prev_total = None, None
        for step, cls in enumerate(dl.HINT_WALK):
            _, cur, ro, data = cases(cls, n)
            c.upload("current", cur)
            c.diff(out=runs)
            want = dl.expected_variant(dl.hint_of(prev_total, n))
            what = f"step {step}: class {cls} under the hint of {prev_cls} (variant {want})"
            assert last_diff() == (want, dl.FORM_GRID), what
            check_stream(runs, ro, data, what)
            seen.add((want if prev_cls else 0, cls))
            prev_cls, prev_total = cls, int(ro[-1])
    # every class under the unknown hint's successor geometries: 64 pages with the slot, 16
    # pages without, 16 pages with the slot
    assert {(v, k) for v in (5, 1, 7) for k in dl.CLASSES} <= seen and (0, "S") in seen


@pytest.mark.parametrize("hint", [1, dl.DENSE64, dl.DENSE64 + 1, dl.DENSE16, dl.DENSE16 + 1])
def test_thresholds_of_the_automatic_table(hint, cases):
    """The table itself at its edges, on the first long list: hint <= 112 -> variant 5,
    113 .. 480 -> 1, beyond -> 7."""
    n = dl.N_LENGTHS[0]
    t, cur, ro, data = cases("X", n)
    with ga.Context(n) as c:
        c.upload("twin", t)
        c.upload("current", cur)
        teach(c, n, hint)
        runs = c.diff(cap=int(ro[-1]) + 4096)
        want = 5 if hint <= 112 else 1 if hint <= 480 else 7
        assert want == dl.expected_variant(hint)
        assert last_diff() == (want, dl.FORM_GRID)
        assert runs.total() == int(ro[-1])


@pytest.mark.parametrize("hint", ["S", "M", "D"])
@pytest.mark.parametrize("n", dl.N_LENGTHS)
def test_first_long_lengths(n, hint, cases):
    """(b) 32 769 pages (the first long list: its last unit has one page) and 33 024 (a multiple
    of every unit and workgroup size), class X under each of the three hints."""
    t, cur, ro, data = cases("X", n)
    with ga.Context(n) as c:
        c.upload("twin", t)
        c.upload("current", cur)
        teach(c, n, TEACH[hint])
        runs = c.diff(cap=int(ro[-1]) + 4096)
        assert last_diff() == (VARIANT[hint], dl.FORM_GRID)
        check_stream(runs, ro, data, f"n = {n}, hint {hint}")


@pytest.mark.parametrize("hint", ["S", "M", "D"])
def test_fused_apply_lists_and_retwin(hint, cases):
    """(c) 33 037 pages of class X under each hint: gdsm_diff_apply_ids with a permuted list and
    another permuted target list into a REPLICA unlike the twin; gdsm_release with re-twin, with
    room for every record and with room for about half the stream (TWIN := CURRENT exactly for
    the pages whose record ended inside the capacity; the total then reports -ENOSPC)."""
    n = dl.N_WALK
    rng = np.random.default_rng(33)
    cases.lists.setdefault("perm_walk", rng.permutation(n).astype(np.uint32))
    ids = cases.lists["perm_walk"]
    tids = np.random.default_rng(34).permutation(n).astype(np.uint32)
    t, cur, ro, data = cases("X", n, ids="perm_walk")
    total = int(ro[-1])
    replica0 = np.ascontiguousarray(t[::-1])
    want_rep = replica0.copy()
    assert oracle.apply(want_rep, ro, data, ids=tids) == 0
    v = (VARIANT[hint], dl.FORM_GRID)
    with ga.Context(n) as c:
        c.upload("twin", t)
        c.upload("current", cur)
        c.upload("replica", replica0)
        d_ids, d_tids = c.ids(ids), c.ids(tids)
        teach(c, n, TEACH[hint])
        runs = c.diff(d_ids, apply_to="replica", target_ids=d_tids, cap=total + 4096)
        assert last_diff() == v
        check_stream(runs, ro, data, "diff_apply_ids")
        assert np.array_equal(c.download("replica"), want_rep)
        assert np.array_equal(c.download("twin"), t)

        teach(c, n, TEACH[hint])
        c.release(d_ids, out=runs)
        assert last_diff() == v
        check_stream(runs, ro, data, "release, room for every record")
        assert np.array_equal(c.download("twin"), cur)

        c.upload("twin", t)
        half = Runs(c, n, cap=total // 2)
        teach(c, n, TEACH[hint])
        c.release(d_ids, out=half)
        assert last_diff() == v
        with pytest.raises(GdsmError) as ei:
            half.total()
        assert ei.value.errno == errno.ENOSPC
        got_ro = np.empty(n + 1, np.uint64)
        L = _lib.load()
        assert L.gdsm_memcpy_d2h(c.handle, got_ro.ctypes.data, half.s.rec_off, got_ro.nbytes) == 0
        assert np.array_equal(got_ro, ro)
        stored = ro[1:] <= half.cap
        assert 0.4 * n < stored.sum() < 0.6 * n
        fit = int(ro[1:][stored].max())
        part = np.empty(fit, np.uint8)
        assert L.gdsm_memcpy_d2h(c.handle, part.ctypes.data, half.s.data, fit) == 0
        dl.assert_stream_equal(ro[:stored.sum() + 1], part, ro[:stored.sum() + 1], data, "stored")
        want_twin = t.copy()
        want_twin[ids[stored]] = cur[ids[stored]]
        assert np.array_equal(c.download("twin"), want_twin)
        assert np.array_equal(c.download("current"), cur)


@pytest.mark.parametrize("variant", [4, 2, 1])
@pytest.mark.parametrize("cls", ["S", "X"])
def test_raw_entry_point_without_a_spill_pool(cls, variant, cases):
    """(e) gdsm_diff_raw of 33 037 pages with the workspace of a 32 768-page list: the status
    granules fit, a spill pool does not, so the capacity per page picks 64, 32 or 16 pages per
    wave without a slot. rec_off is complete, the data equal below min(cap, total) (the capacity
    is put at the end of a record), and every byte past it keeps its guard pattern."""
    n = dl.N_WALK
    t, cur, ro, data = cases(cls, n)
    total = int(ro[-1])
    ask = {4: 128 * n, 2: 384 * n, 1: 1000 * n}[variant]
    cap = ask if total <= ask else int(ro[ro <= ask].max())
    assert dl.raw_variant(cap, n) == variant
    fit = min(cap, total)
    L = _lib.load()
    with ga.Context(n, arenas=("twin", "current")) as c:
        c.upload("twin", t)
        c.upload("current", cur)
        ws_bytes = L.gdsm_diff_workspace_bytes(dl.DIFF_SHORT)
        assert ws_bytes < L.gdsm_diff_workspace_bytes(n) - 4 * dl.SPILL_SLOT
        ws = c.buffer(ws_bytes)
        ro_buf = c.buffer((n + 1) * 8).upload(np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64))
        alloc = cap + 4096
        data_buf = c.buffer(alloc).upload(np.full(alloc, GUARD, np.uint8))
        rc = L.gdsm_diff_raw(c.arena_ptr("twin"), c.arena_ptr("current"), None, n, ro_buf.ptr,
                             data_buf.ptr, cap, ws.ptr, ws_bytes, c.stream)
        assert rc == 0
        assert last_diff() == (variant, dl.FORM_GRID)
        c.sync()
        got_ro = ro_buf.download(np.uint64, n + 1)
        got = data_buf.download(np.uint8, alloc)
        kept = int(np.searchsorted(ro, fit, side="right")) - 1  # records that end inside cap
        assert np.array_equal(got_ro, ro), dl.first_stream_difference(got_ro, got, ro, data)
        dl.assert_stream_equal(ro[:kept + 1], got, ro[:kept + 1], data, f"{cls}, variant {variant}")
        assert int(ro[kept]) == fit
        assert (got[fit:] == GUARD).all()


def _without(ro, data, i):
    """The stream (ro, data) without record i."""
    ro = np.asarray(ro, np.uint64)
    a, b, end = int(ro[i]), int(ro[i + 1]), int(ro[-1])
    off = np.concatenate([ro[:i + 1], ro[i + 2:] - np.uint64(b - a)])
    return off, np.concatenate([data[:a], data[b:end]])


def test_caller_lists_longer_than_one_sweep_of_the_check():
    """(f) gdsm_diff with a list of 262 144 + 300 entries (repeats) over a 2048-page context: the
    prep kernel's check goes round its grid-stride loop. Then one entry >= n_pages planted past
    position 262 144: the next sync fails with EINVAL, every other record is unchanged, and
    apply and twin over the list touch the listed pages and the guard page only."""
    n, m = dl.N_IDS_CTX, dl.N_IDS_LIST
    t, cur = dl.pages("S", n)
    listed = np.flatnonzero(np.arange(n) % 7 != 3)
    rest = np.setdiff1d(np.arange(n), listed)
    ids = np.random.default_rng(262).choice(listed, m).astype(np.uint32)
    assert len(np.unique(ids)) == len(listed)
    ro, data = oracle.diff_pages(t, cur, ids=ids, cap=128 << 20)
    total = int(ro[-1])
    assert total < 128 << 20
    bad_at = 262144 + 150
    bad = ids.copy()
    bad[bad_at] = n
    with ga.Context(n) as c:
        c.upload("twin", t)
        c.upload("current", cur)
        c.upload("replica", t)
        runs = c.diff(c.ids(ids), cap=total + 4096)
        assert last_diff() == (5, dl.FORM_GRID)
        c.sync()
        check_stream(runs, ro, data, "long list")

        d_bad = c.ids(bad)
        runs2 = c.diff(d_bad, cap=total + 10244 + 4096)
        assert last_diff()[1] == dl.FORM_GRID
        with pytest.raises(GdsmError) as ei:
            c.sync()
        assert ei.value.errno == errno.EINVAL
        host = runs2.to_host()
        dl.assert_stream_equal(*_without(host.rec_off, host.data, bad_at),
                               *_without(ro, data, bad_at), "the other entries")
        for apply in (c.apply, c.apply_async):
            c.upload("replica", t)
            apply(runs2, "replica", d_bad)
            with pytest.raises(GdsmError):
                c.sync()
            rep = c.download("replica")
            assert np.array_equal(rep[listed], cur[listed]) and np.array_equal(rep[rest], t[rest])
        c.twin(d_bad)
        with pytest.raises(GdsmError):
            c.sync()
        tw = c.download("twin")
        assert np.array_equal(tw[listed], cur[listed]) and np.array_equal(tw[rest], t[rest])
        assert np.array_equal(c.download("current"), cur)
        c.sync()  # the error word was cleared
