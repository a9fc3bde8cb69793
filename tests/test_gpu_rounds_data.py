"""gdsm_rounds' page-data side (rounds_data_kernel: the fused row writes, the release of the
round's pages, the home apply and the re-twin, round after round in one persistent launch) against
the host model tests/rounds_model.py, i.e. the C oracle's diff round by round: every trace is run
at several prefix lengths on fresh contexts, so that no later round hides an earlier round's
stream, and TWIN, CURRENT, REPLICA and the stream are compared bit for bit. The page-table side
gets empty rounds (tests/test_gpu_rounds_fold.py is its oracle check), except where both sides'
state is carried across calls. tests/test_rounds_model.py checks the model and the traces on the
CPU.

Launch forms: a call whose largest round has <= 32 pages runs on a one-XCD team by default, a
larger one on the whole grid; gdsm_tune "rounds_xcd" 0 / 1 forces the form. The edges, hand-off,
sizes-small and mmult traces run with the key at -1 (automatic: the team), 0 and 1; sizes-large
with it at -1 (the whole grid: its 33- to 2048-page rounds are past the team's domain; rounds of
more than 256 pages make a workgroup release several pages per round)."""
import errno
import functools

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd.gdsm import check, lib
from oracle import oracle
from tests import rounds_model as rm
from tests.helpers import tune, zipf_counts  # noqa: F401  (tune: fixture)

pytestmark = pytest.mark.gpu

XCD = [None, "0", "1"]
ARENAS = ("twin", "current", "replica")


def _set_xcd(tune, xcd):
    """gdsm_tune "rounds_xcd": None = -1 (automatic), "0" = the whole grid, "1" = the team."""
    tune(rounds_xcd=-1 if xcd is None else int(xcd))


@functools.lru_cache(maxsize=None)
def _trace(name):
    return {"edges": rm.edges_trace, "hand-off": rm.handoff_trace,
            "sizes-small": rm.sizes_small_trace, "sizes-large": rm.sizes_large_trace}[name]()


PREFIXES = {"edges": range(1, 9), "hand-off": (1, 2, 17, 300), "sizes-small": range(1, 7),
            "sizes-large": range(1, 9)}


@functools.lru_cache(maxsize=None)
def _wants(name):
    """{k: the model's state after round k - 1}, computed once per trace (the small traces)."""
    keep = set(PREFIXES[name])
    return {k: rm.State(st.twin.copy(), st.cur.copy(), st.rep.copy(), st.rec_off, st.data)
            for k, st in enumerate(rm.replay(_trace(name)), 1) if k in keep}


def _assert_equal(got, want, what):
    """got: rm.DeviceRun; want: rm.State."""
    assert got.n == len(want.rec_off) - 1, what
    assert np.array_equal(got.rec_off, want.rec_off), (what, np.flatnonzero(got.rec_off != want.rec_off)[:8])
    assert len(got.data) == len(want.data), what
    assert np.array_equal(got.data, want.data), (what, np.flatnonzero(got.data != want.data)[:8])
    for a in ("cur", "rep", "twin"):
        g, w = getattr(got, a), getattr(want, a)
        assert np.array_equal(g, w), (what, a, np.argwhere(g != w)[:8])


@pytest.mark.parametrize("xcd", XCD)
@pytest.mark.parametrize("name", ["edges", "hand-off", "sizes-small"])
def test_rounds_data_matches_model_at_every_prefix(name, xcd, tune):
    """edges: every prefix of the 8 edge-case rounds (rounds_model.edges_trace: clean and
    pre-dirtied entries, half-chunk and zero-byte descriptors, runs across the waves' quarter
    edges, a descriptor over three pages, a full and a maximum-size record, two views to one home
    page, empty first / middle / last rounds). hand-off: 1, 2, 17 and 300 rounds on the same three
    pages, the list rotated every round. sizes-small: every prefix of rounds of 1, 32, 0, 17, 31
    and 2 pages."""
    _set_xcd(tune, xcd)
    t, wants = _trace(name), _wants(name)
    for k in PREFIXES[name]:
        got = rm.run_prefix(t, k)
        _assert_equal(got, wants[k], (name, k))
        if not len(t.rounds[k - 1].ids):  # after an empty last round: no records, no bytes
            assert got.n == 0 and got.rec_off.tolist() == [0] and len(got.data) == 0
        if name == "edges" and k == 5:  # the alternating page's record: GDSM_MAX_RECORD bytes
            assert int(np.diff(got.rec_off)[1]) == ga.gdsm.MAX_RECORD == 10244


def test_rounds_data_large_rounds_match_model_at_every_prefix(tune):
    """sizes-large: rounds of 1, 33, 0, 257, 32, 2048, 5 and 256 pages on a 4096-page arena, every
    prefix: the whole grid chosen automatically (> 32 pages), one workgroup releasing several
    pages of a round and looking back across its own iterations (> 256 pages), the 2048-page
    limit."""
    _set_xcd(tune, None)
    t = _trace("sizes-large")
    for k, want in enumerate(rm.replay(t), 1):
        _assert_equal(rm.run_prefix(t, k), want, ("sizes-large", k))


def _mmult_trace(R):
    """The model trace of an MmultReplay's device arrays (its descriptors are absolute addresses:
    CURRENT's arena + dst, d_rows + off)."""
    n_ids, n_desc = int(R.id_off[-1]), int(R.desc_off[-1])
    ids = R.d_ids.download(np.uint32, n_ids)
    home = R.d_home.download(np.uint32, n_ids)
    desc = R.d_desc.download(np.uint64, 3 * n_desc).reshape(-1, 3)
    dst = desc[:, 0] - np.uint64(R.data.arena_ptr("current"))
    off = desc[:, 1] - np.uint64(R.d_rows.ptr)
    t = rm.Trace("mmult", R.data.download("twin"), R.data.download("current"),
                 R.data.download("replica"), R.d_rows.download(np.uint8, R.d_rows.nbytes))
    for r in range(R.T.rounds):
        a, b = int(R.id_off[r]), int(R.id_off[r + 1])
        d0, d1 = R.desc_off[r], R.desc_off[r + 1]
        t.rounds.append(rm.Round(ids[a:b], home[a:b],
                                 [(int(dst[d]), int(off[d]), int(desc[d, 2])) for d in range(d0, d1)]))
    return t


@pytest.mark.parametrize("xcd", XCD)
@pytest.mark.parametrize("ndim,nodes", [(64, 1), (257, 3), (64, 8)])
def test_mmult_device_rounds_match_model(ndim, nodes, xcd, tune):
    """Config 5's trace (MmultReplay, driver="device") as a model trace: after run(), the last
    round's stream, TWIN, CURRENT and the home copy equal the model's (the oracle's diff of every
    round), not only those of another HIP path."""
    from gallocy_amd.replay import MmultReplay
    _set_xcd(tune, xcd)
    R = MmultReplay(ndim=ndim, nodes=nodes, seed=11, driver="device")
    try:
        t = _mmult_trace(R)
        assert rm.contract_violations(t) == []
        R.run()
        got = rm.download_run(R.data, R._runs)
        want = rm.model(t, R.T.rounds)
        _assert_equal(got, want, ("mmult", ndim, nodes))
        assert np.array_equal(R.home_copy(), want.rep[:R.Z].reshape(-1))
        assert int(want.rec_off[-1]) > 0  # the last round ships records
    finally:
        R.close()


# ---------------------------------------------------------------- state carried across calls
def _events(n_pages, n_ev, n_nodes, seed):
    counts = zipf_counts(n_pages, n_ev, s=0.9, seed=seed) if n_ev else np.zeros(n_pages, np.int64)
    return oracle.gen_events(counts, seed=seed + 1, n_nodes=n_nodes, write_pct=30)


def test_rounds_interleaved_with_release_and_coherence_batches():
    """One pair of contexts: gdsm_release of 5 pages, gdsm_rounds (3 rounds, with events),
    gdsm_release of 40 pages (the chained form, which shares the look-back chain and its epoch
    with gdsm_rounds), gdsm_rounds again; on the page-table context gdsm_coherence_batch before,
    between and after. Every step's stream and arenas against oracle.diff_pages / the model, the
    page table and totals against oracle.coherence."""
    n, n_pt, nodes = 64, 100, 4
    rng = np.random.default_rng(77)
    b0 = rm.TraceBuilder.fresh("carry", n, seed=7, dirty=rng.choice(n, 20, replace=False))
    tw, cu, rp = b0.t.twin, b0.t.cur, b0.t.rep
    perm = rm.shifted_perm(rng, n)
    st, fl = oracle.coh_init(n_pt, nodes)

    def host_release(ids):
        ids = np.asarray(ids, np.int64)
        rec = oracle.diff_pages(tw, cu, ids.astype(np.uint32))
        for p in ids:
            m = tw[p] != cu[p]
            rp[perm[p]][m] = cu[p][m]
        tw[ids] = cu[ids]
        return rec

    with ga.Context(n) as d, ga.Context(n_pt, arenas=()) as pt:
        pt.coh_init(nodes)
        for a, h in zip(ARENAS, (tw, cu, rp)):
            d.upload(a, h)

        def check_arenas(what):
            for a, h in zip(ARENAS, (tw, cu, rp)):
                assert np.array_equal(d.download(a), h), (what, a)

        def release(ids, what):
            runs = d.release(d.ids(ids), apply_to="replica", target_ids=d.ids(perm[ids]))
            h = runs.to_host()
            ro, data = host_release(ids)
            assert np.array_equal(h.rec_off, ro) and np.array_equal(h.data, data), what
            assert int(ro[-1]) > 0, what
            check_arenas(what)
            runs.free()

        def batch(seed):
            ev = _events(n_pt, 700, nodes, seed)
            rc, want = oracle.coherence(st, fl, ev, n_nodes=nodes)
            assert rc == 0 and pt.coherence_batch(ev) == want
            gst, gfl = pt.coh_download()
            assert np.array_equal(gst, st) and np.array_equal(gfl, fl)

        def rounds(sizes, seed, what):
            nonlocal tw, cu, rp
            b = rm.TraceBuilder(what, tw, cu, rp, seed)
            for m in sizes:
                ids = rng.choice(n, m, replace=False)
                rm.random_round(b, rng, ids, perm[ids])
            t = b.build()
            k = len(sizes)
            evs = [_events(n_pt, e, nodes, seed + 10 * i) for i, e in enumerate((900, 0, 300))]
            runs = ga.Runs(d, max(sizes), cap=max(sizes) * rm.MAX_RECORD)
            rc, keep = rm.issue_rounds(d, pt, t, k, runs, events=evs)
            check(rc, "gdsm_rounds")
            d.sync()
            pt.sync()
            want = rm.model(t, k)
            _assert_equal(rm.download_run(d, runs), want, what)
            tw, cu, rp = want.twin, want.cur, want.rep
            tots = []
            for ev in evs:
                rc, w = oracle.coherence(st, fl, ev, n_nodes=nodes)
                assert rc == 0
                tots.append([w["invalidations"], w["transfers"], *w["node_faults"]])
            got = keep[-1].download(np.uint64, 10 * k).reshape(k, 10)
            assert np.array_equal(got, np.array(tots, np.uint64)), what
            gst, gfl = pt.coh_download()
            assert np.array_equal(gst, st) and np.array_equal(gfl, fl), what
            runs.free()

        batch(1)
        release(np.array([3, 60, 17, 9, 33]), "release of 5")
        rounds((6, 0, 12), 31, "rounds after the short release")
        batch(2)
        dirty = rng.choice(n, 40, replace=False)
        for p in dirty:  # the application writes between the calls
            m = rng.random(4096) < 0.05
            cu[p, m] ^= rng.integers(1, 256, int(m.sum()), dtype=np.uint8)
        d.upload("current", cu)
        release(dirty, "chained release of 40")
        rounds((9, 33, 2), 32, "rounds after the chained release")
        release(rng.choice(n, 24, replace=False), "chained release after the rounds")
        batch(3)


# ------------------------------------------------------------------- refused or reported
def _edges_contexts():
    t = _trace("edges")
    d, pt = ga.Context(t.n_pages), ga.Context(4, arenas=())
    pt.coh_init(2)
    for a, h in zip(ARENAS, (t.twin, t.cur, t.rep)):
        d.upload(a, h)
    return t, d, pt


@pytest.mark.parametrize("case", ["2049-pages", "n_cap", "cap"])
def test_rounds_rejected_before_anything_runs(case):
    """A round of 2049 pages, a stream with fewer records (n_cap) than the largest round, or
    with fewer bytes than that round's pages * GDSM_MAX_RECORD (a middle round overflowing cap
    would leave its pages dirty with nothing to report it): -EINVAL from the call, the arenas
    untouched, and nothing pending for gdsm_sync."""
    t, d, pt = _edges_contexts()
    try:
        k = len(t.rounds)
        if case == "2049-pages":
            ids = (np.arange(2049) % t.n_pages).astype(np.uint32)
            t = rm.Trace("big", t.twin, t.cur, t.rep, t.src, [rm.Round(ids, ids, [])])
            k = 1
            runs = ga.Runs(d, 2049, cap=2049 * rm.MAX_RECORD)
            # (2048 such entries are accepted: the limit itself runs in sizes-large)
        elif case == "n_cap":
            runs = ga.Runs(d, 5, cap=6 * rm.MAX_RECORD)
        else:
            runs = ga.Runs(d, 6, cap=6 * rm.MAX_RECORD)
            runs.s.cap = 6 * rm.MAX_RECORD - 1
        rc, _keep = rm.issue_rounds(d, pt, t, k, runs)
        assert rc == -errno.EINVAL
        assert lib().gdsm_sync(d.handle) == 0 and lib().gdsm_sync(pt.handle) == 0
        for a, h in zip(ARENAS, (t.twin, t.cur, t.rep)):
            assert np.array_equal(d.download(a), h), a
        if case == "cap":  # one byte more and the same call runs
            runs.s.cap = 6 * rm.MAX_RECORD
            rc, _keep = rm.issue_rounds(d, pt, t, k, runs)
            assert rc == 0 and lib().gdsm_sync(d.handle) == 0 and lib().gdsm_sync(pt.handle) == 0
        runs.free()
    finally:
        d.close()
        pt.close()


def test_rounds_overlapping_descriptors_are_reported_at_the_sync():
    """Two descriptors of one round that cover the same 8-B word: -EINVAL from gdsm_sync on the
    data context (the round's words laid fall short of the words its descriptors hold), and the
    next sync is clean."""
    t, d, pt = _edges_contexts()
    try:
        P = rm.PAGE
        good = t.rounds[1]
        bad = rm.Round(np.array([9, 10], np.uint32), np.array([3, 4], np.uint32),
                       [(9 * P + 64, 0, 64), (9 * P + 120, 64, 16), (10 * P, 128, 8)])
        t2 = rm.Trace("overlap", t.twin, t.cur, t.rep, t.src, [good, bad, good])
        assert rm.contract_violations(t2) == ["round 1: overlapping descriptors"]
        runs = ga.Runs(d, 6, cap=6 * rm.MAX_RECORD)
        rc, _keep = rm.issue_rounds(d, pt, t2, 3, runs)
        assert rc == 0
        assert lib().gdsm_sync(d.handle) == -errno.EINVAL
        assert lib().gdsm_sync(pt.handle) == 0
        assert lib().gdsm_sync(d.handle) == 0  # the error word was cleared
        runs.free()
    finally:
        d.close()
        pt.close()


@pytest.mark.parametrize("bad_id", [rm.EDGES_PAGES, 0xFFFFFFFF])
@pytest.mark.parametrize("where", ["ids", "home"])
def test_rounds_out_of_range_ids_touch_no_unlisted_page_and_fail(where, bad_id):
    """An id >= n_pages among a middle round's ids, or among its home pages: it goes to the
    arenas' guard page (as test_out_of_range_page_ids_touch_no_listed_page_and_fail pins for
    gdsm_diff), gdsm_sync reports -EINVAL, no page that no round lists changes in any arena, and
    the next sync is clean. A bad home page touches REPLICA alone: TWIN and CURRENT equal the
    model's."""
    t, d, pt = _edges_contexts()
    try:
        r1, r2, r4 = t.rounds[1], t.rounds[2], t.rounds[4]
        ids, home = r2.ids.copy(), r2.home.copy()
        (ids if where == "ids" else home)[1] = bad_id
        if where == "ids":  # page 7's part of the three-page descriptor goes with its entry
            dst, so, nb = r2.desc[0]
            desc = [(dst, so, 7 * rm.PAGE - dst)] + r2.desc[1:]
        else:
            desc = r2.desc
        t2 = rm.Trace("bad", t.twin, t.cur, t.rep, t.src, [r1, rm.Round(ids, home, desc), r4])
        runs = ga.Runs(d, 6, cap=6 * rm.MAX_RECORD)
        rc, _keep = rm.issue_rounds(d, pt, t2, 3, runs)
        assert rc == 0
        assert lib().gdsm_sync(d.handle) == -errno.EINVAL
        assert lib().gdsm_sync(pt.handle) == 0
        assert lib().gdsm_sync(d.handle) == 0
        n = t.n_pages
        all_ids = np.concatenate([r.ids for r in t2.rounds])
        all_home = np.concatenate([r.home for r in t2.rounds])
        free_v = np.setdiff1d(np.arange(n), all_ids[all_ids < n])
        free_h = np.setdiff1d(np.arange(n), all_home[all_home < n])
        got = {a: d.download(a) for a in ARENAS}
        assert np.array_equal(got["twin"][free_v], t.twin[free_v])
        assert np.array_equal(got["current"][free_v], t.cur[free_v])
        assert np.array_equal(got["replica"][free_h], t.rep[free_h])
        if where == "home":
            ok = rm.Trace("ok", t.twin, t.cur, t.rep, t.src, [r1, r2, r4])
            want = rm.model(ok, 3)
            assert np.array_equal(got["twin"], want.twin)
            assert np.array_equal(got["current"], want.cur)
            # the last round's stream does not depend on the bad entry's home page
            h = runs.to_host()
            assert np.array_equal(h.rec_off, want.rec_off) and np.array_equal(h.data, want.data)
        runs.free()
    finally:
        d.close()
        pt.close()
