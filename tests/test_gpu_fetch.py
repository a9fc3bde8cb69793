"""gdsm_fetch and gdsm_notices_fetch_list on ONE GPU (docs/SPEC.md §9): G ranks as threads, each
with its own context on cuda:0, wired by the loopback communicator. Every context has Z pages in all
three arenas with distinct random contents per rank and arena; exact bytes are compared throughout
against the numpy model tests/fetch_model.py: the named arenas after a fetch, everything that must
not change, the ordering after gdsm_exchange, the collective refusals, the notice filter, and one
protocol run fault -> notices -> fetch -> write -> release -> fetch against the oracle's page table."""
import ctypes as C
import errno
import threading

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import exchange
from oracle import oracle
from tests import fetch_model as fm

pytestmark = pytest.mark.gpu

ARENAS = ("twin", "current", "replica")


def run_ranks(G, fn):
    errs = [None] * G

    def body(r):
        try:
            fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e
    th = [threading.Thread(target=body, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=110)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    for e in errs:
        if e is not None:
            raise e


class Group:
    """G data contexts of Z pages, every arena filled with its own random bytes (host mirror in
    .host[r][arena]), and their loopback communicators."""

    def __init__(self, G, Z, seed):
        rng = np.random.default_rng(seed)
        self.G, self.Z = G, Z
        self.ctxs = [ga.Context(Z) for _ in range(G)]
        self.host = []
        for c in self.ctxs:
            h = {a: rng.integers(0, 256, (Z, 4096), dtype=np.uint8) for a in ARENAS}
            for a in ARENAS:
                c.upload(a, h[a])
            self.host.append(h)
        self.comms = exchange.Comm.loopback(self.ctxs)

    def download(self):
        return [{a: c.download(a) for a in ARENAS} for c in self.ctxs]

    def assert_unchanged(self):
        for r, now in enumerate(self.download()):
            for a in ARENAS:
                assert np.array_equal(now[a], self.host[r][a]), (r, a)

    def close(self):
        for c in self.comms:
            c.close()
        for c in self.ctxs:
            c.close()


def raw_fetch(grp, r, pages, dst, total, src=ga.REPLICA, mask=0, ctx=None):
    """gdsm_fetch on rank r with host lists (uploaded here); returns the return code."""
    ctx = ctx or grp.ctxs[r]
    pb = ctx.ids(pages) if len(pages) else None
    db = ctx.ids(dst) if dst is not None and len(dst) else None
    rc = ga.gdsm.lib().gdsm_fetch(ctx.handle, grp.comms[r].handle, pb.ptr if pb else None,
                                  db.ptr if db else None, len(pages), total, src, mask)
    ctx.sync()
    for b in (pb, db):
        if b is not None:
            b.free()
    return rc


def request_of(role, rng, r, G, Z):
    """One rank's ascending request list by role (see test_fetch_equals_model)."""
    edges = []
    for h in range(G):
        base, n = fm.block_of(h, Z, G)
        if n:
            edges += [base, base + n - 1]
    if role == 0:    # a random subset plus the first and last page of every block
        pick = rng.choice(Z, max(1, Z // 3), replace=False)
        return np.unique(np.concatenate([pick, edges])).astype(np.uint32)
    if role == 1:    # nothing
        return np.zeros(0, np.uint32)
    if role == 2:    # every page
        return np.arange(Z, dtype=np.uint32)
    if role == 3:    # only pages homed at itself
        base, n = fm.block_of(r, Z, G)
        return np.arange(base, base + n, dtype=np.uint32)
    k = {4: 1, 5: 3, 6: 257}.get(role, max(1, Z // 2))
    return np.sort(rng.choice(Z, min(k, Z), replace=False)).astype(np.uint32)


@pytest.mark.parametrize("G,Z", [(1, 37), (2, 130), (3, 1025), (4, 777), (8, 1031), (8, 5)])
def test_fetch_equals_model(G, Z):
    """Four fetches in a row on the same contexts (dst_ids NULL / a random injective map, both
    arenas / CURRENT only); the ranks' roles rotate from one to the next, so every shape sees an
    empty list, every page, own pages only, block edges, and list lengths 1, 3 and 257."""
    rng = np.random.default_rng(100 * G + Z)
    grp = Group(G, Z, seed=G * 7919 + Z)
    try:
        for v, (with_dst, names) in enumerate([(False, ("current", "twin")), (False, ("current",)),
                                               (True, ("current", "twin")), (True, ("current",))]):
            reqs = [request_of((r + v) % 8, rng, r, G, Z) for r in range(G)]
            dsts = [rng.permutation(Z)[:len(q)].astype(np.uint32) if with_dst else None
                    for q in reqs]
            for r in range(G):
                assert fm.valid_request(reqs[r], dsts[r], Z, Z)
            rep = [h["replica"] for h in grp.host]
            want = fm.fetch(rep, reqs, dsts, [{a: h[a] for a in names} for h in grp.host], Z)
            bufs = [(c.ids(reqs[r]), c.ids(dsts[r]) if with_dst else None)
                    for r, c in enumerate(grp.ctxs)]

            def rank(r):
                pb, db = bufs[r]
                exchange.fetch(grp.ctxs[r], grp.comms[r], pb if len(reqs[r]) else None,
                               db if with_dst and len(reqs[r]) else None, len(reqs[r]), Z,
                               dst=names)
                grp.ctxs[r].sync()
            run_ranks(G, rank)
            now = grp.download()
            for r in range(G):
                for a in ARENAS:
                    exp = want[r][a] if a in names else grp.host[r][a]
                    assert np.array_equal(now[r][a], exp), (v, r, a)
                    grp.host[r][a] = exp
                if len(reqs[r]) and len(names) == 2:
                    d = reqs[r] if dsts[r] is None else dsts[r]
                    ids = grp.ctxs[r].ids(d)
                    out = grp.ctxs[r].diff(ids, n=len(d), cap=max(4096, 64 * len(d)))
                    assert out.total() == 0, (v, r)  # fetched into both arenas: clean pages
                    out.free()
                    ids.free()
            for pb, db in bufs:
                pb.free()
                if db is not None:
                    db.free()
    finally:
        grp.close()


def test_fetch_is_ordered_after_exchange():
    """Every rank diffs one changed page per home and gdsm_exchange ships it; with no sync in
    between, every rank fetches the page that rank 0 patched at home 1: the bytes are the
    post-exchange ones."""
    G, Z = 2, 16
    grp = Group(G, Z, seed=3)
    try:
        per = fm.per_of(Z, G)
        # home d's REPLICA page r starts as writer r's TWIN page 3, so the patch makes it r's CURRENT 3
        for d in range(G):
            for r in range(G):
                grp.ctxs[d].upload("replica", grp.host[r]["twin"][3:4], first=r)
                grp.host[d]["replica"][r] = grp.host[r]["twin"][3]
        target = 1 * per + 0  # global id of home 1's REPLICA page 0, patched by rank 0
        got = [None] * G

        def rank(r):
            ctx, comm = grp.ctxs[r], grp.comms[r]
            src = ctx.ids(np.array([3], np.uint32))
            sid = ctx.ids(np.array([r], np.uint32))
            send = [ctx.diff(src, n=1, cap=16384) for _ in range(G)]
            recv = [ga.Runs(ctx, 4, cap=16384) for _ in range(G)]
            rids = [ctx.buffer(16) for _ in range(G)]
            pg = ctx.ids(np.array([target], np.uint32))
            dst = ctx.ids(np.array([7], np.uint32))
            exchange.exchange_runs(ctx, comm, send, [sid.ptr] * G, recv, [b.ptr for b in rids])
            exchange.fetch(ctx, comm, pg, dst, 1, Z)   # no sync since the diff
            ctx.sync()
            got[r] = ctx.download("current", 7, 1)[0]
        run_ranks(G, rank)
        assert not np.array_equal(grp.host[0]["current"][3], grp.host[0]["twin"][3])
        for r in range(G):
            assert np.array_equal(got[r], grp.host[0]["current"][3]), r
    finally:
        grp.close()


def test_fetch_refusals_are_collective():
    """A fault on ONE rank refuses the fetch on every rank, nothing moves, and the communicators
    work afterwards: a workspace growth that fails (-ENOMEM there, -ECANCELED elsewhere), then
    -EINVAL everywhere for a duplicate id, a descending pair, a page == total_pages, a destination
    == n_pages and a home context smaller than its block."""
    G, Z = 3, 96
    grp = Group(G, Z, seed=11)
    small = ga.Context(10)  # rank 1's block has 32 pages
    lib = ga.gdsm.lib()
    try:
        good = [np.array([1, 40, 70], np.uint32), np.array([0, 95], np.uint32),
                np.array([33, 34, 35, 64], np.uint32)]

        def case(lists, dsts=(None, None, None), total=Z, ctxs=(None, None, None)):
            rcs = [None] * G

            def rank(r):
                rcs[r] = raw_fetch(grp, r, lists[r], dsts[r], total, ctx=ctxs[r])
            run_ranks(G, rank)
            return rcs

        assert lib.gdsm_debug_fail_alloc(grp.ctxs[1].handle, 1) == 0
        assert case(good) == [-errno.ECANCELED, -errno.ENOMEM, -errno.ECANCELED]
        assert lib.gdsm_debug_fail_alloc(grp.ctxs[1].handle, 0) == 0
        grp.assert_unchanged()
        inval = [-errno.EINVAL] * G
        assert case([good[0], np.array([5, 5], np.uint32), good[2]]) == inval       # duplicate
        assert case([np.array([40, 1], np.uint32), good[1], good[2]]) == inval      # descending
        assert case([good[0], good[1], np.array([3, Z], np.uint32)]) == inval       # page == total
        assert case([good[0], good[1], np.array([3, Z], np.uint32)], total=Z + 1) == inval  # dst
        assert case(good, dsts=(None, np.array([2, Z], np.uint32), None)) == inval  # dst == n_pages
        before = small.download("current")
        assert case([good[0], np.zeros(0, np.uint32), good[2]], ctxs=(None, small, None)) == inval
        assert np.array_equal(small.download("current"), before)
        grp.assert_unchanged()
        # immediate refusals with real contexts (the same on every rank by construction)
        c0, m0 = grp.ctxs[0], grp.comms[0]
        ids = c0.ids(good[0])
        for args in [(ids.ptr, None, 3, 0, 2, 0), (ids.ptr, None, 3, (1 << 28) + 1, 2, 0),
                     (None, None, 3, Z, 2, 0), (ids.ptr, None, 3, Z, 3, 0),
                     (ids.ptr, None, 3, Z, -1, 0), (ids.ptr, None, 3, Z, 2, 4),
                     (ids.ptr, None, 3, Z, 1, 0), (ids.ptr, None, 3, Z, 0, 1)]:
            assert lib.gdsm_fetch(c0.handle, m0.handle, *args) == -errno.EINVAL, args
        pt = ga.Context(4, arenas=())
        assert lib.gdsm_fetch(pt.handle, m0.handle, ids.ptr, None, 3, Z, 2, 0) == -errno.EINVAL
        pt.close()
        # a valid fetch on the same communicators
        assert case(good) == [0, 0, 0]
        want = fm.fetch([h["replica"] for h in grp.host], good, [None] * G,
                        [{a: h[a] for a in ("current", "twin")} for h in grp.host], Z)
        now = grp.download()
        for r in range(G):
            for a in ("current", "twin"):
                assert np.array_equal(now[r][a], want[r][a]), (r, a)
            assert np.array_equal(now[r]["replica"], grp.host[r]["replica"])
    finally:
        small.close()
        grp.close()


def test_fetch_refuses_a_recording_context():
    """Both calls read a count back on the host, so a context that is recording a graph refuses
    them with -EBUSY, like the other synchronising calls; nothing is recorded or moved."""
    grp = Group(1, 8, seed=2)
    lib = ga.gdsm.lib()
    try:
        ctx, comm = grp.ctxs[0], grp.comms[0]
        ids = ctx.ids(np.array([1, 2], np.uint32))
        nt = ctx.buffer(16).upload(np.array([1, 2], np.uint64))
        k = C.c_uint64(5)
        ctx.capture_begin()
        try:
            assert lib.gdsm_fetch(ctx.handle, comm.handle, ids.ptr, None, 2, 8, 2, 0) == -errno.EBUSY
            assert lib.gdsm_notices_fetch_list(ctx.handle, nt.ptr, 2, 3, ids.ptr, 2,
                                               C.byref(k)) == -errno.EBUSY
        finally:
            ctx.capture_end().destroy()
        assert k.value == 5
        grp.assert_unchanged()
        assert raw_fetch(grp, 0, np.array([1, 2], np.uint32), None, 8) == 0
    finally:
        grp.close()


def random_notices(rng, n, mode="mixed"):
    """n notices in SPEC §5b packing, page-sorted, one per page."""
    pages = np.sort(rng.choice(1 << 20, n, replace=False)).astype(np.uint64)
    if mode == "all":       # every one a page gained for reading
        before, after = np.zeros(n, np.uint64), np.ones(n, np.uint64)
    elif mode == "none":    # upgrades and losses only
        before = rng.integers(1, 3, n).astype(np.uint64)
        after = rng.integers(0, 3, n).astype(np.uint64)
    else:
        before = rng.integers(0, 3, n).astype(np.uint64)
        after = rng.integers(0, 3, n).astype(np.uint64)
    ob = rng.integers(0, 8, n).astype(np.uint64)
    oa = rng.integers(0, 8, n).astype(np.uint64)
    return (pages | (before << np.uint64(32)) | (after << np.uint64(34)) | (ob << np.uint64(40))
            | (oa << np.uint64(48))).astype(np.uint64)


@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000, 70000])
def test_notices_fetch_list_equals_model(n):
    rng = np.random.default_rng(n + 1)
    lib = ga.gdsm.lib()
    with ga.Context(4, arenas=()) as ctx:
        out = ctx.buffer(4 * max(n, 1))
        for mode in ("mixed", "all", "none"):
            nt = random_notices(rng, n, mode)
            buf = ctx.buffer(8 * max(n, 1)).upload(nt)
            for want in (1, 2, 3):
                exp = fm.fetch_list(nt, want)
                k = exchange.notices_fetch_list(ctx, buf.ptr if n else None, n, want, out.ptr, n)
                assert k == len(exp), (mode, want)
                if mode == "all":
                    assert k == (n if want & 1 else 0)
                if mode == "none":
                    assert k == 0
                got = out.download(np.uint32, k) if k else np.zeros(0, np.uint32)
                assert np.array_equal(got, exp), (mode, want)
                if k:
                    assert (np.diff(got.astype(np.int64)) > 0).all()
                if k > 1:  # too small a list: the count needed comes back with -ENOSPC
                    need = C.c_uint64(0)
                    rc = lib.gdsm_notices_fetch_list(ctx.handle, buf.ptr, n, want, out.ptr, k - 1,
                                                     C.byref(need))
                    assert rc == -errno.ENOSPC and need.value == k
                    assert np.array_equal(out.download(np.uint32, k - 1), exp[:k - 1])
            buf.free()
        z = C.c_uint64(9)
        assert lib.gdsm_notices_fetch_list(ctx.handle, None, 0, 0, out.ptr, 1, C.byref(z)) == -22
        assert lib.gdsm_notices_fetch_list(ctx.handle, None, 0, 4, out.ptr, 1, C.byref(z)) == -22
        assert lib.gdsm_notices_fetch_list(ctx.handle, None, 3, 1, out.ptr, 1, C.byref(z)) == -22


def access_of(state, d):
    """Node d's access per page from SPEC §5 state words: 0 none, 1 read, 2 write."""
    w = np.asarray(state, np.uint32)
    st = (w >> 16) & 3
    held = (((w >> d) & 1) != 0) & (st != 0)
    own = (st == 2) & (((w >> 8) & 0xFF) == d)
    return np.where(held, np.where(own, 2, 1), 0)


def test_protocol_round_fault_notices_fetch_write_release():
    """G = 3 nodes, Z = 96 pages, 4 batches of stamped fault events (at most one writing node per
    page and batch; reads fall before or after the write). Per batch: route + notify on the
    page-table contexts; pages gained for writing are fetched; the nodes holding write access
    after the batch to a page they wrote change random bytes of it, diff, re-twin and release to
    the homes through gdsm_exchange; then pages gained for reading are fetched, with no sync since
    the exchange. After every batch, every node with access to a page holds the home's bytes in
    CURRENT, and both equal a numpy model of the contents."""
    G, Z = 3, 96
    rng = np.random.default_rng(42)
    per = fm.per_of(Z, G)
    data = Group(G, Z, seed=5)
    pts = []
    for r in range(G):
        base, nh = fm.block_of(r, Z, G)
        c = ga.Context(nh, arenas=())
        c.coh_init(G)
        c.coh_upload(np.full(nh, (1 << r) | (r << 8) | (2 << 16), np.uint32),
                     np.zeros(nh, np.uint32))
        pts.append(c)
    pt_comms = exchange.Comm.loopback(pts)
    gst, gfl = oracle.coh_init(Z, G)
    try:
        # initially every home node holds its block with write access: its copies are the contents
        model = np.concatenate([data.host[r]["replica"][:fm.block_of(r, Z, G)[1]]
                                for r in range(G)])
        for r in range(G):
            base, nh = fm.block_of(r, Z, G)
            for a in ("current", "twin"):
                data.ctxs[r].upload(a, model[base:base + nh], first=base)
        recv = [[ga.Runs(data.ctxs[r], Z, cap=Z * 10244) for _ in range(G)] for r in range(G)]
        rids = [[data.ctxs[r].buffer(4 * Z) for _ in range(G)] for r in range(G)]
        for batch in range(4):
            ev = [[] for _ in range(G)]
            wrote = {}
            touched = np.flatnonzero(rng.random(Z) < 0.6)
            clock = iter(rng.permutation(4 * len(touched) + 4).tolist())
            for p in touched:
                if rng.random() < 0.5:
                    w = int(rng.integers(0, G))
                    wrote[int(p)] = w
                    ev[w].append((int(p) << 36) | (next(clock) << 4) | (w << 1) | 1)
                for d in range(G):
                    if rng.random() < 0.35:
                        ev[d].append((int(p) << 36) | (next(clock) << 4) | (d << 1))
            stamped = [np.sort(np.array(e, np.uint64)) for e in ev]
            rc_ref, _, want_nt = oracle.route_round(gst, gfl, stamped, G, Z)
            assert rc_ref == 0
            # who writes what in this batch (the node has write access after the batch), and the
            # new contents
            writes = [[] for _ in range(G)]
            for p, w in sorted(wrote.items()):
                if access_of(gst[p:p + 1], w)[0] == 2:
                    new = model[p].copy()
                    idx = rng.choice(4096, int(rng.integers(1, 200)), replace=False)
                    new[idx] ^= rng.integers(1, 256, len(idx)).astype(np.uint8)
                    model[p] = new
                    writes[w].append(p)
            n_cap = sum(len(s) for s in stamped) + 1

            def rank(r):
                pt, pc, ctx, dc = pts[r], pt_comms[r], data.ctxs[r], data.comms[r]
                evb = pt.buffer(max(8, 8 * len(stamped[r]))).upload(stamped[r])
                bt, nt, tot = pt.buffer(8 * n_cap), pt.buffer(8 * (Z + 1)), pt.buffer(80)
                lst = pt.buffer(4 * Z)
                nb = exchange.route_events(pt, pc, evb.ptr, len(stamped[r]), Z, bt.ptr, n_cap)
                base = fm.block_of(r, Z, G)[0]
                k = exchange.coherence_notify(pt, pc, bt.ptr, nb, base, tot.ptr, nt.ptr, Z + 1)
                assert k == len(want_nt[r])
                m = exchange.notices_fetch_list(pt, nt.ptr, k, 2, lst.ptr, Z)
                exchange.fetch(ctx, dc, lst.ptr, None, m, Z)
                ctx.sync()
                for p in writes[r]:
                    ctx.upload("current", model[p:p + 1], first=p)
                send, sids, keep = [], [], []
                for d in range(G):
                    mine = np.array([p for p in writes[r] if p // per == d], np.uint32)
                    if len(mine):
                        ids = ctx.ids(mine)
                        keep.append(ids)
                        send.append(ctx.diff(ids, n=len(mine), cap=len(mine) * 10244))
                        ctx.twin(ids, n=len(mine))
                        sids.append(ctx.ids(mine - np.uint32(d * per)))
                    else:
                        send.append(ga.Runs.from_host(ctx, ga.gdsm.HostRuns(
                            np.zeros(1, np.uint64), np.zeros(0, np.uint8))))
                        sids.append(ctx.ids(np.zeros(1, np.uint32)))
                exchange.exchange_runs(ctx, dc, send, [b.ptr for b in sids], recv[r],
                                       [b.ptr for b in rids[r]])
                m = exchange.notices_fetch_list(pt, nt.ptr, k, 1, lst.ptr, Z)
                exchange.fetch(ctx, dc, lst.ptr, None, m, Z)  # no sync since the exchange
                ctx.sync()
                pt.sync()
                for b in [evb, bt, nt, tot, lst, *sids, *keep]:
                    b.free()
                for s in send:
                    s.free()
            run_ranks(G, rank)
            now = data.download()
            for h in range(G):
                base, nh = fm.block_of(h, Z, G)
                assert np.array_equal(now[h]["replica"][:nh], model[base:base + nh]), (batch, h)
            holders = 0
            for d in range(G):
                acc = access_of(gst, d)
                for p in np.flatnonzero(acc >= 1):
                    assert np.array_equal(now[d]["current"][p], model[p]), (batch, d, int(p))
                    holders += 1
            assert holders >= Z  # every page has a holder after a batch
    finally:
        for c in pt_comms:
            c.close()
        for c in pts:
            c.close()
        data.close()
