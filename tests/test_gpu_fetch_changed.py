"""gdsm_fetch_changed on ONE GPU (docs/SPEC.md §11): G ranks as threads with loopback communicators,
as tests/test_gpu_fetch.py. Exact comparisons against the numpy model tests/digest_model.py: every
arena of every rank (which is the gdsm_fetch result), the `changed` flags and the four `stats`
counts, with destinations prepared equal to the home copy, differing in one byte or unrelated; then
nothing stale, everything stale, the ordering after gdsm_exchange, the collective refusals, and one
protocol run in which former holders fault again and only the pages written since travel."""
import errno

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import exchange
from oracle import oracle
from tests import digest_model as dm
from tests import fetch_model as fm
from tests.test_gpu_fetch import ARENAS, Group, request_of, run_ranks

pytestmark = pytest.mark.gpu


def home_copy(grp, p):
    h = int(p) // fm.per_of(grp.Z, grp.G)
    return grp.host[h]["replica"][int(p) - h * fm.per_of(grp.Z, grp.G)]


def prepare(grp, rng, reqs, dsts, names, kinds=(0, 1, 2, 3)):
    """Sets every requested entry's destination on every rank (host mirror and device) to one of:
    0 equal to the home copy in A with the other arena different, 1 equal in both, 2 the home copy
    with one byte changed (byte 0, byte 4095 or a random one), 3 unrelated (left as it is)."""
    a = dm.first_arena(names)
    other = "twin" if a == "current" else "current"
    for r in range(grp.G):
        dst = reqs[r] if dsts[r] is None else dsts[r]
        for p, d in zip(reqs[r], dst):
            kind = kinds[int(rng.integers(0, len(kinds)))]
            home = home_copy(grp, p)
            if kind in (0, 1, 2):
                grp.host[r][a][d] = home
            if kind == 1:
                grp.host[r][other][d] = home
            if kind == 2:
                at = (0, 4095, int(rng.integers(0, 4096)))[int(rng.integers(0, 3))]
                grp.host[r][a][d, at] ^= np.uint8(rng.integers(1, 256))
        for name in (a, other):
            grp.ctxs[r].upload(name, grp.host[r][name])


def assert_digests_decide(grp, reqs, dsts, names):
    """The condition on the inputs: for every prepared (requester copy, home copy) pair the digests
    are equal exactly when the bytes are."""
    rep = [h["replica"] for h in grp.host]
    for mine, home, _ in dm.pairs(rep, reqs, dsts, [{a: h[a] for a in names} for h in grp.host],
                                  grp.Z):
        same_bytes = (mine == home).all(axis=1)
        assert np.array_equal(same_bytes, ~dm.digests_differ(mine, home))


def call_and_check(grp, reqs, dsts, names, outputs=True, tag=None):
    """One collective gdsm_fetch_changed; compares arenas, changed and stats with the model, updates
    the host mirror and returns the stats per rank (the model's changed flags: grp.want_changed)."""
    G, Z = grp.G, grp.Z
    rep = [h["replica"] for h in grp.host]
    want, want_ch, want_st = dm.fetch_changed(rep, reqs, dsts,
                                              [{a: h[a] for a in names} for h in grp.host], Z)
    grp.want_changed = want_ch
    got_ch, got_st = [None] * G, [None] * G

    def rank(r):
        ctx, n = grp.ctxs[r], len(reqs[r])
        pb = ctx.ids(reqs[r]) if n else None
        db = ctx.ids(dsts[r]) if dsts[r] is not None and n else None
        ch = ctx.buffer(4 * max(n, 1)).upload(np.full(max(n, 1), 7, np.uint32)) if outputs else None
        st = ctx.buffer(32).upload(np.full(4, 99, np.uint64)) if outputs else None
        exchange.fetch_changed(ctx, grp.comms[r], pb, db, n, Z, dst=names, changed=ch, stats=st)
        ctx.sync()
        if outputs:
            got_ch[r] = ch.download(np.uint32, max(n, 1))[:n]
            got_st[r] = st.download(np.uint64, 4).tolist()
        for b in (pb, db, ch, st):
            if b is not None:
                b.free()
    run_ranks(G, rank)
    now = grp.download()
    for r in range(G):
        for a in ARENAS:
            exp = want[r][a] if a in names else grp.host[r][a]
            assert np.array_equal(now[r][a], exp), (tag, r, a)
            grp.host[r][a] = exp
        if outputs:
            assert np.array_equal(got_ch[r], want_ch[r]), (tag, r)
            assert got_st[r] == want_st[r], (tag, r)
    return want_st


class BlockGroup(Group):
    """As Group for 2 ranks and Z global pages, with contexts of one home block (Z / 2 pages) each
    and every arena derived from one random block (a constant XORed in per rank and arena), which
    keeps a list of more than 65536 pages affordable."""

    def __init__(self, Z, seed):
        rng = np.random.default_rng(seed)
        per = fm.per_of(Z, 2)
        self.G, self.Z = 2, Z
        self.ctxs = [ga.Context(per) for _ in range(2)]
        block = rng.integers(0, 2 ** 64, (per, 512), dtype=np.uint64).view(np.uint8)
        self.host = []
        for r, c in enumerate(self.ctxs):
            h = {a: block ^ np.uint8(1 + 3 * r + i) for i, a in enumerate(ARENAS)}
            for a in ARENAS:
                c.upload(a, h[a])
            self.host.append(h)
        self.comms = exchange.Comm.loopback(self.ctxs)


def scan_carry_case(Z):
    """One call in which rank 0 requests every page homed at rank 1, more than 65536 of them, so
    that the positions of the changed pages (fetchc_pos: 256 flags a block, one workgroup scanning
    256 block counts a step) are scanned past the first step at the requester (its entries homed
    elsewhere) and at the home (the requests it received), with changed pages on both sides of
    entry 65536. Rank 1 requests a few pages of both homes. About one destination in fifteen
    differs from the home copy."""
    per = fm.per_of(Z, 2)
    rng = np.random.default_rng(Z)
    grp = BlockGroup(Z, seed=Z + 1)
    try:
        reqs = [np.arange(per, Z, dtype=np.uint32), np.array([0, 5, per, per + 1, Z - 1], np.uint32)]
        dsts = [rng.permutation(per)[:len(q)].astype(np.uint32) for q in reqs]
        names = ("current", "twin")
        for r in range(2):
            assert fm.valid_request(reqs[r], dsts[r], Z, per)
        prepare(grp, rng, reqs, dsts, names, kinds=(0, 2, 3) + (1,) * 27)
        assert_digests_decide(grp, reqs, dsts, names)
        call_and_check(grp, reqs, dsts, names)
        remote = reqs[0] // per != 0
        changed = grp.want_changed[0][remote]
        assert len(changed) > 65536 and changed[:65536].any() and changed[65536:].any()
    finally:
        grp.close()


@pytest.mark.parametrize("G,Z", [(1, 37), (2, 130), (3, 1025), (4, 777), (8, 1031), (8, 5),
                                 (2, 2 * 66000)])
def test_fetch_changed_equals_model(G, Z):
    """Five calls in a row on the same contexts with the rotating request roles of
    test_fetch_equals_model: dst_ids NULL / injective, both arenas / CURRENT only / TWIN only,
    changed and stats given / NULL. About a quarter of the destinations each: equal in A only,
    equal in both arenas, one byte off, unrelated. The last case is scan_carry_case."""
    if Z > 2 * 65536:
        assert G == 2
        return scan_carry_case(Z)
    rng = np.random.default_rng(100 * G + Z)
    grp = Group(G, Z, seed=G * 7919 + Z + 1)
    try:
        variants = [(False, ("current", "twin"), True), (False, ("current",), True),
                    (True, ("current", "twin"), False), (True, ("twin",), True),
                    (True, ("current", "twin"), True)]
        seen = np.zeros(4, np.int64)
        for v, (with_dst, names, outputs) in enumerate(variants):
            reqs = [request_of((r + v) % 8, rng, r, G, Z) for r in range(G)]
            dsts = [rng.permutation(Z)[:len(q)].astype(np.uint32) if with_dst else None
                    for q in reqs]
            for r in range(G):
                assert fm.valid_request(reqs[r], dsts[r], Z, Z)
            prepare(grp, rng, reqs, dsts, names)
            assert_digests_decide(grp, reqs, dsts, names)
            st = call_and_check(grp, reqs, dsts, names, outputs, tag=v)
            seen += np.sum(st, axis=0)
            if len(names) == 2:  # both arenas: the pages are clean, skipped ones included
                for r in range(G):
                    d = reqs[r] if dsts[r] is None else dsts[r]
                    assert np.array_equal(grp.host[r]["twin"][d], grp.host[r]["current"][d])
        if G > 1 and Z > G:
            assert (seen > 0).all(), seen  # transferred, skipped, local differing, local equal
    finally:
        grp.close()


def test_nothing_stale_moves_no_page():
    G, Z = 4, 203
    rng = np.random.default_rng(5)
    grp = Group(G, Z, seed=21)
    try:
        reqs = [request_of(role, rng, r, G, Z) for r, role in enumerate((0, 2, 7, 5))]
        dsts = [None] * G
        prepare(grp, rng, reqs, dsts, ("current", "twin"), kinds=(0, 1))
        assert_digests_decide(grp, reqs, dsts, ("current", "twin"))
        st = call_and_check(grp, reqs, dsts, ("current", "twin"))
        for r in range(G):
            assert st[r][0] == 0 and st[r][2] == 0 and st[r][1] + st[r][3] == len(reqs[r])
    finally:
        grp.close()


def test_everything_stale_equals_a_plain_fetch():
    G, Z = 3, 150
    rng = np.random.default_rng(6)
    grp = Group(G, Z, seed=22)
    try:
        reqs = [request_of(role, rng, r, G, Z) for r, role in enumerate((2, 0, 7))]
        dsts = [rng.permutation(Z)[:len(q)].astype(np.uint32) for q in reqs]
        before = [{a: h[a].copy() for a in ARENAS} for h in grp.host]
        assert_digests_decide(grp, reqs, dsts, ("current", "twin"))
        st = call_and_check(grp, reqs, dsts, ("current", "twin"))
        for r in range(G):
            assert st[r][1] == 0 and st[r][3] == 0 and st[r][0] + st[r][2] == len(reqs[r])
        changed = grp.download()
        # the same lists through gdsm_fetch from the same start
        for r, c in enumerate(grp.ctxs):
            for a in ARENAS:
                c.upload(a, before[r][a])

        def rank(r):
            ctx = grp.ctxs[r]
            pb, db = ctx.ids(reqs[r]), ctx.ids(dsts[r])
            exchange.fetch(ctx, grp.comms[r], pb, db, len(reqs[r]), Z)
            ctx.sync()
            pb.free()
            db.free()
        run_ranks(G, rank)
        plain = grp.download()
        for r in range(G):
            for a in ARENAS:
                assert np.array_equal(changed[r][a], plain[r][a]), (r, a)
    finally:
        grp.close()


def test_fetch_changed_is_ordered_after_exchange():
    """As test_fetch_is_ordered_after_exchange: rank 0's release patches home 1's REPLICA page 0;
    with no sync in between every rank fetches that page conditionally. Rank 1 (the home, local
    path) and rank 0 (remote) both held the pre-release bytes, so only a fetch ordered after the
    exchange sees a difference and brings the released bytes."""
    G, Z = 2, 16
    grp = Group(G, Z, seed=3)
    try:
        per = fm.per_of(Z, G)
        for d in range(G):
            for r in range(G):
                grp.ctxs[d].upload("replica", grp.host[r]["twin"][3:4], first=r)
                grp.host[d]["replica"][r] = grp.host[r]["twin"][3]
        target = 1 * per + 0
        old = grp.host[0]["twin"][3]
        got, stats = [None] * G, [None] * G

        def rank(r):
            ctx, comm = grp.ctxs[r], grp.comms[r]
            ctx.upload("current", old[None], first=7)   # the copy the node still holds
            src = ctx.ids(np.array([3], np.uint32))
            sid = ctx.ids(np.array([r], np.uint32))
            send = [ctx.diff(src, n=1, cap=16384) for _ in range(G)]
            recv = [ga.Runs(ctx, 4, cap=16384) for _ in range(G)]
            rids = [ctx.buffer(16) for _ in range(G)]
            pg = ctx.ids(np.array([target], np.uint32))
            dst = ctx.ids(np.array([7], np.uint32))
            st = ctx.buffer(32)
            exchange.exchange_runs(ctx, comm, send, [sid.ptr] * G, recv, [b.ptr for b in rids])
            exchange.fetch_changed(ctx, comm, pg, dst, 1, Z, stats=st)   # no sync since the diff
            ctx.sync()
            got[r] = ctx.download("current", 7, 1)[0]
            stats[r] = st.download(np.uint64, 4).tolist()
        run_ranks(G, rank)
        assert not np.array_equal(grp.host[0]["current"][3], old)
        for r in range(G):
            assert np.array_equal(got[r], grp.host[0]["current"][3]), r
        assert stats == [[1, 0, 0, 0], [0, 0, 1, 0]]
    finally:
        grp.close()


def raw_fetch_changed(grp, r, pages, dst, total, src=ga.REPLICA, mask=0, ctx=None):
    ctx = ctx or grp.ctxs[r]
    pb = ctx.ids(pages) if len(pages) else None
    db = ctx.ids(dst) if dst is not None and len(dst) else None
    rc = ga.gdsm.lib().gdsm_fetch_changed(ctx.handle, grp.comms[r].handle, pb.ptr if pb else None,
                                          db.ptr if db else None, len(pages), total, src, mask,
                                          None, None)
    ctx.sync()
    for b in (pb, db):
        if b is not None:
            b.free()
    return rc


def test_fetch_changed_refusals_are_collective():
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
                rcs[r] = raw_fetch_changed(grp, r, lists[r], dsts[r], total, ctx=ctxs[r])
            run_ranks(G, rank)
            return rcs

        assert lib.gdsm_debug_fail_alloc(grp.ctxs[1].handle, 1) == 0
        assert case(good) == [-errno.ECANCELED, -errno.ENOMEM, -errno.ECANCELED]
        assert lib.gdsm_debug_fail_alloc(grp.ctxs[1].handle, 0) == 0
        grp.assert_unchanged()
        inval = [-errno.EINVAL] * G
        assert case([good[0], np.array([5, 5], np.uint32), good[2]]) == inval       # duplicate
        assert case([np.array([40, 1], np.uint32), good[1], good[2]]) == inval      # unsorted
        assert case([good[0], good[1], np.array([3, Z], np.uint32)]) == inval       # page == total
        assert case(good, dsts=(None, np.array([2, Z], np.uint32), None)) == inval  # dst == n_pages
        before = small.download("current")
        assert case([good[0], np.zeros(0, np.uint32), good[2]], ctxs=(None, small, None)) == inval
        assert np.array_equal(small.download("current"), before)
        grp.assert_unchanged()
        c0, m0 = grp.ctxs[0], grp.comms[0]
        ids = c0.ids(good[0])
        for args in [(ids.ptr, None, 3, 0, 2, 0), (ids.ptr, None, 3, (1 << 28) + 1, 2, 0),
                     (None, None, 3, Z, 2, 0), (ids.ptr, None, 3, Z, 3, 0),
                     (ids.ptr, None, 3, Z, -1, 0), (ids.ptr, None, 3, Z, 2, 4),
                     (ids.ptr, None, 3, Z, 1, 0), (ids.ptr, None, 3, Z, 0, 1)]:
            assert lib.gdsm_fetch_changed(c0.handle, m0.handle, *args, None, None) == -errno.EINVAL
        pt = ga.Context(4, arenas=())
        assert lib.gdsm_fetch_changed(pt.handle, m0.handle, ids.ptr, None, 3, Z, 2, 0, None,
                                      None) == -errno.EINVAL
        pt.close()
        ids.free()
        # a valid call on the same communicators
        call_and_check(grp, good, [None] * G, ("current", "twin"))
    finally:
        small.close()
        grp.close()


def test_fetch_changed_refuses_a_recording_context():
    grp = Group(1, 8, seed=2)
    lib = ga.gdsm.lib()
    try:
        ctx, comm = grp.ctxs[0], grp.comms[0]
        ids = ctx.ids(np.array([1, 2], np.uint32))
        ctx.capture_begin()
        try:
            assert lib.gdsm_fetch_changed(ctx.handle, comm.handle, ids.ptr, None, 2, 8, 2, 0, None,
                                          None) == -errno.EBUSY
        finally:
            ctx.capture_end().destroy()
        grp.assert_unchanged()
        assert raw_fetch_changed(grp, 0, np.array([1, 2], np.uint32), None, 8) == 0
    finally:
        grp.close()


def test_protocol_round_refetch_moves_only_what_was_written():
    """G = 4 nodes, Z = 96 pages, three batches over the pages S (every third page). Batch 0: node
    a(p) = home + 1 faults on p for reading and fetches it. Batch 1: node b(p) = home + 2 faults for
    writing (a loses its access), fetches, changes the pages of W (half of S), and releases them to
    the homes through gdsm_exchange. Batch 2: the former holders a fault again for reading and fetch
    conditionally, with no sync since the exchange: of their entries exactly those in W are
    transferred, the others are found equal by digest, and every holder has the home's bytes.
    Notices come from the page-table contexts (checked against the oracle's counts); the stats of
    every call are compared with the host model."""
    G, Z = 4, 96
    rng = np.random.default_rng(77)
    per = fm.per_of(Z, G)
    data = Group(G, Z, seed=9)
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
        S = np.arange(0, Z, 3)
        W = set(int(p) for p in S[::2])
        a_of = {int(p): (int(p) // per + 1) % G for p in S}
        b_of = {int(p): (int(p) // per + 2) % G for p in S}
        recv = [[ga.Runs(data.ctxs[r], Z, cap=Z * 10244) for _ in range(G)] for r in range(G)]
        rids = [[data.ctxs[r].buffer(4 * Z) for _ in range(G)] for r in range(G)]
        seq = 0
        for batch, (who, rw) in enumerate([(a_of, 0), (b_of, 1), (a_of, 0)]):
            ev = [[] for _ in range(G)]
            for p in S:
                d = who[int(p)]
                ev[d].append((int(p) << 36) | (seq << 4) | (d << 1) | rw)
                seq += 1
            stamped = [np.sort(np.array(e, np.uint64)) for e in ev]
            rc_ref, _, want_nt = oracle.route_round(gst, gfl, stamped, G, Z)
            assert rc_ref == 0
            lists = [fm.fetch_list(want_nt[r], 3) for r in range(G)]
            for r in range(G):
                mine = sorted(p for p, d in who.items() if d == r)
                assert lists[r].tolist() == mine, (batch, r)
            names = ("current", "twin")
            rep = [h["replica"] for h in data.host]
            want, _, want_st = dm.fetch_changed(rep, lists, [None] * G,
                                                [{a: h[a] for a in names} for h in data.host], Z)
            writes = [[p for p in lists[r] if int(p) in W] if rw else [] for r in range(G)]
            new = {}
            for r in range(G):
                for p in writes[r]:
                    page = want[r]["current"][p].copy()
                    idx = rng.choice(4096, int(rng.integers(1, 200)), replace=False)
                    page[idx] ^= rng.integers(1, 256, len(idx)).astype(np.uint8)
                    new[int(p)] = page
            n_cap = sum(len(s) for s in stamped) + 1
            got_st = [None] * G

            def rank(r):
                pt, pc, ctx, dc = pts[r], pt_comms[r], data.ctxs[r], data.comms[r]
                evb = pt.buffer(max(8, 8 * len(stamped[r]))).upload(stamped[r])
                bt, nt, tot = pt.buffer(8 * n_cap), pt.buffer(8 * (Z + 1)), pt.buffer(80)
                lst, st = pt.buffer(4 * Z), ctx.buffer(32)
                nb = exchange.route_events(pt, pc, evb.ptr, len(stamped[r]), Z, bt.ptr, n_cap)
                k = exchange.coherence_notify(pt, pc, bt.ptr, nb, fm.block_of(r, Z, G)[0], tot.ptr,
                                              nt.ptr, Z + 1)
                assert k == len(want_nt[r])
                m = exchange.notices_fetch_list(pt, nt.ptr, k, 3, lst.ptr, Z)
                assert m == len(lists[r])
                if rw:   # writers: fetch, write, release; the fetch is synchronised by the upload
                    exchange.fetch_changed(ctx, dc, lst.ptr, None, m, Z, stats=st)
                    ctx.sync()
                    for p in writes[r]:
                        ctx.upload("current", new[int(p)][None], first=int(p))
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
                if not rw:  # readers: after the exchange, no sync in between
                    exchange.fetch_changed(ctx, dc, lst.ptr, None, m, Z, stats=st)
                ctx.sync()
                pt.sync()
                got_st[r] = st.download(np.uint64, 4).tolist()
                for b in [evb, bt, nt, tot, lst, st, *sids, *keep]:
                    b.free()
                for s in send:
                    s.free()
            run_ranks(G, rank)
            # the host model: the fetch, then the writes at the writers and at the homes
            for r in range(G):
                for a in names:
                    data.host[r][a] = want[r][a]
                for p in writes[r]:
                    for a in names:
                        data.host[r][a][p] = new[int(p)]
                    data.host[int(p) // per]["replica"][int(p) % per] = new[int(p)]
            now = data.download()
            for r in range(G):
                assert got_st[r] == want_st[r], (batch, r)
                for a in ARENAS:
                    assert np.array_equal(now[r][a], data.host[r][a]), (batch, r, a)
            if batch == 2:   # only what the writers changed travels
                for r in range(G):
                    mine = [int(p) for p in lists[r]]
                    assert all(p // per != r for p in mine)
                    assert got_st[r] == [sum(p in W for p in mine), sum(p not in W for p in mine),
                                         0, 0], r
                assert sum(s[0] for s in got_st) == len(W)
                assert sum(s[1] for s in got_st) == len(S) - len(W)
            else:            # first contact: every copy is stale
                for r in range(G):
                    assert got_st[r] == [len(lists[r]), 0, 0, 0], (batch, r)
    finally:
        for c in pt_comms:
            c.close()
        for c in pts:
            c.close()
        data.close()
