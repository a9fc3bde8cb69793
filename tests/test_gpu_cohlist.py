"""gdsm_coh_clean and gdsm_coh_lookup on the GPU (docs/SPEC.md §15) against the numpy model
tests/cohlist_model.py, exactly (table words, faults, counts, statuses, fields): list lengths around
the wave and the 1024-entry workgroup, every list shape and every offset of the list from a 16-byte
boundary, a list of more tiles than a clean has workgroups, every node on a table a GPU coherence batch made, hand-made words, repeats, ids out of
range, the empty list, NULL outputs, every immediate refusal, both calls recorded, the dirty bit
before and after a clean, the release chain on two loopback ranks and the forward chain lookup ->
split -> apply. Every output goes into a canary-padded buffer."""
import errno
import threading

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import exchange
from gallocy_amd.gdsm import lib
from oracle import oracle
from tests import cohlist_model as cm
from tests import split_model
from tests import sweep_model as sm

pytestmark = pytest.mark.gpu

T = 1024           # list entries per workgroup (gdsm_cohlist.hip kTile)
CLEAN_BLOCKS = 2048  # workgroups of a clean at most (gdsm_cohlist.hip kCleanBlocks)
Z = 3 * 2048 + 77  # pages of the shared table
PAD = 8            # canary elements around every output
CANARY32 = 0xDEADBEEF
CANARY8 = 0xC3
FILL64 = 0xA5A5A5A5A5A5A5A5
DIRTY = 1 << 18
EINVAL = -errno.EINVAL
LENGTHS = [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
SELECTIONS = [(0, 0xFF & ~(1 << 5) & ~(1 << 2)), (8, 0xFF), (0, 0xFFFFFFFF)]


def word(copyset, owner, state, dirty=0):
    return copyset | (owner << 8) | (state << 16) | (dirty << 18)


def table_ctx(n_pages, n_nodes=8):
    ctx = ga.Context(n_pages, arenas=())
    ctx.coh_init(n_nodes)
    return ctx


@pytest.fixture(scope="module")
def gpu_made():
    """A context whose table a GPU coherence batch produced (8 nodes; it is what the oracle makes of
    the same events), as downloaded, with bits 19-31 set by hand in every seventh word and random
    faults."""
    with table_ctx(Z) as ctx:
        counts = np.random.default_rng(142).integers(0, 9, Z).astype(np.uint64)
        ev = ctx.gen_events(counts, seed=143, n_nodes=8, write_pct=30)
        ctx.coherence_batch(ev)
        ev.free()
        st, fl = ctx.coh_download()
        ost, ofl = oracle.coh_init(Z, 8)
        rc, _ = oracle.coherence(ost, ofl, oracle.gen_events(counts, seed=143, n_nodes=8,
                                                             write_pct=30), n_nodes=8)
        assert rc == 0 and np.array_equal(st, ost) and np.array_equal(fl, ofl)
        plain = st.copy()
        high = np.arange(len(st[::7]), dtype=np.uint64) * 2654435761 % (1 << 13)
        st[::7] |= (high << 19).astype(np.uint32)
        fl = np.random.default_rng(144).integers(0, 1 << 32, Z, dtype=np.uint64).astype(np.uint32)
        yield ctx, st, fl, plain


# ------------------------------------------------------------------------------ device plumbing
class Buf:
    """n elements of `dtype` on the device, `off` elements behind an aligned allocation, with
    canaries in front and behind."""

    def __init__(self, ctx, n, dtype, fill, off=0, data=None):
        self.n, self.off, self.dtype, self.fill = n, off, np.dtype(dtype), fill
        host = np.full(off + n + PAD, fill, dtype)
        if data is not None:
            host[off:off + n] = np.asarray(data)[:n]
        self.buf = ctx.buffer(max(16, host.nbytes)).upload(host)
        self.ptr = self.buf.ptr + off * self.dtype.itemsize

    def read(self):
        got = self.buf.download(self.dtype, self.off + self.n + PAD)
        assert (got[:self.off] == self.fill).all() and (got[self.off + self.n:] == self.fill).all()
        return got[self.off:self.off + self.n]

    def free(self):
        self.buf.free()


def run_clean(ctx, node, ids, n=None, base=0, off=0, ooff=0, want_status=True, want_stats=True):
    """One gdsm_coh_clean with the list `off` elements behind a 16-byte boundary and the status
    bytes `ooff` behind one -> (stats dict or None, status or None, what gdsm_sync returned)."""
    n = len(ids) if n is None else n
    d_ids = Buf(ctx, n, np.uint32, 0xFFFFFFFF, off, ids) if ids is not None else None
    d_st = Buf(ctx, n, np.uint8, CANARY8, ooff) if want_status else None
    d_tot = Buf(ctx, 4, np.uint64, FILL64) if want_stats else None
    try:
        rc = lib().gdsm_coh_clean(ctx.handle, node, d_ids.ptr if d_ids else None, n, base,
                                  d_st.ptr if d_st else None, d_tot.ptr if d_tot else None, 0)
        assert rc == 0, rc
        src = lib().gdsm_sync(ctx.handle)
        stats = dict(zip(cm.KEYS, (int(x) for x in d_tot.read()))) if d_tot else None
        return stats, d_st.read() if d_st else None, src
    finally:
        for b in (d_ids, d_st, d_tot):
            if b:
                b.free()


def run_lookup(ctx, ids, n=None, base=0, shift=0, mask=0xFFFFFFFF, off=0, ooff=0, faults=True):
    """-> (out, faults_out or None, what gdsm_sync returned)."""
    n = len(ids) if n is None else n
    d_ids = Buf(ctx, n, np.uint32, 0xFFFFFFFF, off, ids) if ids is not None else None
    d_out = Buf(ctx, n, np.uint32, CANARY32, ooff)
    d_fl = Buf(ctx, n, np.uint32, CANARY32, (ooff + 1) % 4) if faults else None
    try:
        rc = lib().gdsm_coh_lookup(ctx.handle, d_ids.ptr if d_ids else None, n, base, shift, mask,
                                   d_out.ptr, d_fl.ptr if d_fl else None)
        assert rc == 0, rc
        src = lib().gdsm_sync(ctx.handle)
        return d_out.read(), d_fl.read() if d_fl else None, src
    finally:
        for b in (d_ids, d_out, d_fl):
            if b:
                b.free()


def check_clean(ctx, st, fl, node, ids, n=None, base=0, off=0, ooff=0, tag=""):
    """Uploads (st, fl); one clean against the model: table, faults, stats, status, the error the
    next sync reports (once). -> the model's (table, stats, status)."""
    want_st, want_stats, want_status, bad = cm.clean(st, node, ids, n, base)
    ctx.coh_upload(st, fl)
    stats, status, src = run_clean(ctx, node, ids, n, base, off, ooff)
    assert src == (EINVAL if bad else 0) and lib().gdsm_sync(ctx.handle) == 0, tag
    assert stats == want_stats and sum(stats.values()) == len(want_status), (tag, stats)
    assert np.array_equal(status, want_status), (tag, np.flatnonzero(status != want_status)[:8])
    gst, gfl = ctx.coh_download()
    assert np.array_equal(gst, want_st), (tag, np.flatnonzero(gst != want_st)[:8])
    assert np.array_equal(gfl, fl), tag
    return want_st, want_stats, want_status


def check_lookup(ctx, st, fl, ids, n=None, base=0, off=0, ooff=0, tag=""):
    """The three field selections, with and without faults_out, on the uploaded table."""
    for k, (shift, mask) in enumerate(SELECTIONS):
        want_out, want_fl, bad = cm.lookup(st, fl, ids, n, base, shift, mask)
        for faults in (True, False):
            out, fo, src = run_lookup(ctx, ids, n, base, shift, mask, off, (ooff + k) % 4, faults)
            assert src == (EINVAL if bad else 0), tag
            assert np.array_equal(out, want_out), (tag, shift, mask)
            assert fo is None or np.array_equal(fo, want_fl), (tag, "faults")


def shapes(rng, n, base):
    """(name, list or None, offset of the list from a 16-byte boundary in elements)."""
    start = int(rng.integers(0, Z - n + 1))
    dense = base + start + np.arange(n)
    yield "dense", dense.astype(np.uint32), 0
    yield "sparse", (base + np.sort(rng.choice(Z, n, replace=False))).astype(np.uint32), 0
    perm = (base + rng.permutation(Z)[:n]).astype(np.uint32)
    yield "permutation", perm, 0
    yield "null", None, 0
    for off in (1, 2, 3):
        yield f"offset {off}", perm, off


# ------------------------------------------------------------------------------ lengths, shapes
@pytest.mark.parametrize("n", LENGTHS)
def test_list_lengths_and_shapes(gpu_made, n):
    ctx, st, fl, _ = gpu_made
    rng = np.random.default_rng(200 + n)
    base = 5000
    for k, (name, ids, off) in enumerate(shapes(rng, n, base)):
        node = (n + k) % 8
        check_clean(ctx, st, fl, node, ids, n, base, off, ooff=k % 4, tag=(n, name))
        ctx.coh_upload(st, fl)
        check_lookup(ctx, st, fl, ids, n, base, off, ooff=k % 4, tag=(n, name))
        gst, gfl = ctx.coh_download()
        assert np.array_equal(gst, st) and np.array_equal(gfl, fl)   # lookup only reads


@pytest.mark.parametrize("node", range(8))
def test_every_node(gpu_made, node):
    """The whole table as a list, in a random order, offset by `node` elements; the dirty pages the
    node owns are cleaned and no others, and bits 19-31 survive."""
    ctx, st, fl, _ = gpu_made
    base = 1 << 20
    ids = (base + np.random.default_rng(210 + node).permutation(Z)).astype(np.uint32)
    want_st, stats, status = check_clean(ctx, st, fl, node, ids, base=base, off=node % 4,
                                         ooff=node % 3, tag=node)
    own_dirty = (((st >> 8) & 0xFF) == node) & ((st >> 16) & 3 != 0) & ((st >> 18) & 1 == 1)
    assert stats["cleaned"] == int(own_dirty.sum()) > 0 and stats["stale"] > stats["already"] > 0
    assert np.array_equal(want_st >> 19, st >> 19) and (st >> 19).any()
    # idempotent: the same call again cleans nothing
    stats2, status2, src = run_clean(ctx, node, ids, base=base)
    assert src == 0 and stats2 == {"cleaned": 0, "already": stats["cleaned"] + stats["already"],
                                   "stale": stats["stale"], "skipped": stats["skipped"]}
    assert np.array_equal(ctx.coh_download()[0], want_st)


def test_hand_made_words():
    n_pages = 70
    st = np.zeros(n_pages, np.uint32)                       # INVALID everywhere else
    fl = (np.arange(n_pages, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    x = 4
    st[1] = 0x1FF | DIRTY                                   # INVALID, stray low bits and bit 18
    st[2] = word(1 << x, x, sm.EXCLUSIVE, 1)                # owned, dirty
    st[3] = word(1 << x, x, sm.EXCLUSIVE, 0)                # owned, clean
    st[4] = word(1 << x | 1 << 6, x, sm.SHARED, 1) | (0x1ABC << 19)
    st[5] = word(1 << x | 1 << 6, x, sm.SHARED, 0)
    st[6] = word(1 << 6, 6, sm.EXCLUSIVE, 1)                # another owner, dirty
    st[7] = word(1 << 6, 6, sm.EXCLUSIVE, 0)
    st[8] = word(0xFF, 6, sm.SHARED, 1)                     # x holds a copy, owns nothing
    st[9] = word(0xFF, 6, sm.SHARED, 0)
    st[69] = word(1 << x, x, sm.SHARED, 1)                  # the last page of the table
    ids = np.arange(n_pages, dtype=np.uint32)
    with table_ctx(n_pages) as ctx:
        want_st, stats, status = check_clean(ctx, st, fl, x, ids)
        assert status[:10].tolist() == [3, 3, 0, 1, 0, 1, 2, 2, 2, 2] and status[69] == 0
        assert stats == {"cleaned": 3, "already": 2, "stale": 4, "skipped": 61}
        assert want_st[1] == st[1] and want_st[4] == st[4] & ~np.uint32(DIRTY)
        check_clean(ctx, st, fl, x, None, n_pages)          # the same through ids == NULL
        ctx.coh_upload(st, fl)
        check_lookup(ctx, st, fl, ids)
        out, _, _ = run_lookup(ctx, ids)
        assert out[1] == 0 and out[4] == st[4]              # INVALID reads as 0, high bits are read


def test_repeats():
    """A third of the entries repeat a page listed before; a page is cleaned once, the other
    entries of it report ALREADY, whichever of them the device picked."""
    n = 3 * T + 5
    rng = np.random.default_rng(220)
    st, fl = oracle.coh_init(Z, 8)
    ev = oracle.gen_events(rng.integers(0, 6, Z).astype(np.uint64), seed=221, write_pct=50)
    assert oracle.coherence(st, fl, ev)[0] == 0
    first = rng.choice(Z, n - n // 3, replace=False)
    ids = np.concatenate([first, rng.choice(first, n // 3)])
    ids = (77 + rng.permutation(ids)).astype(np.uint32)
    assert len(np.unique(ids)) < len(ids) == n
    with table_ctx(Z) as ctx:
        for node in (0, 5):
            want_st, want_stats, want_status, bad = cm.clean(st, node, ids, base=77)
            assert not bad and want_stats["cleaned"] > 50
            ctx.coh_upload(st, fl)
            stats, status, src = run_clean(ctx, node, ids, base=77, off=1)
            assert src == 0 and stats == want_stats
            assert cm.status_multisets(ids, status) == cm.status_multisets(ids, want_status)
            gst, gfl = ctx.coh_download()
            assert np.array_equal(gst, want_st) and np.array_equal(gfl, fl)
    # one page, a whole workgroup's worth of entries: cleaned exactly once
    ids = np.full(T + 3, 9, np.uint32)
    st2 = st.copy()
    st2[9] = word(2, 1, sm.EXCLUSIVE, 1)
    with table_ctx(Z) as ctx:
        ctx.coh_upload(st2, fl)
        stats, status, src = run_clean(ctx, 1, ids)
        assert src == 0 and stats == {"cleaned": 1, "already": T + 2, "stale": 0, "skipped": 0}
        assert sorted(status.tolist()) == [0] + [1] * (T + 2)
        assert ctx.coh_download()[0][9] == word(2, 1, sm.EXCLUSIVE, 0)


def test_more_tiles_than_workgroups(gpu_made):
    """A clean launches at most CLEAN_BLOCKS workgroups, which stride over the tiles: here every
    workgroup takes 2 tiles and the first four a third (the last of them partial), so the counts carried from
    tile to tile and the status stores of a workgroup's later tiles are compared. The list repeats
    every page of the table some 700 times, lies 3 elements behind a 16-byte boundary and has ids
    out of range in its first and in its last tile; the expectations are the model's whole-array
    form (held to the per-entry loop by tests/test_cohlist.py)."""
    ctx, st, fl, _ = gpu_made
    n = 2 * CLEAN_BLOCKS * T + 3 * T + 5
    base, node = 12345, 4
    rng = np.random.default_rng(225)
    ids = (base + rng.integers(0, Z, n)).astype(np.uint32)
    at = np.array([3, 700, n - CLEAN_BLOCKS * T - 9, n - 3, n - 1])
    ids[at] = [base - 1, base + Z, 0xFFFFFFFF, 0, base + Z + 7]
    want_st, want_stats, want_status, bad = cm.clean_vec(st, node, ids, base=base)
    assert bad and want_stats["cleaned"] > 50 and want_stats["already"] > n // 20
    ctx.coh_upload(st, fl)
    stats, status, src = run_clean(ctx, node, ids, base=base, off=3, ooff=1)
    assert src == EINVAL and lib().gdsm_sync(ctx.handle) == 0
    assert stats == want_stats and sum(stats.values()) == n
    # what does not depend on which entry of a page cleaned it is equal entry by entry
    fixed = want_status >= cm.STALE
    assert np.array_equal(status[fixed], want_status[fixed]) and (status[at] == 4).all()
    assert (status[~fixed] <= cm.ALREADY).all()
    # per page, the multiset of statuses (out-of-range ids share one row)
    page = np.where(want_status == cm.OUT_OF_RANGE, Z, ids.astype(np.int64) - base)
    got_h = np.bincount(page * 5 + status, minlength=5 * (Z + 1))
    want_h = np.bincount(page * 5 + want_status, minlength=5 * (Z + 1))
    assert np.array_equal(got_h, want_h)
    assert got_h.reshape(Z + 1, 5)[:Z, cm.CLEANED].max() == 1
    gst, gfl = ctx.coh_download()
    assert np.array_equal(gst, want_st) and np.array_equal(gfl, fl)
    # again on the cleaned table: nothing is cleaned, every entry as the model has it
    want2 = cm.clean_vec(want_st, node, ids, base=base)
    stats, status, src = run_clean(ctx, node, ids, base=base, off=1, ooff=0)
    assert src == EINVAL and stats == want2[1] and stats["cleaned"] == 0
    assert np.array_equal(status, want2[2])
    assert np.array_equal(ctx.coh_download()[0], want_st)


def test_ids_out_of_range(gpu_made):
    ctx, st, fl, _ = gpu_made
    base = 4096
    rng = np.random.default_rng(230)
    for n, off in ((T + 70, 0), (9, 3)):
        ids = (base + rng.permutation(Z)[:n]).astype(np.uint32)
        at = rng.choice(n, 6, replace=False)
        ids[at] = [base - 1, 0, base + Z, base + Z + 1, 0xFFFFFFFF, 0x80000000]
        _, stats, status = check_clean(ctx, st, fl, 3, ids, base=base, off=off, tag=n)
        assert (status[at] == 4).all() and (status == 4).sum() == 6 and stats["skipped"] >= 6
        assert stats["cleaned"] > 0 or n < 100                # the rest of the list is processed
        ctx.coh_upload(st, fl)
        check_lookup(ctx, st, fl, ids, base=base, off=off, tag=n)
        out, fo, src = run_lookup(ctx, ids, base=base)
        assert src == EINVAL and not out[at].any() and not fo[at].any()
        assert lib().gdsm_sync(ctx.handle) == 0               # reported once


def test_empty_list_and_null_outputs(gpu_made):
    ctx, st, fl, _ = gpu_made
    ctx.coh_upload(st, fl)
    ids = np.arange(100, dtype=np.uint32)
    # n == 0: four zeros and nothing else, with and without a list
    for lst in (ids, None):
        stats, status, src = run_clean(ctx, 0, lst, 0)
        assert src == 0 and stats == dict.fromkeys(cm.KEYS, 0) and len(status) == 0
        out, fo, src = run_lookup(ctx, lst, 0)
        assert src == 0 and len(out) == 0
    assert lib().gdsm_coh_clean(ctx.handle, 0, None, 0, 0, None, None, 0) == 0
    assert lib().gdsm_coh_lookup(ctx.handle, None, 0, 0, 0, 0, None, None) == 0
    assert np.array_equal(ctx.coh_download()[0], st)
    # NULL stats, NULL status_out, both NULL: the table is cleaned all the same
    want_st, want_stats, want_status, _ = cm.clean(st, 2, ids)
    assert want_stats["cleaned"] > 0
    for want_status_out, want_tot in ((True, False), (False, True), (False, False)):
        ctx.coh_upload(st, fl)
        stats, status, src = run_clean(ctx, 2, ids, want_status=want_status_out,
                                       want_stats=want_tot)
        assert src == 0
        assert stats is None or stats == want_stats
        assert status is None or np.array_equal(status, want_status)
        assert np.array_equal(ctx.coh_download()[0], want_st)


def test_immediate_refusals():
    n_pages = 100
    lb = lib()
    big = 1 << 28   # GDSM_MAX_COH_PAGES
    with ga.Context(n_pages, arenas=()) as ctx:
        h = ctx.handle
        d_ids = Buf(ctx, n_pages, np.uint32, 0, data=np.arange(n_pages))
        d_st = Buf(ctx, n_pages, np.uint8, CANARY8)
        d_tot = Buf(ctx, 4, np.uint64, FILL64)
        d_out = Buf(ctx, n_pages, np.uint32, CANARY32)
        d_fl = Buf(ctx, n_pages, np.uint32, CANARY32)
        i, s, t, o, f = d_ids.ptr, d_st.ptr, d_tot.ptr, d_out.ptr, d_fl.ptr
        # no page table yet
        assert lb.gdsm_coh_clean(h, 0, i, n_pages, 0, s, t, 0) == EINVAL
        assert lb.gdsm_coh_lookup(h, i, n_pages, 0, 0, 0xFF, o, f) == EINVAL
        ctx.coh_init(4)
        st0, fl0 = ctx.coh_download()
        bad_clean = [
            (None, 0, i, n_pages, 0, s, t, 0),                   # no context
            (h, 4, i, n_pages, 0, s, t, 0),                      # node >= n_nodes
            (h, 0xFFFFFFFF, i, n_pages, 0, s, t, 0),
            (h, 0, i, n_pages, 0, s, t, 1),                      # unknown flags
            (h, 0, i, n_pages, 0, s, t, 1 << 31),
            (h, 0, i, (1 << 32) + 1, 0, s, t, 0),                # n > 2^32
            (h, 0, i, (1 << 64) - 1, 0, s, t, 0),
            (h, 0, i, n_pages, big + 1, s, t, 0),                # base > GDSM_MAX_COH_PAGES
            (h, 0, i, n_pages, (1 << 64) - 1, s, t, 0),
            (h, 0, None, n_pages + 1, 0, s, t, 0),               # no list, n > gdsm_n_pages
        ]
        for args in bad_clean:
            assert lb.gdsm_coh_clean(*args) == EINVAL, args
        bad_lookup = [
            (None, i, n_pages, 0, 0, 0xFF, o, f),
            (h, i, n_pages, 0, 32, 0xFF, o, f),                  # shift > 31
            (h, i, n_pages, 0, 0xFFFFFFFF, 0xFF, o, f),
            (h, i, (1 << 32) + 1, 0, 0, 0xFF, o, f),
            (h, i, n_pages, big + 1, 0, 0xFF, o, f),
            (h, None, n_pages + 1, 0, 0, 0xFF, o, f),
            (h, i, n_pages, 0, 0, 0xFF, None, f),                # n > 0 with no out
            (h, i, 1, 0, 0, 0xFF, None, None),
        ]
        for args in bad_lookup:
            assert lb.gdsm_coh_lookup(*args) == EINVAL, args
        ctx.sync()   # none of the refusals left anything behind
        assert (d_st.read() == CANARY8).all() and (d_tot.read() == FILL64).all()
        assert (d_out.read() == CANARY32).all() and (d_fl.read() == CANARY32).all()
        st, fl = ctx.coh_download()
        assert np.array_equal(st, st0) and np.array_equal(fl, fl0)
        # the edges that are allowed: shift 31, base at its limit (every id below it is out of
        # range), the whole table without a list
        assert lb.gdsm_coh_lookup(h, i, n_pages, 0, 31, 1, o, None) == 0
        assert lb.gdsm_coh_lookup(h, None, n_pages, 0, 8, 0xFF, o, f) == 0
        ctx.sync()
        assert np.array_equal(d_out.read(), (st0 >> 8) & 0xFF) and not d_fl.read().any()
        assert lb.gdsm_coh_clean(h, 3, i, n_pages, big, s, t, 0) == 0
        assert lb.gdsm_sync(h) == EINVAL
        assert (d_st.read() == 4).all() and d_tot.read().tolist() == [0, 0, 0, n_pages]
        assert lb.gdsm_coh_clean(h, 3, None, n_pages, big, s, t, 0) == 0
        ctx.sync()
        assert d_tot.read().tolist() == [0, 25, 75, 0]          # coh_init: nothing is dirty
        assert np.array_equal(ctx.coh_download()[0], st0)


# ------------------------------------------------------------------------------ recorded
def test_recorded_calls_read_the_table_and_the_list_again(gpu_made):
    ctx, st, fl, _ = gpu_made
    n, base = T + 9, 300
    rng = np.random.default_rng(240)
    ids = (base + rng.permutation(Z)[:n]).astype(np.uint32)
    ctx.coh_upload(st, fl)
    d_ids = Buf(ctx, n, np.uint32, 0xFFFFFFFF, 1, ids)
    d_st, d_tot = Buf(ctx, n, np.uint8, CANARY8, 1), Buf(ctx, 4, np.uint64, FILL64)
    d_out, d_fl = Buf(ctx, n, np.uint32, CANARY32, 2), Buf(ctx, n, np.uint32, CANARY32)
    lb, h = lib(), ctx.handle
    ctx.capture_begin()
    try:
        assert lb.gdsm_coh_lookup(h, d_ids.ptr, n, base, 0, 0xFFFFFFFF, d_out.ptr, d_fl.ptr) == 0
        assert lb.gdsm_coh_clean(h, 6, d_ids.ptr, n, base, d_st.ptr, d_tot.ptr, 0) == 0
    finally:
        g = ctx.capture_end()
    try:
        assert np.array_equal(ctx.coh_download()[0], st)                 # recorded, not run
        assert (d_st.read() == CANARY8).all() and (d_out.read() == CANARY32).all()
        # another table and another list in the same buffers
        st2, fl2 = oracle.coh_init(Z, 8)
        ev = oracle.gen_events(rng.integers(0, 7, Z).astype(np.uint64), seed=241, write_pct=40)
        assert oracle.coherence(st2, fl2, ev)[0] == 0
        ids2 = (base + rng.permutation(Z)[:n]).astype(np.uint32)
        for table, faults, lst in ((st2, fl2, ids2), (st, fl, ids)):
            ctx.coh_upload(table, faults)
            host = np.full(1 + n + PAD, 0xFFFFFFFF, np.uint32)
            host[1:1 + n] = lst
            d_ids.buf.upload(host)
            g.launch(ctx)
            ctx.sync()
            want_out, want_fl, _ = cm.lookup(table, faults, lst, base=base)
            want_st, want_stats, want_status, _ = cm.clean(table, 6, lst, base=base)
            assert want_stats["cleaned"] > 0
            assert np.array_equal(d_out.read(), want_out) and np.array_equal(d_fl.read(), want_fl)
            assert d_tot.read().tolist() == [want_stats[k] for k in cm.KEYS]
            assert np.array_equal(d_st.read(), want_status)
            gst, gfl = ctx.coh_download()
            assert np.array_equal(gst, want_st) and np.array_equal(gfl, faults)
    finally:
        g.destroy()
        for b in (d_ids, d_st, d_tot, d_out, d_fl):
            b.free()


# ------------------------------------------------------------------------------ the dirty bit
def test_the_dirty_bit_now_means_something(gpu_made):
    ctx, _, _, st = gpu_made          # the table as the batch left it
    fl = np.zeros(Z, np.uint32)
    d, heir, base = 3, 4, 1 << 16
    mask, value = 0xFF00 | DIRTY, d << 8 | DIRTY
    ctx.coh_upload(st, fl)
    # 1. the node's release list, and what a crash of it would lose
    pages, count = ctx.coh_select(mask, value, base=base)
    before = ctx.coh_retire(d, heir, dry=True, cap=0)
    assert count == len(pages) > 0 and before["orphaned"] > 0
    # 2. the release reached the home
    d_pages = ctx.ids(pages)
    r = ctx.coh_clean(d, d_pages, n=count, base=base, status=True)
    assert r["cleaned"] == count and r["already"] == r["stale"] == r["skipped"] == 0
    assert not r["status"].any()
    want_st = cm.clean(st, d, pages, base=base)[0]
    assert np.array_equal(ctx.coh_download()[0], want_st)
    # 3. nothing is left to release, nothing would be lost
    assert ctx.coh_select(mask, value, base=base)[1] == 0
    after = ctx.coh_retire(d, heir, dry=True, cap=0)
    assert after["orphaned"] == 0 and after["moved"] == before["moved"]
    assert after["held"] == before["held"]
    # 4. d writes some of those pages again (others read or write other pages)
    rng = np.random.default_rng(250)
    again = np.sort(rng.choice(pages - base, max(1, count // 3), replace=False))
    counts = rng.integers(0, 3, Z).astype(np.uint64)
    ev = oracle.gen_events(counts, seed=251, n_nodes=8, write_pct=0).tolist()   # reads only
    ev += [(int(p) << 4) | (d << 1) | 1 for p in again]                         # d's writes last
    ev = np.array(sorted(ev, key=lambda e: e >> 4), np.uint64)                   # (stable)
    want_fl = fl.copy()
    rc, want_tot = oracle.coherence(want_st, want_fl, ev)
    assert rc == 0
    tot = ctx.coherence_batch(ev)
    gst, gfl = ctx.coh_download()
    assert tot == want_tot and np.array_equal(gst, want_st) and np.array_equal(gfl, want_fl)
    got, n_got = ctx.coh_select(mask, value, base=base)
    assert n_got == len(again) and np.array_equal(got, base + again)
    d_pages.free()


# ------------------------------------------------------------------------------ release chain
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
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    for e in errs:
        if e is not None:
            raise e


def test_release_then_exchange_then_clean_on_two_loopback_ranks():
    """scan -> diff -> split by home -> exchange -> clean. Every rank writes its own pages of both
    homes. In the homes' tables two thirds of a writer's pages are owned dirty by it (CLEANED) and
    a third were written by the other node since (STALE)."""
    G, total = 2, 130
    per = -(-total // G)
    rng = np.random.default_rng(260)
    base_pages = rng.integers(0, 256, (total, 4096), dtype=np.uint8)
    writer = rng.integers(0, 3, total)      # 0 and 1 write theirs, 2: nobody writes the page
    curs = []
    for r in range(G):
        cur = base_pages.copy()
        for p in np.flatnonzero(writer == r):
            cur[p, rng.integers(0, 4096, 20)] ^= rng.integers(1, 256, 20).astype(np.uint8)
        curs.append(cur)
    tables = []
    for h in range(G):
        lo, hi = h * per, min(total, (h + 1) * per)
        st = np.full(hi - lo, word(3, h, sm.SHARED, 0), np.uint32)
        for p in range(lo, hi):
            w = int(writer[p])
            if w < 2:
                o = w if p % 3 else 1 - w
                st[p - lo] = word(1 << o, o, sm.EXCLUSIVE, 1)
        tables.append(st)
    ctxs = [ga.Context(total) for _ in range(G)]
    pts = [table_ctx(min(total, (h + 1) * per) - h * per, G) for h in range(G)]
    for r, c in enumerate(ctxs):
        c.upload("twin", base_pages)
        c.upload("current", curs[r])
        c.upload("replica", base_pages[r * per:min(total, (r + 1) * per)])
        pts[r].coh_upload(tables[r], np.zeros(len(tables[r]), np.uint32))
    comms = exchange.Comm.loopback(ctxs)
    results = [None] * G
    try:
        def rank(r):
            c, pt = ctxs[r], pts[r]
            dl = c.dirty_scan()
            count, bound = dl.count, dl.bound
            runs = ga.Runs(c, count, cap=bound)
            c.diff(dl.pages, n=count, out=runs)
            res = exchange.split_by_home(c, runs, dl.pages, total, G)
            recv = [ga.Runs(c, per, cap=per * 1024) for _ in range(G)]
            rids = [c.buffer(4 * per) for _ in range(G)]
            exchange.exchange_runs(c, comms[r], res.runs, [b.ptr for b in res.ids], recv,
                                   [b.ptr for b in rids])
            c.sync()    # the table has a context of its own: the lists must be complete first
            got = []
            for s in range(G):
                lst, n = (res.ids[r], int(res.counts[r, 0])) if s == r else (rids[s], recv[s].n)
                out = pt.coh_clean(s, lst, n=n, base=0, status=True)
                out["ids"] = lst.download(np.uint32, n)
                got.append(out)
            results[r] = got
        run_ranks(G, rank)
        for h in range(G):
            lo, hi = h * per, min(total, (h + 1) * per)
            want_st = tables[h]
            for s in range(G):
                shipped = np.flatnonzero(writer[lo:hi] == s).astype(np.uint32)   # local ids
                got = results[h][s]
                assert np.array_equal(got["ids"], shipped) and len(shipped) > 5
                want_st, want_stats, want_status, bad = cm.clean(want_st, s, shipped)
                assert not bad and {k: got[k] for k in cm.KEYS} == want_stats
                assert np.array_equal(got["status"], want_status)
                mine = (lo + shipped) % 3 != 0
                assert (want_status[mine] == cm.CLEANED).all() and mine.any()
                assert (want_status[~mine] == cm.STALE).all() and (~mine).any()
            gst, gfl = pts[h].coh_download()
            assert np.array_equal(gst, want_st) and not gfl.any()
            assert not ((gst >> 18) & 1)[(lo + np.arange(hi - lo)) % 3 != 0].any()
            expect = base_pages[lo:hi].copy()
            for s in range(G):
                sel = np.flatnonzero(writer[lo:hi] == s)
                expect[sel] = curs[s][lo:hi][sel]
            assert np.array_equal(ctxs[h].download("replica", 0, hi - lo), expect)
    finally:
        for cm_ in comms:
            cm_.close()
        for c in ctxs + pts:
            c.close()


# ------------------------------------------------------------------------------ forward chain
@pytest.mark.parametrize("writer,home", [(0, 1), (2, 2)])
def test_lookup_then_split_then_apply(writer, home):
    """A home forwards a writer's stream to the nodes that hold copies: the masks come from the
    table on the device, the split's outputs equal the model on masks computed from the downloaded
    table, and out[d] applied to a second context changes exactly the pages d holds."""
    G, n_table, base = 3, 200, 64
    n_arena = base + n_table
    rng = np.random.default_rng(270 + writer)
    st, fl = oracle.coh_init(n_table, G)
    ev = oracle.gen_events(rng.integers(0, 8, n_table).astype(np.uint64), seed=271, n_nodes=G,
                           write_pct=15)
    assert oracle.coherence(st, fl, ev, n_nodes=G)[0] == 0
    twin = rng.integers(0, 256, (n_arena, 4096), dtype=np.uint8)
    cur = twin.copy()
    changed = np.sort(rng.choice(n_table, 120, replace=False)) + base
    for p in changed:
        k = int(rng.integers(1, 60))
        cur[p, rng.integers(0, 4096, k)] ^= rng.integers(1, 256, k).astype(np.uint8)
    ids = changed.astype(np.uint32)                       # ascending global ids
    sel = 0xFF & ~(1 << writer) & ~(1 << home)
    with ga.Context(n_arena) as a, ga.Context(n_arena) as b, table_ctx(n_table, G) as pt:
        pt.coh_upload(st, fl)
        a.upload("twin", twin)
        a.upload("current", cur)
        d_ids = a.ids(ids)
        runs = a.diff(d_ids, n=len(ids))
        a.sync()
        dest = pt.coh_lookup(d_ids.ptr, n=len(ids), base=base, shift=0, mask=sel)
        pt.sync()
        gst, _ = pt.coh_download()
        w = gst[ids - base]
        masks = np.where((w >> 16) & 3 != 0, w & np.uint32(sel), 0).astype(np.uint32)
        assert np.array_equal(dest.download(np.uint32, len(ids)), masks) and masks.any()
        host = runs.to_host()
        err, want, want_counts = split_model.split(host.rec_off, host.data, ids, masks, 0, G)
        assert err == 0
        res = a.runs_split(runs, ids=d_ids, dest=dest.ptr, G=G)
        assert np.array_equal(res.counts, want_counts)
        assert res.counts[writer, 0] == 0 and res.counts[home, 0] == 0
        assert int(res.counts[:, 0].sum()) > 0
        for d in range(G):
            k = int(want_counts[d, 0])
            assert res.runs[d].n == k
            if k:
                got = res.runs[d].to_host()
                assert np.array_equal(got.rec_off, want[d][0])
                assert np.array_equal(got.data[:int(want[d][0][-1])], want[d][1])
                assert np.array_equal(res.ids[d].download(np.uint32, k), want[d][2])
            b.upload("current", twin)
            b.apply(res.runs[d], "current", res.ids[d])
            b.sync()
            holds = ids[(masks >> d) & 1 == 1]
            expect = twin.copy()
            expect[holds] = cur[holds]
            assert np.array_equal(b.download("current"), expect), d
            assert d in (writer, home) or len(holds) > 0
        res.free()
        runs.free()
        dest.free()
        d_ids.free()


def test_python_wrappers(gpu_made):
    ctx, st, fl, _ = gpu_made
    ctx.coh_upload(st, fl)
    ids = (9 + np.random.default_rng(280).permutation(Z)[:500]).astype(np.uint32)
    d_ids = ctx.ids(ids)
    out, fo = ctx.coh_lookup(d_ids, base=9, shift=8, mask=0xFF, faults=True)
    words = ctx.coh_lookup(d_ids, base=9)
    whole = ctx.coh_lookup(n=100)
    ctx.sync()
    want = cm.lookup(st, fl, ids, base=9, shift=8, mask=0xFF)
    assert np.array_equal(out.download(np.uint32, 500), want[0])
    assert np.array_equal(fo.download(np.uint32, 500), want[1])
    assert np.array_equal(words.download(np.uint32, 500), cm.lookup(st, fl, ids, base=9)[0])
    assert np.array_equal(whole.download(np.uint32, 100), cm.lookup(st, fl, None, 100)[0])
    want_st, want_stats, want_status, _ = cm.clean(st, 1, ids, base=9)
    r = ctx.coh_clean(1, d_ids, base=9, status=True)
    assert {k: r[k] for k in cm.KEYS} == want_stats and np.array_equal(r["status"], want_status)
    assert "status" not in ctx.coh_clean(1, d_ids, base=9)
    assert np.array_equal(ctx.coh_download()[0], want_st)
    r = ctx.coh_clean(1)    # the whole table
    assert r == cm.clean(want_st, 1, None, Z)[1]
    for bfr in (out, fo, words, whole, d_ids):
        bfr.free()
