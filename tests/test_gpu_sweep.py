"""gdsm_coh_retire and gdsm_coh_select on the GPU (docs/SPEC.md §14) against the numpy model
tests/sweep_model.py, exactly (table words, faults, counts and lists): table sizes around the
64-page flag word and the 2048-page workgroup tile, a table of more than 256 tiles, sub-ranges with
odd ends, every node retired from a table a GPU coherence batch made, the heir forms, hand-made
words, dry against wet, capacities below the count, the fold after a retire, the select questions,
a restarted node rebuilt by select -> fetch, every immediate refusal and a recorded sweep. Outputs
go into canary-padded buffers."""
import errno
import threading

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import exchange
from gallocy_amd.gdsm import lib
from oracle import oracle
from tests import fetch_model as fm
from tests import sweep_model as sm
from tests.helpers import tuned

pytestmark = pytest.mark.gpu

T = 2048           # table pages per workgroup of the flag kernel
CANARY = 0xDEADBEEF
PAD = 8            # canary words behind every list
FILL64 = 0xA5A5A5A5A5A5A5A5
EXCL, DIRTY = sm.EXCLUSIVE << 16, 1 << 18
ZERO = {"held": 0, "moved": 0, "orphaned": 0}


def word(copyset, owner, state, dirty=0):
    return copyset | (owner << 8) | (state << 16) | (dirty << 18)


def host_table(n_pages, n_nodes=8, seed=0, write_pct=25, most=5):
    """A valid table made on the host (the initial one after a random batch of up to `most` events
    per page), with random faults."""
    rng = np.random.default_rng(seed)
    st, fl = oracle.coh_init(n_pages, n_nodes)
    counts = rng.integers(0, most + 1, n_pages).astype(np.uint64)
    ev = oracle.gen_events(counts, seed=seed + 1, n_nodes=n_nodes, write_pct=write_pct)
    rc, _ = oracle.coherence(st, fl, ev, n_nodes=n_nodes)
    assert rc == 0
    return st, rng.integers(0, 1 << 32, n_pages, dtype=np.uint64).astype(np.uint32)


def table_ctx(n_pages, n_nodes=8):
    ctx = ga.Context(n_pages, arenas=())
    ctx.coh_init(n_nodes)
    return ctx


def call(ctx, invoke, words, pick, cap, want_list=True):
    """One sweep, invoke(list, cap, totals) -> rc, into canary-filled buffers: (the `words` totals,
    the list cut to what the call may have written); asserts that nothing behind that was."""
    d_out = None
    if want_list:
        d_out = ctx.buffer(4 * (cap + PAD)).upload(np.full(cap + PAD, CANARY, np.uint32))
    d_tot = ctx.buffer(8 * (words + 1)).upload(np.full(words + 1, FILL64, np.uint64))
    try:
        rc = invoke(ctx._ptr(d_out), cap, d_tot.ptr)
        assert rc == 0, rc
        ctx.sync()
        tot = d_tot.download(np.uint64, words + 1)
        assert tot[words] == FILL64
        tot = [int(x) for x in tot[:words]]
        lst = np.zeros(0, np.uint32)
        if d_out is not None:
            got = d_out.download(np.uint32, cap + PAD)
            used = min(tot[pick], cap)
            assert (got[used:] == CANARY).all()
            lst = got[:used]
    finally:
        d_tot.free()
        if d_out is not None:
            d_out.free()
    return tot, lst


def retire(ctx, x, heir, base=0, per=0, first=0, n=None, cap=None, dry=False, want_list=True):
    """gdsm_coh_retire -> ({held, moved, orphaned}, moved_out)."""
    n = ctx.n_pages - first if n is None else n
    cap = 0 if not want_list else n if cap is None else cap
    tot, lst = call(ctx, lambda out, c, stats: lib().gdsm_coh_retire(
        ctx.handle, x, heir, base, per, first, n, out, c, stats, int(dry)), 3, 1, cap, want_list)
    return dict(zip(("held", "moved", "orphaned"), tot)), lst


def select(ctx, mask, value, base=0, first=0, n=None, cap=None, want_list=True):
    """gdsm_coh_select -> (pages, count)."""
    n = ctx.n_pages - first if n is None else n
    cap = 0 if not want_list else n if cap is None else cap
    tot, lst = call(ctx, lambda out, c, count: lib().gdsm_coh_select(
        ctx.handle, mask, value, base, first, n, out, c, count), 1, 0, cap, want_list)
    return lst, tot[0]


def check_retire(ctx, st, fl, x, heir, base=0, per=0, first=0, n=None, n_nodes=8, tag=""):
    """Uploads (st, fl); the dry call, the wet call and a second wet call against the model."""
    n = len(st) - first if n is None else n
    want_st, want_stats, want_out = sm.retire(st, x, heir, base, per, first, n, n_nodes)
    ctx.coh_upload(st, fl)
    args = (x, heir, base, per, first, n)
    stats, out = retire(ctx, *args, dry=True)
    assert stats == want_stats and np.array_equal(out, want_out), (tag, "dry")
    gst, gfl = ctx.coh_download()
    assert np.array_equal(gst, st) and np.array_equal(gfl, fl), (tag, "dry")
    stats, out = retire(ctx, *args)
    assert stats == want_stats and np.array_equal(out, want_out), (tag, "wet")
    gst, gfl = ctx.coh_download()
    assert np.array_equal(gst, want_st), (tag, np.flatnonzero(gst != want_st)[:8])
    assert np.array_equal(gfl, fl), tag
    stats, out = retire(ctx, *args)
    assert stats == ZERO and len(out) == 0, (tag, "again")
    gst, gfl = ctx.coh_download()
    assert np.array_equal(gst, want_st) and np.array_equal(gfl, fl), (tag, "again")
    return want_st, want_stats, want_out


def check_select(ctx, st, mask, value, base=0, first=0, n=None, tag=""):
    n = len(st) - first if n is None else n
    want = sm.select(st, mask, value, base, first, n)
    got = select(ctx, mask, value, base, first, n)
    assert got[1] == want[1] and np.array_equal(got[0], want[0]), tag
    return want


# ------------------------------------------------------------------------------ sizes and ranges
@pytest.mark.parametrize("Z", [1, 63, 64, 65, T - 1, T, T + 1])
def test_sizes_around_the_flag_word_and_the_tile(Z):
    st, fl = host_table(Z, seed=Z)
    st[Z // 2] = word(1 << 3, 3, sm.EXCLUSIVE, 1)  # (a table of one page must still move it)
    with table_ctx(Z) as ctx:
        _, stats, _ = check_retire(ctx, st, fl, 3, 5, base=7, tag=Z)
        assert stats["moved"] >= 1 and stats["orphaned"] >= 1
        ctx.coh_upload(st, fl)
        for d in (0, 3):
            check_select(ctx, st, 1 << d, 1 << d, base=7, tag=(Z, d))
        assert check_select(ctx, st, 0, 0)[1] == Z


@pytest.fixture(scope="module")
def long_table():
    """259 tiles: 17 of the 16-tile groups a thread of the sum kernel takes, the last one partial
    (still one step of its scan: see test_scan_of_more_than_one_step). The model's answers are
    computed once."""
    Z = 258 * T + 5
    st, fl = host_table(Z, seed=140)
    return Z, st, fl, sm.retire(st, 2, 6, 0, 0, 1, Z - 2), sm.select(st, 1 << 2, 1 << 2, 0, 1, Z - 2)


def test_more_than_256_tiles(long_table):
    """(The per-page loop of the model, on the longest table it is quick for.)"""
    Z, st, fl, (want_st, want_stats, want_out), (want_pages, want_count) = long_table
    assert want_count > want_stats["moved"] > 256 * 64
    with table_ctx(Z) as ctx:
        ctx.coh_upload(st, fl)
        pages, count = select(ctx, 1 << 2, 1 << 2, 0, 1, Z - 2)
        assert count == want_count and np.array_equal(pages, want_pages)
        stats, out = retire(ctx, 2, 6, 0, 0, 1, Z - 2)
        assert stats == want_stats and np.array_equal(out, want_out)
        gst, gfl = ctx.coh_download()
        assert np.array_equal(gst, want_st) and np.array_equal(gfl, fl)
        assert select(ctx, 1 << 2, 1 << 2, want_list=False)[1] == int(
            ((st[[0, Z - 1]] >> 2) & 1).sum())     # only the two pages outside the range keep it


def test_scan_of_more_than_one_step():
    """4098 tiles. The sum kernel scans 16 tiles per thread and 256 threads per step, 4096 tiles a
    step, so this table takes a second step: the carry, the groups' counts kept from a step's load
    to its store, the held and orphan sums of a thread over two groups, and list entries past tile
    4096. An odd `first` and a tail of 3 pages; homes by `per`, some equal to the node that leaves
    and some past the nodes. Expectations from the model's whole-array form (held to the per-page
    loop by tests/test_sweep.py)."""
    Z = 4097 * T + 3
    st, fl = host_table(Z, seed=145, write_pct=30, most=2)
    x, heir, base, per, first, n = 5, 0, 3 << 20, 1400000, 1, Z - 2
    want_st, want_stats, want_out = sm.retire_vec(st, x, heir, base, per, first, n)
    want_pages, want_count = sm.select_vec(st, 1 << x, 1 << x, base, first, n)
    past = base + 4096 * T
    assert (want_out & 0x7FFFFFFF).max() >= past and want_pages.max() >= past
    assert want_stats["held"] == want_count > want_stats["moved"] > want_stats["orphaned"] > 0
    homes = (want_out & 0x7FFFFFFF) // per
    assert (homes == x).any() and (homes >= 8).any() and (homes < x).any()
    with table_ctx(Z) as ctx:
        ctx.coh_upload(st, fl)
        pages, count = select(ctx, 1 << x, 1 << x, base, first, n)
        assert count == want_count and np.array_equal(pages, want_pages)
        stats, out = retire(ctx, x, heir, base, per, first, n, dry=True)
        assert stats == want_stats and np.array_equal(out, want_out)
        assert np.array_equal(ctx.coh_download()[0], st)
        stats, out = retire(ctx, x, heir, base, per, first, n)
        assert stats == want_stats and np.array_equal(out, want_out)
        gst, gfl = ctx.coh_download()
        assert np.array_equal(gst, want_st) and np.array_equal(gfl, fl)
        stats, _ = retire(ctx, x, heir, base, per, first, n, want_list=False)
        assert stats == ZERO
        # a capacity that ends inside the second step's tiles
        cap = 4096 * T + 1000
        pages, count = select(ctx, 0, 0, base, first, n, cap=cap)
        assert count == n and np.array_equal(pages, base + first + np.arange(cap))


RANGES = [(1, 1), (1, 2), (2, 1), (63, 3), (65, 2 * T - 1), (T - 1, T + 3), (T + 1, 511),
          (3, 3 * T + 100 - 3 - 2), (3 * T + 99, 1), (511, 513)]


def test_sub_ranges_with_odd_ends():
    Z = 3 * T + 100
    st, fl = host_table(Z, seed=141)
    with table_ctx(Z) as ctx:
        for first, n in RANGES:
            want_st, _, _ = check_retire(ctx, st, fl, 1, 4, base=12345, first=first, n=n,
                                         tag=(first, n))
            assert np.array_equal(want_st[:first], st[:first])       # (what the device equalled)
            assert np.array_equal(want_st[first + n:], st[first + n:])
            ctx.coh_upload(st, fl)
            want = check_select(ctx, st, 1 << 1, 1 << 1, 12345, first, n, tag=(first, n))
            assert n < 64 or want[1] > 0
            assert check_select(ctx, st, 0, 0, 9, first, n)[1] == n


# ------------------------------------------------------------------------------ retire forms
def gpu_made_table(ctx, n_nodes):
    """The table of ctx (initialised for n_nodes) after a GPU coherence batch, as downloaded; it is
    what the oracle makes of the same events."""
    Z = ctx.n_pages
    counts = np.random.default_rng(142).integers(0, 9, Z).astype(np.uint64)
    ev = ctx.gen_events(counts, seed=143, n_nodes=n_nodes, write_pct=30)
    ctx.coherence_batch(ev)
    ev.free()
    st, fl = ctx.coh_download()
    ost, ofl = oracle.coh_init(Z, n_nodes)
    rc, _ = oracle.coherence(ost, ofl, oracle.gen_events(counts, seed=143, n_nodes=n_nodes,
                                                         write_pct=30), n_nodes=n_nodes)
    assert rc == 0 and np.array_equal(st, ost) and np.array_equal(fl, ofl)
    return st, fl


@pytest.fixture(scope="module")
def gpu_made():
    """A table a GPU coherence batch produced, 8 nodes."""
    with table_ctx(2 * T + 77) as ctx:
        st, fl = gpu_made_table(ctx, 8)
        yield ctx, st, fl


@pytest.mark.parametrize("x", range(8))
def test_every_node_retired_from_a_gpu_made_table(gpu_made, x):
    ctx, st, fl = gpu_made
    per = -(-len(st) // 8)   # coh_init's homes: x's own block falls to the heir
    for heir, p in (((x + 1) % 8, 0), ((x + 5) % 8, per)):
        _, stats, _ = check_retire(ctx, st, fl, x, heir, per=p, tag=(x, heir, p))
        assert stats["held"] > stats["moved"] > stats["orphaned"] > 0


@pytest.mark.parametrize("n_nodes", [2, 3, 4, 5, 6, 7])
def test_every_node_of_a_smaller_cluster(n_nodes):
    """Clusters of 2 to 7 nodes, each table made by a GPU coherence batch, every node retired in
    turn, with the heir alone and with coh_init's homes. (A table of one node has nobody to retire
    to: heir == node is refused, see the refusals.)"""
    Z = 700
    with table_ctx(Z, n_nodes) as ctx:
        st, fl = gpu_made_table(ctx, n_nodes)
        for x in range(n_nodes):
            for per in (0, -(-Z // n_nodes)):
                _, stats, _ = check_retire(ctx, st, fl, x, (x + 1) % n_nodes, per=per,
                                           n_nodes=n_nodes, tag=(n_nodes, x, per))
                assert stats["held"] >= stats["moved"] > 0


def test_homes_past_the_nodes_and_homes_that_left():
    """per = 1000 with a base near the end of node 6's block: pages at homes 6, 7 and 8 (past the 8
    nodes); retiring 6 and 7 sends their own blocks, and the block past the nodes, to the heir."""
    Z = 2600
    st, fl = host_table(Z, seed=160)
    base = 6 * 1000 + 500
    with table_ctx(Z) as ctx:
        for x, heir in ((6, 7), (7, 0), (2, 6)):
            want_st, _, out = check_retire(ctx, st, fl, x, heir, base=base, per=1000, tag=x)
            owners = {h: set(((want_st[(out & 0x7FFFFFFF) - base] >> 8) & 0xFF)[
                ((out & 0x7FFFFFFF) // 1000) == h].tolist()) for h in (6, 7, 8)}
            assert owners[8] == {heir}
            assert owners[6] == {heir if x == 6 else 6} and owners[7] == {heir if x == 7 else 7}


def test_hand_made_words():
    Z = 3 * 64
    x, heir = 4, 1
    st = np.zeros(Z, np.uint32)                      # INVALID everywhere else
    fl = (np.arange(Z, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    st[64:128] = word(0xFF, x, sm.SHARED)            # all-8-node copysets, owned by x
    st[70] = word(0xFF, 2, sm.SHARED, 1)             # ... and by another node
    st[130] = word(1 << x, x, sm.EXCLUSIVE, 1)       # an orphan
    st[131] = word(1 << x, x, sm.EXCLUSIVE, 0)       # beside a page x owned alone but never wrote
    st[132] = word(1 << x | 1 << 6, x, sm.SHARED, 1)  # and one somebody else still holds
    st[191] = word(1 << heir, heir, sm.SHARED)       # a lone owner stays SHARED
    st[5] = 0x1FF | DIRTY                            # INVALID with stray bits: not touched
    with table_ctx(Z) as ctx:
        want_st, stats, out = check_retire(ctx, st, fl, x, heir, base=1 << 20)
        assert stats == {"held": 64 + 3, "moved": 63 + 3, "orphaned": 1}
        assert out[-3:].tolist() == [(1 << 20) + 130 | 1 << 31, (1 << 20) + 131, (1 << 20) + 132]
        assert want_st[5] == st[5] and want_st[0] == 0 and want_st[191] == st[191]
        assert sm.fields(int(want_st[64])) == (0xFF & ~(1 << x), heir, sm.SHARED, 0)
        assert sm.fields(int(want_st[130])) == (1 << heir, heir, sm.EXCLUSIVE, 1)
        assert sm.fields(int(want_st[132])) == (1 << 6 | 1 << heir, heir, sm.SHARED, 1)


# ------------------------------------------------------------------------------ capacity
def test_cap_below_the_count_count_only_and_an_empty_range(gpu_made):
    ctx, st, fl = gpu_made
    Z = len(st)
    want_st, want_stats, want_out = sm.retire(st, 3, 0, 50, 0, 1, Z - 1)
    want_pages, want_count = sm.select(st, 1 << 3, 1 << 3, 50, 1, Z - 1)
    assert want_stats["moved"] > 100 and want_count > 100
    ctx.coh_upload(st, fl)
    for cap in (1, 100):
        pages, count = select(ctx, 1 << 3, 1 << 3, 50, 1, Z - 1, cap=cap)
        assert count == want_count and np.array_equal(pages, want_pages[:cap])
        stats, out = retire(ctx, 3, 0, 50, 0, 1, Z - 1, cap=cap, dry=True)
        assert stats == want_stats and np.array_equal(out, want_out[:cap])
    assert select(ctx, 1 << 3, 1 << 3, 50, 1, Z - 1, want_list=False)[1] == want_count
    # an empty range: zero counts, nothing else; a wet retire with a short list does the whole range
    for first in (0, 7, Z):
        stats, out = retire(ctx, 3, 0, first=first, n=0, cap=4)
        assert stats == ZERO and len(out) == 0
        assert select(ctx, 0, 0, first=first, n=0, cap=4)[1] == 0
    assert np.array_equal(ctx.coh_download()[0], st)
    stats, out = retire(ctx, 3, 0, 50, 0, 1, Z - 1, cap=1)
    assert stats == want_stats and np.array_equal(out, want_out[:1])
    stats, out = retire(ctx, 3, 0, 50, 0, 1, Z - 1, want_list=False)
    assert stats == ZERO
    gst, gfl = ctx.coh_download()
    assert np.array_equal(gst, want_st) and np.array_equal(gfl, fl)


# ------------------------------------------------------------------------------ fold after retire
@pytest.mark.parametrize("variant,per_page", [(0, 1), (1, 6), (2, 6)])
def test_fold_after_retire(gpu_made, variant, per_page):
    """The retired table is a valid fold input: a further GPU batch equals the oracle's fold of the
    model-retired table. variant 0 with a small batch: the chained form; 1: the streaming fold; 2:
    the single-pass fold. The retired node takes part in the events again."""
    ctx, st, fl = gpu_made
    Z = len(st)
    want_st, _, _ = sm.retire(st, 5, 2, 0, -(-Z // 8), 0, Z)
    rng = np.random.default_rng(170 + variant)
    counts = np.zeros(Z, np.uint64)
    if variant == 0:
        counts[rng.choice(Z, 300, replace=False)] = per_page
    else:
        counts[:] = rng.integers(0, 2 * per_page, Z)
    ev = oracle.gen_events(counts, seed=171, n_nodes=8, write_pct=30)
    want_fl = fl.copy()
    rc, want_tot = oracle.coherence(want_st, want_fl, ev)
    assert rc == 0
    with tuned(coh_variant=variant):
        ctx.coh_upload(st, fl)
        retire(ctx, 5, 2, per=-(-Z // 8), want_list=False)
        tot = ctx.coherence_batch(ev)
    gst, gfl = ctx.coh_download()
    assert tot == want_tot
    assert np.array_equal(gst, want_st) and np.array_equal(gfl, want_fl)


# ------------------------------------------------------------------------------ select
def test_select_questions(gpu_made):
    ctx, st, fl = gpu_made
    ctx.coh_upload(st, fl)
    base = 1 << 16
    for d in range(8):
        held = check_select(ctx, st, 1 << d, 1 << d, base, tag=("holds", d))
        own = check_select(ctx, st, 0xFF00 | DIRTY, d << 8 | DIRTY, base, tag=("owns dirty", d))
        assert held[1] > own[1] > 0
    excl = check_select(ctx, st, 3 << 16, EXCL, base)
    assert 0 < excl[1] < len(st)
    everything = check_select(ctx, st, 0, 0, base)
    assert everything[0].tolist() == list(range(base, base + len(st)))
    assert check_select(ctx, st, 0xFF, 0x100, base)[1] == 0      # a value outside the mask
    assert np.array_equal(ctx.coh_download()[0], st)


def test_python_wrappers(gpu_made):
    ctx, st, fl = gpu_made
    ctx.coh_upload(st, fl)
    want_st, want_stats, want_out = sm.retire(st, 1, 7, 9, 0, 3, 1000)
    for dry in (True, False):
        r = ctx.coh_retire(1, 7, base=9, first=3, n=1000, dry=dry)
        assert {k: r[k] for k in ZERO} == want_stats
        assert np.array_equal(r["pages"], want_out & 0x7FFFFFFF)
        assert np.array_equal(r["orphan_flags"], (want_out >> 31) != 0)
    assert np.array_equal(ctx.coh_download()[0], want_st)
    pages, count = ctx.coh_select(1 << 7, 1 << 7, base=9)
    want = sm.select(want_st, 1 << 7, 1 << 7, 9)
    assert count == want[1] and np.array_equal(pages, want[0])
    assert ctx.coh_select(1 << 7, 1 << 7, cap=0)[1] == want[1]
    assert ctx.coh_retire(1, 7, cap=0)["moved"] == int(
        ((((want_st >> 8) & 0xFF) == 1) & ((want_st >> 16) & 3 != 0)).sum())


# ------------------------------------------------------------------------------ rebuild chain
def test_restarted_node_is_rebuilt_by_select_then_fetch():
    """2 ranks on one GPU (loopback): each home's select(bit(1)) over its shard, with the shard's
    base, is rank 1's fetch list as it stands (strictly ascending, global): the home copies arrive
    in rank 1's CURRENT and TWIN."""
    G, Z = 2, 130
    per = fm.per_of(Z, G)
    rng = np.random.default_rng(180)
    ctxs = [ga.Context(Z) for _ in range(G)]
    host = []
    for c in ctxs:
        h = {a: rng.integers(0, 256, (Z, 4096), dtype=np.uint8) for a in ("twin", "current",
                                                                        "replica")}
        for a, pages in h.items():
            c.upload(a, pages)
        host.append(h)
    comms = exchange.Comm.loopback(ctxs)
    pts = [table_ctx(per, G) for _ in range(G)]
    try:
        want_cur = host[1]["current"].copy()
        for h in range(G):
            st = np.where(rng.random(per) < 0.4, word(3, 0, sm.SHARED), word(1, 0, sm.EXCLUSIVE))
            st = st.astype(np.uint32)
            pts[h].coh_upload(st, np.zeros(per, np.uint32))
            base, block = fm.block_of(h, Z, G)
            lst = pts[h].buffer(4 * per)
            cnt = pts[h].buffer(8)
            assert lib().gdsm_coh_select(pts[h].handle, 2, 2, base, 0, block, lst.ptr, per,
                                         cnt.ptr) == 0
            pts[h].sync()
            m = int(cnt.download(np.uint64, 1)[0])
            want_list = base + np.flatnonzero(st[:block] & 2)
            assert m == len(want_list) > 0
            errs = []

            def rank(r):
                try:
                    exchange.fetch(ctxs[r], comms[r], lst if r == 1 else None, None,
                                   m if r == 1 else 0, Z)
                    ctxs[r].sync()
                except BaseException as e:  # noqa: BLE001
                    errs.append(e)
            th = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=60)
            assert not errs and not any(t.is_alive() for t in th), errs
            want_cur[want_list] = host[h]["replica"][want_list - base]
            lst.free()
            cnt.free()
        assert np.array_equal(ctxs[1].download("current"), want_cur)
        assert np.array_equal(ctxs[1].download("twin")[want_list], want_cur[want_list])
        assert np.array_equal(ctxs[0].download("current"), host[0]["current"])
    finally:
        for c in comms:
            c.close()
        for c in ctxs + pts:
            c.close()


# ------------------------------------------------------------------------------ refusals, recording
def test_immediate_refusals():
    Z = 100
    lb = lib()
    with ga.Context(Z, arenas=()) as ctx:
        out, tot = ctx.buffer(4 * Z), ctx.buffer(24)
        h = ctx.handle
        # no page table yet
        assert lb.gdsm_coh_retire(h, 0, 1, 0, 0, 0, Z, out.ptr, Z, tot.ptr, 0) == -errno.EINVAL
        assert lb.gdsm_coh_select(h, 0, 0, 0, 0, Z, out.ptr, Z, tot.ptr) == -errno.EINVAL
        ctx.coh_init(4)
        st0, fl0 = ctx.coh_download()
        big = 1 << 28   # GDSM_MAX_COH_PAGES
        bad_retire = [
            (None, 0, 1, 0, 0, 0, Z, out.ptr, Z, tot.ptr, 0),       # no context
            (h, 4, 1, 0, 0, 0, Z, out.ptr, Z, tot.ptr, 0),          # node >= n_nodes
            (h, 0, 4, 0, 0, 0, Z, out.ptr, Z, tot.ptr, 0),          # heir >= n_nodes
            (h, 2, 2, 0, 0, 0, Z, out.ptr, Z, tot.ptr, 0),          # heir == node
            (h, 0, 1, 0, 0, 0, Z, out.ptr, Z, tot.ptr, 2),          # unknown flags
            (h, 0, 1, 0, 0, 0, Z, out.ptr, Z, tot.ptr, 3),
            (h, 0, 1, 0, 0, 1, Z, out.ptr, Z, tot.ptr, 0),          # first + n > n_pages
            (h, 0, 1, 0, 0, Z + 1, 0, out.ptr, Z, tot.ptr, 0),
            (h, 0, 1, 0, 0, 0, (1 << 64) - 1, out.ptr, Z, tot.ptr, 0),
            (h, 0, 1, 0, 0, 2, (1 << 64) - 1, out.ptr, Z, tot.ptr, 0),
            (h, 0, 1, big - Z + 1, 0, 0, Z, out.ptr, Z, tot.ptr, 0),  # base + first + n > 2^28
            (h, 0, 1, big - Z + 1, 0, 1, Z - 1, out.ptr, Z, tot.ptr, 1),
            (h, 0, 1, (1 << 64) - 1, 0, 0, 1, out.ptr, Z, tot.ptr, 0),
            (h, 0, 1, 0, 0, 0, Z, None, Z, tot.ptr, 0),             # a capacity with no list
        ]
        for args in bad_retire:
            assert lb.gdsm_coh_retire(*args) == -errno.EINVAL, args
        bad_select = [
            (None, 0, 0, 0, 0, Z, out.ptr, Z, tot.ptr),
            (h, 0, 0, 0, 1, Z, out.ptr, Z, tot.ptr),
            (h, 0, 0, 0, Z + 1, 0, out.ptr, Z, tot.ptr),
            (h, 0, 0, 0, 1, (1 << 64) - 1, out.ptr, Z, tot.ptr),
            (h, 0, 0, big - Z + 1, 0, Z, out.ptr, Z, tot.ptr),
            (h, 0, 0, (1 << 64) - 1, 0, 1, out.ptr, Z, tot.ptr),
            (h, 0, 0, 0, 0, Z, None, 1, tot.ptr),
        ]
        for args in bad_select:
            assert lb.gdsm_coh_select(*args) == -errno.EINVAL, args
        # the edges that are allowed: the last global page, NULL totals, a list nobody asked for
        assert lb.gdsm_coh_select(h, 0, 0, big - Z, 0, Z, out.ptr, Z, None) == 0
        assert lb.gdsm_coh_retire(h, 0, 1, big - Z, 0, 0, Z, None, 0, None, 1) == 0
        assert lb.gdsm_coh_retire(h, 0, 1, 0, 0, Z, 0, None, 0, tot.ptr, 0) == 0
        ctx.sync()   # none of the refusals left anything behind
        assert out.download(np.uint32, Z).tolist() == list(range(big - Z, big))
        assert tot.download(np.uint64, 3).tolist() == [0, 0, 0]
        st, fl = ctx.coh_download()
        assert np.array_equal(st, st0) and np.array_equal(fl, fl0)
    with table_ctx(4, 1) as one:   # one node: there is no heir
        assert lb.gdsm_coh_retire(one.handle, 0, 0, 0, 0, 0, 4, None, 0, None, 0) == -errno.EINVAL
        assert lb.gdsm_coh_select(one.handle, 1, 1, 0, 0, 4, None, 0, None) == 0
        one.sync()


def test_recorded_sweeps_read_the_table_again():
    Z = 3 * T + 100
    st, fl = host_table(Z, seed=190)
    with table_ctx(Z) as ctx:
        ctx.coh_upload(st, fl)
        fill = np.full(Z + PAD, CANARY, np.uint32)
        d_sel, d_mov = ctx.buffer(4 * (Z + PAD)), ctx.buffer(4 * (Z + PAD))
        d_cnt, d_stats = ctx.buffer(8), ctx.buffer(24)
        lb, h = lib(), ctx.handle
        sel = (h, 1 << 6, 1 << 6, 40, 1, Z - 1, d_sel.ptr, Z, d_cnt.ptr)
        ret = (h, 6, 0, 40, 0, 1, Z - 1, d_mov.ptr, Z, d_stats.ptr, 0)
        # a short sweep before recording: the workspace of one tile
        assert lb.gdsm_coh_select(h, 0, 0, 0, 0, 100, None, 0, d_cnt.ptr) == 0
        ctx.sync()
        ctx.capture_begin()
        try:
            assert lb.gdsm_coh_select(h, 0, 0, 0, 0, 100, None, 0, d_cnt.ptr) == 0
            assert lb.gdsm_coh_select(*sel) == -errno.EBUSY    # would have to grow
            assert lb.gdsm_coh_retire(*ret) == -errno.EBUSY
        finally:
            ctx.capture_end().destroy()
        assert lb.gdsm_coh_select(*sel) == 0                   # sized by one call
        ctx.sync()
        ctx.capture_begin()
        try:
            assert lb.gdsm_coh_select(*sel) == 0
            assert lb.gdsm_coh_retire(*ret) == 0
        finally:
            g = ctx.capture_end()
        assert np.array_equal(ctx.coh_download()[0], st)        # recorded, not run
        st2, fl2 = host_table(Z, seed=191, write_pct=40)        # another table
        ctx.coh_upload(st2, fl2)
        d_sel.upload(fill)
        d_mov.upload(fill)
        g.launch(ctx)
        ctx.sync()
        want_pages, want_count = sm.select(st2, 1 << 6, 1 << 6, 40, 1, Z - 1)
        want_st, want_stats, want_out = sm.retire(st2, 6, 0, 40, 0, 1, Z - 1)
        assert d_cnt.download(np.uint64, 1).tolist() == [want_count]
        assert d_stats.download(np.uint64, 3).tolist() == [want_stats[k] for k in ZERO]
        got_sel, got_mov = d_sel.download(np.uint32, Z + PAD), d_mov.download(np.uint32, Z + PAD)
        assert np.array_equal(got_sel[:want_count], want_pages)
        assert (got_sel[want_count:] == CANARY).all()
        assert np.array_equal(got_mov[:len(want_out)], want_out)
        assert (got_mov[len(want_out):] == CANARY).all()
        gst, gfl = ctx.coh_download()
        assert np.array_equal(gst, want_st) and np.array_equal(gfl, fl2)
        g.destroy()
