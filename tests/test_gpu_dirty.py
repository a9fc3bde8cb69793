"""gdsm_dirty_scan on the GPU (docs/SPEC.md §12) against the numpy model tests/dirty_model.py,
exactly (pages, positions, count, bound): list lengths around the wave's 16 entries and the
workgroup's 64-entry tile, a list long enough for the tile scan to pass its first block, every list
form, page patterns that single out a byte, a quarter and a lane, dirty layouts around the tile
borders, each arena pair, a capacity below the count, an id out of range, the raw entry point on
torch tensors, the round scan -> release -> scan again, and a recorded scan."""
import errno

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd.gdsm import GdsmError, lib
from oracle import oracle
from tests import dirty_model as dm

pytestmark = pytest.mark.gpu

Z = 300
TILE = 64          # list entries per workgroup (one flag word)
CANARY = 0xDEADBEEF
PAD = 8            # canary words behind every output
KIND = {"twin": ga.TWIN, "current": ga.CURRENT, "replica": ga.REPLICA}
# page p of CURRENT against TWIN, by p % 10
CLEAN_KINDS = (0, 9)


def make_arenas():
    """TWIN random; CURRENT = TWIN but, by p % 10: 1 byte 0, 2 byte 4095, 3..6 one byte of quarter
    0..3 at lanes 5, 16, 27, 38, 7 every byte, 8 alternating bytes (0 and 9 stay equal). REPLICA =
    CURRENT but for one byte of the pages with p % 7 == 3."""
    rng = np.random.default_rng(130)
    twin = rng.integers(0, 256, (Z, 4096), dtype=np.uint8)
    cur = twin.copy()
    for p in range(Z):
        k = p % 10
        if k == 1:
            cur[p, 0] ^= 0x01
        elif k == 2:
            cur[p, 4095] ^= 0x80
        elif 3 <= k <= 6:
            q = k - 3
            cur[p, 1024 * q + 16 * (5 + 11 * q) + 3] ^= 0x10
        elif k == 7:
            cur[p] ^= 0xFF
        elif k == 8:
            cur[p, 0::2] ^= 0xFF
    rep = cur.copy()
    rep[3::7, 2222] ^= 0x04
    return {"twin": twin, "current": cur, "replica": rep}


@pytest.fixture(scope="module")
def shard():
    host = make_arenas()
    ctx = ga.Context(Z)
    for a, pages in host.items():
        ctx.upload(a, pages)
    yield ctx, host
    ctx.close()


def scan(ctx, a, b, ids, n, cap=None, want_pages=True, want_pos=True):
    """gdsm_dirty_scan into canary-filled buffers: (pages, pos, count, bound) as downloaded, the
    outputs cut to what the call may have written; asserts that nothing behind that was."""
    cap = n if cap is None else cap
    fill = np.full(cap + PAD, CANARY, np.uint32)
    d_ids = ctx.ids(ids) if ids is not None and len(ids) else None
    d_pages = ctx.buffer(4 * (cap + PAD)).upload(fill) if want_pages else None
    d_pos = ctx.buffer(4 * (cap + PAD)).upload(fill) if want_pos else None
    d_stats = ctx.buffer(16).upload(np.full(2, 0xA5A5A5A5A5A5A5A5, np.uint64))
    rc = lib().gdsm_dirty_scan(ctx.handle, KIND[a], KIND[b], ctx._ptr(d_ids), n,
                               ctx._ptr(d_pages), ctx._ptr(d_pos), cap, d_stats.ptr)
    assert rc == 0, rc
    try:
        ctx.sync()
    finally:
        count, bound = (int(x) for x in d_stats.download(np.uint64, 2))
        used = min(count, cap)
        out = []
        for buf in (d_pages, d_pos):
            if buf is None:
                out.append(None)
                continue
            got = buf.download(np.uint32, cap + PAD)
            assert (got[used:] == CANARY).all()
            out.append(got[:used])
            buf.free()
        d_stats.free()
        if d_ids is not None:
            d_ids.free()
    return out[0], out[1], count, bound


def check(ctx, host, a, b, ids, n, tag=""):
    got = scan(ctx, a, b, ids, n)
    want = dm.dirty_scan(host[a], host[b], ids, n)
    assert (got[2], got[3]) == (want[2], want[3]), tag
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), tag
    return want


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 4 * TILE + 3])
def test_scan_equals_model(shard, n):
    ctx, host = shard
    rng = np.random.default_rng(n)
    lists = {"none": None,
             "permutation": rng.permutation(Z)[:n].astype(np.uint32),
             "repeats": rng.integers(0, max(1, min(Z, n // 2 + 1)), n).astype(np.uint32)}
    for kind, ids in lists.items():
        want = check(ctx, host, "twin", "current", ids, n, kind)
        if ids is None and n:  # pages 0 .. n-1: eight of every ten differ
            assert want[2] == sum(p % 10 not in CLEAN_KINDS for p in range(n))


def test_long_list_of_repeats(shard):
    """1094 tiles: the one-workgroup scan of the tile counts takes five rounds of 256."""
    ctx, host = shard
    n = 70001
    ids = np.random.default_rng(131).integers(0, Z, n).astype(np.uint32)
    want = check(ctx, host, "twin", "current", ids, n)
    assert 0.7 * n < want[2] < 0.9 * n


def test_page_patterns_one_by_one(shard):
    """Every pattern alone in a list, so that a byte, a quarter or a lane left out of the reduction
    shows as a missing page, and its bound as the model gives it."""
    ctx, host = shard
    bounds = {}
    for k in range(10):
        ids = np.array([20 + k], np.uint32)
        pages, pos, count, bound = scan(ctx, "twin", "current", ids, 1)
        clean = k in CLEAN_KINDS
        assert count == (0 if clean else 1) and pages.tolist() == ([] if clean else [20 + k]), k
        assert bound == dm.dirty_scan(host["twin"], host["current"], ids)[3], k
        bounds[k] = bound
    assert bounds[0] == 0 and bounds[1] == 52 and bounds[6] == 52
    assert bounds[7] == 10244 and bounds[8] == 10244  # 4 + 48 x 256 chunks, capped


def test_dirty_layouts(shard):
    ctx, host = shard
    clean = np.array([p for p in range(Z) if p % 10 in CLEAN_KINDS], np.uint32)
    dirty = np.array([p for p in range(Z) if p % 10 not in CLEAN_KINDS], np.uint32)
    n = 4 * TILE + 3
    rng = np.random.default_rng(132)
    none = rng.choice(clean, n)
    every = rng.choice(dirty, n)
    one_per_64 = none.copy()
    for t in range(n // TILE):
        one_per_64[TILE * t + (7 * t + 3) % TILE] = dirty[t]
    edges = none.copy()
    at = [15, 16, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 4 * TILE - 1, 4 * TILE, n - 1]
    edges[at] = rng.choice(dirty, len(at))
    for tag, ids, count in (("none", none, 0), ("all", every, n), ("one per 64", one_per_64, 4),
                            ("edges", edges, len(at))):
        want = check(ctx, host, "twin", "current", ids, n, tag)
        assert want[2] == count, tag
    assert check(ctx, host, "twin", "current", edges, n)[1].tolist() == at


@pytest.mark.parametrize("a,b", [("twin", "current"), ("replica", "current"), ("current", "twin")])
def test_arena_pairs_and_inputs_unchanged(shard, a, b):
    ctx, host = shard
    want = check(ctx, host, a, b, None, Z)
    if a == "replica":
        assert want[0].tolist() == list(range(3, Z, 7)) and want[3] == 52 * want[2]
    for k, pages in host.items():
        assert np.array_equal(ctx.download(k), pages), k


def test_cap_below_the_count_and_count_only(shard):
    ctx, host = shard
    ids = np.random.default_rng(133).integers(0, Z, 500).astype(np.uint32)
    want = dm.dirty_scan(host["twin"], host["current"], ids)
    assert want[2] > 100
    for cap in (1, 100):
        pages, pos, count, bound = scan(ctx, "twin", "current", ids, len(ids), cap=cap)
        assert (count, bound) == (want[2], want[3])      # the full count and bound
        assert np.array_equal(pages, want[0][:cap]) and np.array_equal(pos, want[1][:cap])
    # only one of the two outputs
    pages, pos, count, _ = scan(ctx, "twin", "current", ids, len(ids), want_pos=False)
    assert pos is None and np.array_equal(pages, want[0]) and count == want[2]
    pages, pos, count, _ = scan(ctx, "twin", "current", ids, len(ids), want_pages=False)
    assert pages is None and np.array_equal(pos, want[1])
    # count only
    pages, pos, count, bound = scan(ctx, "twin", "current", ids, len(ids), cap=0,
                                    want_pages=False, want_pos=False)
    assert (count, bound) == (want[2], want[3])


def test_id_out_of_range(shard):
    ctx, host = shard
    ids = np.array([21, Z, 27, 0xFFFFFFFF, 20, 28] + [22] * 20, np.uint32)
    with pytest.raises(GdsmError) as ei:
        scan(ctx, "twin", "current", ids, len(ids))
    assert ei.value.errno == errno.EINVAL
    ctx.sync()  # reported once
    # the same call again, the error taken off by a sync of our own
    d_ids = ctx.ids(ids)
    dl = ctx.dirty_scan(ids=d_ids, want_pos=True)
    with pytest.raises(GdsmError):
        ctx.sync()
    want = dm.dirty_scan(host["twin"], host["current"], ids)
    assert want[0][:3].tolist() == [21, 27, 28] and want[2] == 23
    assert dl.count == want[2] and dl.bound == want[3]
    assert np.array_equal(dl.pages.download(np.uint32, want[2]), want[0])
    assert np.array_equal(dl.pos.download(np.uint32, want[2]), want[1])
    dl.free()
    d_ids.free()


def test_immediate_refusals_on_a_context(shard):
    ctx, _ = shard
    out = ctx.buffer(64)
    lb, h = lib(), ctx.handle
    assert lb.gdsm_dirty_scan(h, ga.TWIN, ga.TWIN, None, 4, out.ptr, None, 4, None) == -22
    assert lb.gdsm_dirty_scan(h, 3, ga.CURRENT, None, 4, out.ptr, None, 4, None) == -22
    assert lb.gdsm_dirty_scan(h, ga.TWIN, -1, None, 4, out.ptr, None, 4, None) == -22
    assert lb.gdsm_dirty_scan(h, ga.TWIN, ga.CURRENT, None, 4, None, None, 4, None) == -22
    assert lb.gdsm_dirty_scan(h, ga.TWIN, ga.CURRENT, None, (1 << 32) + 1, out.ptr, None, 4,
                              None) == -22
    with ga.Context(4, arenas=("twin", "current")) as two:
        assert lb.gdsm_dirty_scan(two.handle, ga.REPLICA, ga.CURRENT, None, 4, out.ptr, None, 4,
                                  None) == -22
        assert lb.gdsm_dirty_scan(two.handle, ga.TWIN, ga.CURRENT, None, 4, out.ptr, None, 4,
                                  None) == 0
        two.sync()
    ctx.sync()  # none of the refusals left anything behind
    out.free()


def test_python_result_object(shard):
    ctx, host = shard
    want = dm.dirty_scan(host["twin"], host["current"])
    dl = ctx.dirty_scan()
    assert dl.pos is None and dl.cap == Z
    assert (dl.count, dl.bound) == (want[2], want[3])
    assert np.array_equal(dl.pages.download(np.uint32, dl.count), want[0])
    dl.free()
    dl = ctx.dirty_scan("replica", "current", cap=0)
    assert dl.pages is None and dl.pos is None and dl.count == len(range(3, Z, 7))
    dl.free()


def test_raw_on_torch_tensors():
    import torch
    host = make_arenas()
    a = torch.from_numpy(host["twin"]).cuda()
    b = torch.from_numpy(host["current"]).cuda()
    ids = np.random.default_rng(134).integers(0, Z, 777).astype(np.uint32)
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    lb = lib()
    for lst, n in ((None, Z), (ids, len(ids))):
        want = dm.dirty_scan(host["twin"], host["current"], lst, n)
        pages = torch.full((n + PAD,), -1, dtype=torch.int32, device="cuda")
        pos = torch.full((n + PAD,), -1, dtype=torch.int32, device="cuda")
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")
        need = lb.gdsm_dirty_scan_workspace_bytes(n)
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        args = (a.data_ptr(), b.data_ptr(), d_ids.data_ptr() if lst is not None else None, n,
                pages.data_ptr(), pos.data_ptr(), n, stats.data_ptr())
        assert lb.gdsm_dirty_scan_raw(*args, ws.data_ptr(), need - 1, stream) == -22
        assert lb.gdsm_dirty_scan_raw(*args, None, need, stream) == -22
        assert lb.gdsm_dirty_scan_raw(*args, ws.data_ptr(), need, stream) == 0
        torch.cuda.synchronize()
        assert stats.cpu().tolist() == [want[2], want[3]]
        got_pages = pages.cpu().numpy().view(np.uint32)
        got_pos = pos.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_pages[:want[2]], want[0])
        assert np.array_equal(got_pos[:want[2]], want[1])
        assert (got_pages[want[2]:] == 0xFFFFFFFF).all() and (got_pos[want[2]:] == 0xFFFFFFFF).all()
    assert np.array_equal(a.cpu().numpy(), host["twin"])
    assert np.array_equal(b.cpu().numpy(), host["current"])


def test_round_scan_release_scan_again():
    """The writer's end of a round: which pages? -> a stream sized by the bound -> release."""
    rng = np.random.default_rng(135)
    base = rng.integers(0, 256, (Z, 4096), dtype=np.uint8)
    cur = base.copy()
    written = np.sort(rng.choice(Z, Z // 20, replace=False))
    for p in written:
        k = int(rng.integers(1, 200))
        cur[p, rng.integers(0, 4096, k)] ^= rng.integers(1, 256, k).astype(np.uint8)
    with ga.Context(Z) as ctx:
        ctx.upload("twin", base)
        ctx.upload("replica", base)
        ctx.upload("current", cur)
        dl = ctx.dirty_scan()
        count, bound = dl.count, dl.bound
        assert count == len(written)
        assert dl.pages.download(np.uint32, count).tolist() == written.tolist()
        runs = ga.Runs(ctx, count, cap=bound)
        ctx.release(dl.pages, n=count, out=runs, apply_to="replica", retwin=True)
        assert runs.total() <= bound < count * ga.MAX_RECORD
        got = runs.to_host()
        ro, data = oracle.diff_pages(base, cur, written.astype(np.uint32))
        assert np.array_equal(got.rec_off, ro) and np.array_equal(got.data, data)
        assert np.array_equal(ctx.download("replica"), cur)
        again = ctx.dirty_scan(cap=0)
        assert again.count == 0 and again.bound == 0
        for x in (dl, again):
            x.free()
        runs.free()


def test_recorded_scan_reads_the_arenas_again():
    host = make_arenas()
    with ga.Context(Z) as ctx:
        for a, pages in host.items():
            ctx.upload(a, pages)
        fill = np.full(Z + PAD, CANARY, np.uint32)
        d_pages, d_pos = ctx.buffer(4 * (Z + PAD)), ctx.buffer(4 * (Z + PAD))
        d_stats = ctx.buffer(16)
        long_ids = ctx.ids(np.arange(4 * Z, dtype=np.uint32) % Z)
        args = (ctx.handle, ga.TWIN, ga.CURRENT, None, Z, d_pages.ptr, d_pos.ptr, Z, d_stats.ptr)
        assert lib().gdsm_dirty_scan(*args) == 0   # scan once before recording: the workspace
        ctx.sync()
        ctx.capture_begin()
        try:
            assert lib().gdsm_dirty_scan(*args) == 0
            # a list whose workspace would have to grow
            assert lib().gdsm_dirty_scan(ctx.handle, ga.TWIN, ga.CURRENT, long_ids.ptr, 4 * Z,
                                         None, None, 0, d_stats.ptr) == -errno.EBUSY
        finally:
            g = ctx.capture_end()
        cur = host["twin"].copy()        # a new interval: other pages written
        cur[5:40:3, 100] ^= 0x20
        cur[299] ^= 0xFF
        ctx.upload("current", cur)
        d_pages.upload(fill)
        d_pos.upload(fill)
        g.launch(ctx)
        ctx.sync()
        want = dm.dirty_scan(host["twin"], cur)
        assert want[0].tolist() == list(range(5, 40, 3)) + [299]
        assert d_stats.download(np.uint64, 2).tolist() == [want[2], want[3]]
        got_pages, got_pos = d_pages.download(np.uint32, Z + PAD), d_pos.download(np.uint32, Z + PAD)
        assert np.array_equal(got_pages[:want[2]], want[0])
        assert np.array_equal(got_pos[:want[2]], want[1])
        assert (got_pages[want[2]:] == CANARY).all() and (got_pos[want[2]:] == CANARY).all()
        g.destroy()
