"""gdsm_merge on the GPU (docs/SPEC.md §8) against the numpy model tests/merge_model.py: offsets,
data, per-page conflicts and the totals are compared exactly in every case; the bytes of the out
buffer the merge must not write (past the stream, past the capacity) carry a guard pattern."""
import ctypes as C

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd.gdsm import GdsmError, lib
from oracle import oracle
from tests import merge_model as mm

pytestmark = pytest.mark.gpu

GUARD = 0xA5
N_PAGES = 1024


@pytest.fixture(scope="module")
def ctx():
    with ga.Context(N_PAGES) as c:
        yield c


def d2h(ctx, ptr, dtype, count):
    out = np.empty(count, dtype)
    if out.nbytes:
        ga.gdsm.check(lib().gdsm_memcpy_d2h(ctx.handle, out.ctypes.data, ptr, out.nbytes), "d2h")
    return out


def record(runs) -> np.ndarray:
    """A record from [(off, payload bytes)] as given: not made canonical, not checked."""
    hdr = np.array([len(runs)] + [o | (len(p) << 16) for o, p in runs], "<u4").tobytes()
    pay = b"".join(bytes(p) for _, p in runs)
    return np.frombuffer(hdr + pay + b"\0" * (-len(pay) % 4), np.uint8)


def stream(records):
    """(rec_off, data) of per-page records (an empty array = an empty record)."""
    ro = np.zeros(len(records) + 1, np.uint64)
    ro[1:] = np.cumsum([len(r) for r in records])
    data = np.concatenate([np.asarray(r, np.uint8) for r in records]) if records else np.zeros(0, np.uint8)
    return ro, data.astype(np.uint8)


EMPTY = np.zeros(0, np.uint8)
GOOD = record([(100, b"good bytes"), (300, b"more")])


def upload(ctx, s):
    return ga.Runs.from_host(ctx, ga.HostRuns(np.asarray(s[0], np.uint64), np.asarray(s[1], np.uint8)))


def run_merge(ctx, streams, ids=None, out_ids=None, cap=None, einval=False, pass_out_ids=True):
    """Merges on the device and compares everything with the model; returns (model, device
    rec_off, device data). einval: the sync after the merge must report -EINVAL."""
    caps = [max(16, len(s[1])) for s in streams]
    m_ro, m_data, m_conf, m_ov, m_cf, m_bad = mm.merge_ex(streams, ids, out_ids, caps=caps)
    assert m_bad == einval
    n_out = len(m_ro) - 1
    need = int(m_ro[-1])
    cap = need if cap is None else cap
    alloc = cap + 64
    out = ga.Runs(ctx, n_out, alloc)
    guard = np.full(alloc, GUARD, np.uint8)
    ga.gdsm.check(lib().gdsm_memcpy_h2d(ctx.handle, out.s.data, guard.ctypes.data, alloc), "h2d")
    out.s.cap = cap
    dev = [upload(ctx, s) for s in streams]
    res = ctx.merge(dev, ids, out_ids if pass_out_ids else None, out=out, want_conflicts=True)
    if einval:
        with pytest.raises(GdsmError) as e:
            ctx.sync()
        assert e.value.errno == 22
    else:
        ctx.sync()
    assert out.n == n_out
    ro = d2h(ctx, out.s.rec_off, np.uint64, n_out + 1)
    raw = d2h(ctx, out.s.data, np.uint8, alloc)
    conflicts, stats = res.conflicts, res.stats
    res.free()
    for r in dev:
        r.free()
    out.s.cap = alloc
    assert np.array_equal(ro, m_ro)
    w = min(need, cap) // 4 * 4
    assert np.array_equal(raw[:w], m_data[:w])
    assert (raw[w:] == GUARD).all(), "bytes past the stream or the capacity were written"
    assert np.array_equal(conflicts, m_conf)
    assert stats == {"overlap_bytes": m_ov, "conflict_bytes": m_cf}
    return (m_ro, m_data, m_conf, m_ov, m_cf), out


# ---- 1. K = 1 identity -------------------------------------------------------------------
def test_k1_identity_config1(ctx):
    ctx.gen_pages(seed=1, mode=ga.GEN_UNIFORM, ppm=10000)
    runs = ctx.diff(n=64)
    res = ctx.merge([runs], want_conflicts=True)
    a, b = runs.to_host(), res.runs.to_host()
    assert len(a.data) > 0
    assert np.array_equal(a.rec_off, b.rec_off) and np.array_equal(a.data, b.data)
    assert res.stats == {"overlap_bytes": 0, "conflict_bytes": 0}
    assert not res.conflicts.any()
    m = mm.merge([(a.rec_off, a.data)])
    assert np.array_equal(m[0], b.rec_off) and np.array_equal(m[1], b.data)
    res.free()
    res.runs.free()
    runs.free()


# ---- 2. fusing ---------------------------------------------------------------------------
def test_abutting_runs_fuse(ctx):
    rec = record([(0, b"abcdefgh"), (8, b"ijklmnop")])
    (ro, data, *_), out = run_merge(ctx, [stream([rec])])
    assert data.tobytes() == record([(0, b"abcdefghijklmnop")]).tobytes()
    out.free()


@pytest.mark.parametrize("order", [0, 1])
def test_even_and_odd_bytes_fuse_into_one_run(ctx, order):
    rng = np.random.default_rng(2)
    page = rng.integers(0, 256, 4096, dtype=np.uint8)
    even = record([(o, page[o:o + 1]) for o in range(0, 4096, 2)])
    odd = record([(o, page[o:o + 1]) for o in range(1, 4096, 2)])
    assert len(even) == 10244
    (ro, data, _, ov, _), out = run_merge(ctx, [stream([even]), stream([odd])][::1 - 2 * order])
    assert int(ro[1]) == 4104 and ov == 0
    assert data.tobytes() == record([(0, page)]).tobytes()
    out.free()


# ---- 3. lane and chunk edges ---------------------------------------------------------------
EDGES = [(63, 65), (0, 1), (4095, 4096), (0, 4096), (15, 17), (1023, 1025)]


def test_lane_and_chunk_edges(ctx):
    rng = np.random.default_rng(3)
    a, b = [], []
    for lo, hi in EDGES:
        sh = -1 if hi == 4096 else 1  # the second stream's run, one byte along
        lo2, hi2 = max(lo + sh, 0), min(hi + sh, 4096)
        a.append(record([(lo, rng.integers(0, 256, hi - lo, dtype=np.uint8))]))
        b.append(record([(lo2, rng.integers(0, 256, hi2 - lo2, dtype=np.uint8))]))
    # a run ending at 4095 next to one starting at 0 of the following page
    a += [record([(4000, rng.integers(0, 256, 96, dtype=np.uint8))]), EMPTY]
    b += [EMPTY, record([(0, rng.integers(0, 256, 7, dtype=np.uint8))])]
    (ro, data, *_), out = run_merge(ctx, [stream(a), stream(b)])
    assert (np.diff(ro.astype(np.int64)) > 0).all()
    out.free()


# ---- 4. priority and counts ----------------------------------------------------------------
def test_priority_and_counts(ctx):
    rng = np.random.default_rng(4)
    pa = rng.integers(0, 256, 100, dtype=np.uint8)
    pb = pa.copy()
    pb[rng.choice(100, 37, replace=False)] ^= 0x5A
    A, B = stream([record([(200, pa)])]), stream([record([(200, pb)])])
    (ro, data, conf, ov, cf), out = run_merge(ctx, [A, B])
    assert (ov, cf, conf.tolist()) == (100, 37, [37]) and data[8:108].tobytes() == pb.tobytes()
    out.free()
    (ro, data, conf, ov, cf), out = run_merge(ctx, [B, A])
    assert (ov, cf) == (100, 37) and data[8:108].tobytes() == pa.tobytes()
    out.free()
    (ro, data, conf, ov, cf), out = run_merge(ctx, [A, A])
    assert (ov, cf) == (100, 0)
    out.free()


def test_eight_streams_on_one_byte(ctx):
    ss = [stream([record([(2048, bytes([v]))])]) for v in (1, 2, 1, 1, 3, 3, 3, 1)]
    (ro, data, conf, ov, cf), out = run_merge(ctx, ss)
    assert (ov, cf, conf.tolist()) == (1, 1, [1]) and data[8] == 1
    out.free()


# ---- 5. empties ----------------------------------------------------------------------------
def test_all_records_empty(ctx):
    (ro, data, *_), out = run_merge(ctx, [stream([EMPTY] * 9)] * 3)
    assert not ro.any() and len(data) == 0
    out.free()


def test_page_dirty_in_one_of_three(ctx):
    rec = record([(5, b"xyz")])
    ss = [stream([EMPTY, EMPTY, EMPTY]), stream([EMPTY, rec, EMPTY]), stream([EMPTY] * 3)]
    (ro, data, _, ov, _), out = run_merge(ctx, ss)
    assert ro.tolist() == [0, 0, len(rec), len(rec)] and data.tobytes() == rec.tobytes() and ov == 0
    out.free()


def test_one_out_entry(ctx):
    (ro, data, *_), out = run_merge(ctx, [stream([record([(9, b"q")])]), stream([record([(10, b"r")])])])
    assert data.tobytes() == record([(9, b"qr")]).tobytes()
    out.free()


# ---- 6. id join ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joined():
    rng = np.random.default_rng(6)
    twin = rng.integers(0, 256, (300, 4096), dtype=np.uint8)
    lists, streams = [], []
    for k in range(3):
        ids = np.sort(rng.choice(300, 90, replace=False)).astype(np.uint32)
        cur = twin.copy()
        for p in ids:
            for _ in range(3):
                o = int(rng.integers(0, 4040))
                cur[p, o:o + int(rng.integers(1, 56))] ^= np.uint8(k + 1)
        lists.append(ids)
        streams.append(oracle.diff_pages(twin, cur, ids=ids))
    union = np.unique(np.concatenate(lists))
    assert len(union) < 300 and len(np.intersect1d(lists[0], lists[1])) > 0
    return lists, streams, union


def test_id_join_union(ctx, joined):
    lists, streams, union = joined
    # out_ids None with host lists: the wrapper computes the union
    (ro, data, _, ov, _), out = run_merge(ctx, streams, lists, union, pass_out_ids=False)
    assert ov > 0
    out.free()


def test_id_join_subset(ctx, joined):
    lists, streams, union = joined
    _, out = run_merge(ctx, streams, lists, union[1::3])
    out.free()
    # a stream without a list beside listed ones: its record i is out entry i
    _, out = run_merge(ctx, [streams[0], streams[1]], [None, lists[1]], lists[0])
    out.free()


def test_all_lists_null(ctx, joined):
    lists, streams, union = joined
    same = [oracle.diff_pages(np.zeros((40, 4096), np.uint8),
                              np.random.default_rng(60 + k).integers(0, 2, (40, 4096), dtype=np.uint8))
            for k in range(2)]
    (_, _, _, ov, _), out = run_merge(ctx, same)
    assert ov > 0
    out.free()


# ---- 7. bulk, offsets across workgroups, apply-equivalence, associativity -------------------
@pytest.mark.parametrize("n,K,mode,ppm", [(257, 3, 1, 100000), (1000, 3, 0, 10000),
                                          (64, 8, 0, 400000)])
def test_bulk(ctx, n, K, mode, ppm):
    twin, curs, streams = mm.writer_streams(n, K, mode, ppm, oracle)
    (ro, data, _, ov, cf), out = run_merge(ctx, streams)
    assert ov > 0
    # apply-equivalence on the device
    rng = np.random.default_rng(n)
    replica = rng.integers(0, 256, (n, 4096), dtype=np.uint8)
    ctx.upload("replica", replica)
    dev = [upload(ctx, s) for s in streams]
    for r in dev:
        ctx.apply(r)
    ctx.sync()
    want = ctx.download("replica", 0, n)
    ctx.upload("replica", replica)
    out.s.cap = int(ro[-1])
    ctx.apply(out)
    ctx.sync()
    assert np.array_equal(ctx.download("replica", 0, n), want)
    # merge(merge(A, B), C...) == merge(A, B, C...)
    ab = ctx.merge(dev[:2])
    abc = ctx.merge([ab.runs] + dev[2:])
    h = abc.runs.to_host()
    assert np.array_equal(h.rec_off, ro) and np.array_equal(h.data, data)
    for x in (ab, abc):
        x.free()
        x.runs.free()
    for r in dev:
        r.free()
    out.free()


def test_largest_records_in_the_last_wave(ctx):
    """The longest records on the fourth page of a workgroup (its wave's staging buffer is the one
    farthest into the workgroup's LDS): the 10 244-B canonical record against its complement, and
    the longest record apply accepts, 2048 abutting 2-byte runs (12 292 B), which fuses into one."""
    rng = np.random.default_rng(12)
    page = rng.integers(0, 256, 4096, dtype=np.uint8)
    even = record([(o, page[o:o + 1]) for o in range(0, 4096, 2)])
    odd = record([(o, page[o:o + 1]) for o in range(1, 4096, 2)])
    abut = record([(o, page[o:o + 2]) for o in range(0, 4096, 2)])
    assert len(abut) == 12292
    for rec_a, rec_b in ((even, odd), (abut, even)):
        a, b = stream([EMPTY, GOOD, EMPTY, rec_a]), stream([GOOD, EMPTY, EMPTY, rec_b])
        (ro, data, *_), out = run_merge(ctx, [a, b])
        assert data[int(ro[3]):].tobytes() == record([(0, page)]).tobytes()
        out.free()


def test_offsets_across_scan_tiles(ctx):
    """More out pages than one 4096-page scan tile (sparse pages keep the model quick)."""
    with ga.Context(4100) as big:
        twin, curs, streams = mm.writer_streams(4100, 2, 0, 3000, oracle)
        (ro, data, _, ov, _), out = run_merge(big, streams)
        assert int(ro[4096]) > 0 and int(ro[-1]) > int(ro[4096])
        out.free()


# ---- 8. capacity ---------------------------------------------------------------------------
def test_capacity(ctx):
    twin, curs, streams = mm.writer_streams(257, 3, 1, 100000, oracle)
    need = int(mm.merge(streams)[0][-1])
    cap = need // 2 // 4 * 4
    (ro, data, *_), out = run_merge(ctx, streams, cap=cap)  # offsets complete, guard intact
    out.s.cap = cap
    with pytest.raises(GdsmError) as e:
        out.total()
    assert e.value.errno == 28 and int(ro[-1]) == need
    out.free()


# ---- 9. refusals ---------------------------------------------------------------------------
BAD_RECORDS = {
    "nruns0_size8": np.zeros(8, np.uint8),
    "run_past_page": record([(4090, b"12345678")]),
    "overlapping_runs": record([(0, b"12345678"), (4, b"abcd")]),
    "four_bytes_longer": np.concatenate([GOOD, np.zeros(4, np.uint8)]),
}


def _after_refusal(ctx):
    """The context still merges: the refusal left nothing behind."""
    _, out = run_merge(ctx, [stream([GOOD]), stream([record([(104, b"xx")])])])
    out.free()


@pytest.mark.parametrize("name", sorted(BAD_RECORDS))
def test_malformed_record_contributes_nothing(ctx, name):
    a = stream([GOOD, BAD_RECORDS[name], GOOD, EMPTY])
    b = stream([record([(102, b"BB")]), record([(7, b"kept")]), EMPTY, GOOD])
    (ro, data, *_), out = run_merge(ctx, [a, b], einval=True)
    # the page of the refused record holds the other stream's record alone
    assert data[int(ro[1]):int(ro[2])].tobytes() == record([(7, b"kept")]).tobytes()
    out.free()
    _after_refusal(ctx)


def test_decreasing_offsets_refused(ctx):
    ro = np.array([0, 2 * len(GOOD), len(GOOD), 3 * len(GOOD)], np.uint64)
    a = (ro, np.concatenate([GOOD, GOOD, GOOD]))
    (m_ro, *_), out = run_merge(ctx, [a, stream([GOOD, GOOD, GOOD])], einval=True)
    assert not m_ro.any()
    out.free()
    _after_refusal(ctx)


def test_unsorted_lists_refused(ctx):
    s = stream([GOOD, GOOD, GOOD])
    (m_ro, *_), out = run_merge(ctx, [s, s], [np.array([1, 5, 3], np.uint32), np.array([1, 3, 5], np.uint32)],
                                np.array([1, 3, 5], np.uint32), einval=True)
    assert not m_ro.any()
    out.free()
    _after_refusal(ctx)
    (m_ro, *_), out = run_merge(ctx, [s], [np.array([1, 3, 5], np.uint32)],
                                np.array([3, 3, 5], np.uint32), einval=True)
    out.free()
    _after_refusal(ctx)


# ---- 10. wire ------------------------------------------------------------------------------
def test_merged_stream_over_the_wire(ctx, joined):
    lists, streams, union = joined
    dev = [upload(ctx, s) for s in streams]
    res = ctx.merge(dev, lists)
    text = ctx.wire_encode(res.runs, res.out_ids)
    rng = np.random.default_rng(10)
    replica = rng.integers(0, 256, (300, 4096), dtype=np.uint8)
    want = replica.copy()
    for ids, (ro, data) in zip(lists, streams):
        oracle.apply(want, ro, data, ids=ids)
    with ga.Context(300) as follower:
        follower.upload("replica", replica)
        assert follower.wire_apply(text) == len(union)
        assert np.array_equal(follower.download("replica"), want)
    res.free()
    res.runs.free()
    for r in dev:
        r.free()


# ---- 11. gdsm_merge_raw --------------------------------------------------------------------
def test_merge_raw_on_caller_buffers(ctx):
    n, K = 257, 3
    twin, curs, streams = mm.writer_streams(n, K, 1, 100000, oracle)
    m_ro, m_data, m_conf, m_ov, m_cf = mm.merge(streams)
    need = int(m_ro[-1])
    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a)
        b = ctx.buffer(max(a.nbytes, 16)).upload(a)
        bufs.append(b)
        return b.ptr

    vp = C.c_void_p
    ro = (vp * K)(*[dev(s[0]) for s in streams])
    data = (vp * K)(*[dev(s[1]) for s in streams])
    caps = (C.c_uint64 * K)(*[len(s[1]) for s in streams])
    ns = (C.c_uint64 * K)(*[n] * K)
    out_ro, out_data = ctx.buffer(8 * (n + 1)), ctx.buffer(need + 64).upload(np.full(need + 64, GUARD, np.uint8))
    conf, stats, err = ctx.buffer(4 * n), ctx.buffer(16), ctx.buffer(4).upload(np.zeros(1, np.uint32))
    wsb = lib().gdsm_merge_workspace_bytes(n)
    ws = ctx.buffer(wsb)
    bufs += [out_ro, out_data, conf, stats, err, ws]
    rc = lib().gdsm_merge_raw(K, ro, data, caps, None, ns, None, n, out_ro.ptr, out_data.ptr, need,
                              conf.ptr, stats.ptr, err.ptr, ws.ptr, wsb, ctx.stream)
    assert rc == 0
    ctx.sync()
    assert np.array_equal(out_ro.download(np.uint64, n + 1), m_ro)
    raw = out_data.download(np.uint8, need + 64)
    assert np.array_equal(raw[:need], m_data) and (raw[need:] == GUARD).all()
    assert np.array_equal(conf.download(np.uint32, n), m_conf)
    assert stats.download(np.uint64, 2).tolist() == [m_ov, m_cf]
    assert err.download(np.uint32, 1)[0] == 0
    for b in bufs:
        b.free()
