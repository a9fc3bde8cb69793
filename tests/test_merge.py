"""CPU checks of gdsm_merge's semantics (docs/SPEC.md §8) on the numpy model tests/merge_model.py,
against the C oracle's diff and apply, and of the entry points' argument checks (no device)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from tests import merge_model as mm

# the overlap recipe of merge_model.writer_streams: (pages, K, mode, ppm)
WORKLOADS = [(64, 3, 0, 10000), (64, 3, 1, 100000), (64, 3, 0, 400000)]


@pytest.fixture(scope="module", params=WORKLOADS, ids=lambda w: f"n{w[0]}k{w[1]}m{w[2]}p{w[3]}")
def work(request):
    n, K, mode, ppm = request.param
    twin, curs, streams = mm.writer_streams(n, K, mode, ppm, oracle)
    return n, twin, curs, streams, mm.merge(streams)


def _apply_all(target, streams):
    for ro, data in streams:
        oracle.apply(target, ro, data)
    return target


def test_model_apply_equivalence(work):
    n, twin, curs, streams, (ro, data, conflicts, ov, cf) = work
    rng = np.random.default_rng(5)
    target = rng.integers(0, 256, (n, 4096), dtype=np.uint8)
    want = _apply_all(target.copy(), streams)
    got = target.copy()
    oracle.apply(got, ro, data)
    assert np.array_equal(got, want)
    # the counts, restated on the pages: a byte two writers changed, and changed differently
    wrote = np.stack([c != twin for c in curs])
    overlap = wrote.sum(0) >= 2
    assert ov == int(overlap.sum()) and ov > 0
    vals = np.stack(curs)
    lo = np.where(wrote, vals, 255).min(0)
    hi = np.where(wrote, vals, 0).max(0)
    differ = overlap & (lo != hi)
    assert cf == int(differ.sum())
    assert np.array_equal(conflicts, differ.sum(1))


def test_model_is_associative(work):
    n, twin, curs, streams, (ro, data, _, _, _) = work
    ab = mm.merge(streams[:2])
    left = mm.merge([(ab[0], ab[1]), streams[2]])
    assert np.array_equal(left[0], ro) and np.array_equal(left[1], data)
    bc = mm.merge(streams[1:])
    right = mm.merge([streams[0], (bc[0], bc[1])])
    assert np.array_equal(right[0], ro) and np.array_equal(right[1], data)


def test_model_k1_identity(work):
    n, twin, curs, streams, _ = work
    for s in streams:
        ro, data, conflicts, ov, cf = mm.merge([s])
        assert np.array_equal(ro, s[0]) and np.array_equal(data, s[1])
        assert ov == 0 and cf == 0 and not conflicts.any()


def test_model_issue_figures():
    """The three workloads the feature was sized on (K = 3): merged bytes, overlapped and
    conflicting bytes, and the longest record of the dense one."""
    want = {(257, 0, 10000): (48232, 291, 291), (257, 1, 100000): (306092, 30046, 29940),
            (64, 0, 400000): (230252, 92078, 91826)}
    for (n, mode, ppm), (size, ov, cf) in want.items():
        _, _, streams = mm.writer_streams(n, 3, mode, ppm, oracle)
        ro, data, _, o, c = mm.merge(streams)
        assert (int(ro[-1]), o, c) == (size, ov, cf), (n, mode, ppm)
        if ppm == 400000:
            nruns = [int(data[int(a):int(a) + 4].view("<u4")[0]) for a, b in zip(ro[:-1], ro[1:])
                     if b > a]
            assert max(nruns) == 116


def test_model_id_join_and_selection():
    rng = np.random.default_rng(9)
    twin = rng.integers(0, 256, (40, 4096), dtype=np.uint8)
    lists, streams = [], []
    for k in range(3):
        ids = np.sort(rng.choice(40, 12, replace=False)).astype(np.uint32)
        cur = twin.copy()
        for p in ids:
            o = int(rng.integers(0, 4000))
            cur[p, o:o + 50] ^= np.uint8(k + 1)
        lists.append(ids)
        streams.append(oracle.diff_pages(twin, cur, ids=ids))
    union = np.unique(np.concatenate(lists))
    ro, data, _, _, _ = mm.merge(streams, lists, union)
    want = twin.copy()
    for ids, (r, d) in zip(lists, streams):
        oracle.apply(want, r, d, ids=ids)
    got = twin.copy()
    oracle.apply(got, ro, data, ids=union)
    assert np.array_equal(got, want)
    sub = union[::2]
    ro, data, _, _, _ = mm.merge(streams, lists, sub)
    got = twin.copy()
    oracle.apply(got, ro, data, ids=sub)
    sel = np.zeros(40, bool)
    sel[sub] = True
    assert np.array_equal(got[sel], want[sel]) and np.array_equal(got[~sel], twin[~sel])


def test_model_refuses_what_apply_refuses():
    rec = lambda hdrs, pay: np.frombuffer(  # noqa: E731
        np.array([len(hdrs)] + hdrs, "<u4").tobytes() + pay, np.uint8)
    good = rec([0 | (4 << 16)], b"abcd")
    assert mm.parse_record(good)[0][:4].all()
    for bad in (np.zeros(8, np.uint8),                            # nruns = 0, size 8
                rec([4090 | (8 << 16)], b"x" * 8),                # past the page
                rec([0 | (8 << 16), 4 | (4 << 16)], b"x" * 12),   # overlapping
                np.concatenate([good, np.zeros(4, np.uint8)])):   # 4 bytes longer
        assert mm.parse_record(bad)[0] == "bad"
        ro = np.array([0, len(bad), len(bad) + len(good)], np.uint64)
        out = mm.merge_ex([(ro, np.concatenate([bad, good]))])
        assert out[5] and out[0].tolist() == [0, 0, len(good)] and np.array_equal(out[1], good)
    # offsets that decrease, or an unsorted list: the output is empty
    ro = np.array([0, 8, 4], np.uint64)
    assert mm.merge_ex([(ro, np.zeros(8, np.uint8))])[5]
    ro = np.array([0, len(good), 2 * len(good)], np.uint64)
    out = mm.merge_ex([(ro, np.concatenate([good, good]))], [np.array([5, 3])], np.array([3, 5]))
    assert out[5] and not out[0].any() and len(out[1]) == 0


def test_merge_argument_checks():
    """Everything gdsm_merge and gdsm_merge_raw refuse at once (-EINVAL) is refused before any
    device is touched."""
    from gallocy_amd import _lib
    lib = _lib.load()
    R = _lib.GdsmRuns
    runs = (R * 2)()
    out = R()
    assert lib.gdsm_merge(None, 1, runs, None, None, 0, C.byref(out), None, None) == -22
    assert lib.gdsm_merge_workspace_bytes(1) >= 256 + 2 * 256 + 16
    sizes = [lib.gdsm_merge_workspace_bytes(n) for n in (0, 1, 4096, 4097, 1 << 20)]
    assert sizes == sorted(sizes)

    # the raw form takes every rule without a context: fake (never dereferenced) device pointers
    def raw(K=2, ro=(0x1000, 0x2000), data=(0x3000, 0x4000), caps=(64, 64), ids=None, n=(4, 4),
            out_ids=None, n_out=4, out_ro=0x5000, out_data=0x6000, out_cap=64, ws=0x7000,
            ws_bytes=1 << 20):
        vp = C.c_void_p
        a = lambda xs: (vp * 8)(*xs)  # noqa: E731
        u = lambda xs: (C.c_uint64 * 8)(*xs)  # noqa: E731
        return lib.gdsm_merge_raw(K, a(ro), a(data), u(caps), None if ids is None else a(ids),
                                  u(n), out_ids, n_out, out_ro, out_data, out_cap, None, None,
                                  None, ws, ws_bytes, None)
    assert raw(K=0) == -22 and raw(K=9) == -22
    assert raw(ro=(0x1000, None)) == -22                       # a stream without offsets
    assert raw(n=(4, 5)) == -22                                # no list, and not n_out records
    assert raw(ids=(0x8000, None), out_ids=None) == -22        # a list, but the identity out list
    assert raw(ids=(0x8000, None), out_ids=0x9000, n=(9, 5)) == -22
    assert raw(out_ro=0x2000) == -22 and raw(out_data=0x4000) == -22   # out shares an input
    assert raw(out_ro=None) == -22 and raw(out_data=None) == -22
    assert raw(ws=None) == -22 and raw(ws_bytes=64) == -22
    assert raw(n_out=1 << 32, n=(1 << 32, 1 << 32), ws_bytes=1 << 40) == -22
