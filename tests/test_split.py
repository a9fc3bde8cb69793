"""CPU checks of the stream split (docs/SPEC.md §13): the numpy model tests/split_model.py against
hand-written cases and against the oracle (applying the outputs equals applying the input
restricted to each destination's pages), the concatenation property of the home form, and the
immediate argument checks of gdsm_runs_split, gdsm_runs_split_raw and
gdsm_runs_split_workspace_bytes, which refuse before they touch a context or a GPU."""
import ctypes as C

import numpy as np

from oracle import oracle
from tests import split_model as sm


def stream(sizes, seed=0):
    """A stream of opaque records of the given sizes (multiples of 4), bytes random."""
    ro = np.zeros(len(sizes) + 1, np.uint64)
    ro[1:] = np.cumsum(np.asarray(sizes, np.uint64))
    data = np.random.default_rng(seed).integers(0, 256, int(ro[-1]), dtype=np.uint8)
    return ro, data


def test_mask_form_by_hand():
    ro, data = stream([4, 0, 8, 12])
    dest = np.array([0b01, 0b11, 0b10, 0b11], np.uint32)
    ids = np.array([7, 9, 11, 30], np.uint32)
    err, outs, counts = sm.split(ro, data, ids, dest, 0, 2)
    assert err == 0
    assert outs[0][0].tolist() == [0, 4, 4, 16] and outs[0][2].tolist() == [7, 9, 30]
    assert outs[0][1].tobytes() == data[0:4].tobytes() + data[12:24].tobytes()
    assert outs[1][0].tolist() == [0, 0, 8, 20] and outs[1][2].tolist() == [9, 11, 30]
    assert outs[1][1].tobytes() == data[4:24].tobytes()
    assert counts.tolist() == [[3, 16], [3, 20]]
    # the flag drops the empty record everywhere
    err, outs, counts = sm.split(ro, data, ids, dest, 0, 2, sm.DROP_EMPTY)
    assert outs[0][0].tolist() == [0, 4, 16] and outs[0][2].tolist() == [7, 30]
    assert outs[1][0].tolist() == [0, 8, 20] and outs[1][2].tolist() == [11, 30]
    assert counts.tolist() == [[2, 16], [2, 20]]
    # mask 0 everywhere; ids NULL = the record's index
    err, outs, counts = sm.split(ro, data, None, np.zeros(4, np.uint32), 0, 3)
    assert err == 0 and counts.tolist() == [[0, 0]] * 3
    assert all(o[0].tolist() == [0] and len(o[1]) == 0 for o in outs)
    err, outs, _ = sm.split(ro, data, None, np.full(4, 4, np.uint32), 0, 3)
    assert outs[2][2].tolist() == [0, 1, 2, 3] and outs[2][1].tobytes() == data.tobytes()


def test_home_form_by_hand():
    ro, data = stream([8, 4, 0, 16, 4])
    ids = np.array([12, 3, 25, 10, 29], np.uint32)  # unsorted; per 10: homes 1, 0, 2, 1, 2
    err, outs, counts = sm.split(ro, data, ids, None, 10, 3)
    assert err == 0
    assert outs[0][2].tolist() == [3] and outs[1][2].tolist() == [2, 0] and outs[2][2].tolist() == [5, 9]
    assert outs[1][0].tolist() == [0, 8, 24]
    assert outs[1][1].tobytes() == data[0:8].tobytes() + data[12:28].tobytes()
    assert outs[2][0].tolist() == [0, 0, 4]
    assert counts.tolist() == [[1, 4], [2, 24], [2, 4]]
    # ids NULL: the home of record i is i // per
    err, outs, counts = sm.split(ro, data, None, None, 2, 3)
    assert [o[2].tolist() for o in outs] == [[0, 1], [0, 1], [0]]
    # an uneven last block and a home out of range
    assert sm.split(ro, data, None, None, 2, 2)[0] == sm.ERR_IDS
    err, outs, counts = sm.split(ro, data, ids, None, 10, 2)
    assert err == sm.ERR_IDS and counts.tolist() == [[0, 0], [0, 0]]
    assert all(o[0].tolist() == [0] for o in outs)


def test_refusals_and_capacity_of_the_model():
    ro, data = stream([4, 8, 4])
    one = np.ones(3, np.uint32)
    for bad in ([4, 4, 12, 16], [0, 4, 2, 16], [0, 8, 4, 16], [0, 4, 12, 20]):
        assert sm.split(np.array(bad, np.uint64), data, None, one, 0, 1)[0] == sm.ERR_STREAM, bad
    assert sm.split(ro, data, None, np.array([1, 2, 1], np.uint32), 0, 1)[0] == sm.ERR_IDS
    assert sm.split(np.array([4, 4, 12, 16], np.uint64), data, None,
                    np.array([1, 2, 1], np.uint32), 0, 1)[0] == sm.ERR_IDS | sm.ERR_STREAM
    err, outs, counts = sm.split(ro, data, None, one, 0, 1)
    assert sm.verdict(err, counts, [16], [3]) == 0
    assert sm.verdict(err, counts, [16], [2]) == sm.ENOSPC
    assert sm.verdict(err, counts, [12], [3]) == sm.ENOSPC
    assert sm.verdict(sm.ERR_IDS, counts, [16], [3]) == sm.EINVAL
    o, buf, ids = sm.written(outs[0], 10, 2)
    assert o.tolist() == [0, 4, 12] and len(buf) == 8 and ids.tolist() == [0, 1]
    # the immediate refusals
    assert sm.immediate(3, 1, True, 0, 0) == 0 and sm.immediate(3, 8, False, 5, 1) == 0
    assert sm.immediate(3, 0, True, 0, 0) == sm.EINVAL and sm.immediate(3, 9, True, 0, 0) == sm.EINVAL
    assert sm.immediate(3, 2, True, 5, 0) == sm.EINVAL and sm.immediate(3, 2, False, 0, 0) == sm.EINVAL
    assert sm.immediate(3, 2, True, 0, 2) == sm.EINVAL
    assert sm.immediate((1 << 32) + 1, 2, True, 0, 0) == sm.EINVAL
    assert sm.immediate(3, 2, True, 0, 0, [(10, 20), (30, 20)], (1, 2)) == sm.EINVAL
    assert sm.immediate(3, 2, True, 0, 0, [(10, 20), (1, 40)], (1, 2)) == sm.EINVAL
    assert sm.immediate(3, 2, True, 0, 0, [(10, 20), (30, 40)], (1, 2)) == 0


def real_stream(seed, Z=64, frac=0.6):
    rng = np.random.default_rng(seed)
    twin = rng.integers(0, 256, (Z, 4096), dtype=np.uint8)
    cur = twin.copy()
    for p in rng.choice(Z, int(Z * frac), replace=False):
        k = int(rng.integers(1, 60))
        cur[p, rng.integers(0, 4096, k)] ^= rng.integers(1, 256, k).astype(np.uint8)
    ids = np.sort(rng.choice(Z, Z * 3 // 4, replace=False)).astype(np.uint32)
    ro, data = oracle.diff_pages(twin, cur, ids)
    return twin, cur, ids, ro, data


def test_applying_the_outputs_equals_applying_the_restricted_input():
    twin, cur, ids, ro, data = real_stream(140)
    rng = np.random.default_rng(141)
    G = 4
    dest = rng.integers(0, 1 << G, len(ids)).astype(np.uint32)
    for flags in (0, sm.DROP_EMPTY):
        err, outs, counts = sm.split(ro, data, ids, dest, 0, G, flags)
        assert err == 0
        for d in range(G):
            sel = np.flatnonzero((dest >> d) & 1)
            want = twin.copy()
            sub_ro, sub_data = oracle.diff_pages(twin, cur, ids[sel])
            assert oracle.apply(want, sub_ro, sub_data, ids[sel]) == 0
            got = twin.copy()
            o, buf, pages = outs[d]
            assert oracle.apply(got, o, buf, pages) == 0
            assert np.array_equal(got, want), (flags, d)
            assert np.array_equal(want[ids[sel]], cur[ids[sel]])
            if not flags:
                assert np.array_equal(o, sub_ro) and np.array_equal(buf, sub_data)
            assert np.all(np.diff(pages.astype(np.int64)) > 0)
    # home form: each home's output applied at the home's own index
    per = 24  # 64 pages over 3 homes: 24, 24, 16
    err, outs, counts = sm.split(ro, data, ids, None, per, 3)
    assert err == 0 and int(counts[:, 0].sum()) == len(ids)
    for d in range(3):
        block = slice(d * per, min(64, (d + 1) * per))
        got = twin[block].copy()
        assert oracle.apply(got, *outs[d][:2], outs[d][2]) == 0
        want = twin[block].copy()
        mine = ids[(ids >= block.start) & (ids < block.stop)]
        want[mine - block.start] = cur[mine]
        assert np.array_equal(got, want), d


def test_home_form_concatenates_to_the_input():
    _, _, ids, ro, data = real_stream(142)
    for per, G in ((64, 1), (32, 2), (24, 3), (8, 8)):
        err, outs, counts = sm.split(ro, data, ids, None, per, G)
        assert err == 0
        assert np.concatenate([o[1] for o in outs]).tobytes() == data[:int(ro[-1])].tobytes()
        assert int(counts[:, 1].sum()) == int(ro[-1])
        back = np.concatenate([o[2].astype(np.int64) + d * per for d, o in enumerate(outs)])
        assert np.array_equal(back, ids)


def test_runs_split_argument_checks():
    from gallocy_amd import _lib
    from gallocy_amd._lib import GdsmRuns
    lib = _lib.load()
    buf = (C.c_uint64 * 64)()
    base = C.cast(buf, C.c_void_p).value
    p = lambda k: C.c_void_p(base + 8 * k)  # distinct fake device pointers, never dereferenced
    fake_ctx = p(0)  # refused on the arguments before the context is looked at

    def runs(k, n=4):
        return GdsmRuns(n=n, rec_off=base + 64 * k, data=base + 64 * k + 32, cap=64, n_cap=4)

    def ctx_call(ctx, inp, dest, per, G, outs, flags=0, ids=None):
        arr = (GdsmRuns * 8)(*outs) if outs is not None else None
        return lib.gdsm_runs_split(ctx, C.byref(inp) if inp is not None else None, ids, dest, per,
                                   G, arr, None, None, flags)

    inp, outs = runs(1), [runs(2), runs(3)]
    assert ctx_call(None, inp, p(1), 0, 2, outs) == -22
    assert ctx_call(fake_ctx, None, p(1), 0, 2, outs) == -22
    assert ctx_call(fake_ctx, inp, p(1), 0, 2, None) == -22
    assert ctx_call(fake_ctx, inp, p(1), 0, 0, outs) == -22
    assert ctx_call(fake_ctx, inp, p(1), 0, 9, outs) == -22
    assert ctx_call(fake_ctx, inp, p(1), 5, 2, outs) == -22      # both forms
    assert ctx_call(fake_ctx, inp, None, 0, 2, outs) == -22      # neither
    assert ctx_call(fake_ctx, inp, p(1), 0, 2, outs, flags=2) == -22
    assert ctx_call(fake_ctx, runs(1, (1 << 32) + 1), p(1), 0, 2, outs) == -22
    assert ctx_call(fake_ctx, inp, p(1), 0, 2, [runs(2), runs(2)]) == -22  # two outputs, one buffer
    assert ctx_call(fake_ctx, inp, p(1), 0, 2, [runs(2), runs(1)]) == -22  # an output is the input
    shared = runs(3)
    shared.data = inp.data
    assert ctx_call(fake_ctx, inp, None, 7, 2, [runs(2), shared]) == -22
    odd = runs(3)
    odd.data = odd.data + 2
    assert ctx_call(fake_ctx, inp, p(1), 0, 2, [runs(2), odd]) == -22  # a data pointer at 2 mod 4

    def raw_call(n=4, G=2, dest=p(1), per=0, flags=0, ro=None, data=None, counts=p(2), ws=p(8),
                 ws_bytes=None, in_ro=p(40), in_data=p(44)):
        ro = ro or [base + 128, base + 192]
        data = data or [base + 160, base + 224]
        ro_a = (C.c_void_p * 8)(*ro)
        da_a = (C.c_void_p * 8)(*data)
        caps = (C.c_uint64 * 8)(*([32] * 8))
        ncaps = (C.c_uint64 * 8)(*([4] * 8))
        if ws_bytes is None:
            ws_bytes = lib.gdsm_runs_split_workspace_bytes(n, G)
        return lib.gdsm_runs_split_raw(in_ro, in_data, 32, None, dest, per, n, G, ro_a, da_a, caps,
                                       ncaps, None, counts, None, flags, ws, ws_bytes, None)

    assert raw_call(G=0) == -22 and raw_call(G=9) == -22
    assert raw_call(per=3) == -22 and raw_call(dest=None) == -22
    assert raw_call(flags=4) == -22
    assert raw_call(n=(1 << 32) + 1) == -22
    assert raw_call(in_ro=None) == -22
    assert raw_call(ro=[base + 128, base + 128]) == -22
    assert raw_call(data=[base + 160, base + 160]) == -22
    assert raw_call(ro=[base + 320, base + 192]) == -22          # in_ro = p(40) = base + 320
    assert raw_call(data=[base + 352, base + 224]) == -22        # the input's data = p(44)
    assert raw_call(ro=[None, base + 192]) == -22
    # data pointers that are not 4-byte aligned: an output's, the input's
    assert raw_call(data=[base + 162, base + 224]) == -22
    assert raw_call(in_data=C.c_void_p(base + 353)) == -22
    assert raw_call(counts=None) == -22
    # no workspace, one that is too small, one that is not 8-byte aligned
    assert raw_call(ws=None) == -22
    assert raw_call(ws_bytes=lib.gdsm_runs_split_workspace_bytes(4, 2) - 1) == -22
    assert raw_call(ws=C.c_void_p(base + 68)) == -22
    assert list(buf) == [0] * 64


def test_workspace_is_monotone_in_n_and_G():
    from gallocy_amd import _lib
    lib = _lib.load()
    ns = (0, 1, 255, 256, 257, 70000, 1 << 20, 1 << 32)
    for G in range(1, 9):
        sizes = [lib.gdsm_runs_split_workspace_bytes(n, G) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] > 0, G
    for n in ns:
        sizes = [lib.gdsm_runs_split_workspace_bytes(n, G) for G in range(1, 9)]
        assert sizes == sorted(sizes), n
    # no n x G table of positions: 16 B per 256-record tile and destination
    assert lib.gdsm_runs_split_workspace_bytes(1 << 20, 8) <= (1 << 20) // 2 + 4096
