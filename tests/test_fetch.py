"""CPU checks of the page fetch (docs/SPEC.md §9): the numpy model's own properties (block bounds,
the notice filter, what a fetch writes) and the immediate argument checks of gdsm_fetch and
gdsm_notices_fetch_list, which refuse before they touch a context or a GPU."""
import ctypes as C

import numpy as np

from tests import fetch_model as fm


def notice(page, before, after, ob=0, oa=0):
    return np.uint64(page | (before << 32) | (after << 34) | (ob << 40) | (oa << 48))


def test_block_bounds_cover_the_pages_once():
    for total, G in [(37, 1), (130, 2), (1025, 3), (777, 4), (1031, 8), (5, 8), (1, 8), (8, 8)]:
        per = fm.per_of(total, G)
        blocks = [fm.block_of(r, total, G) for r in range(G)]
        assert sum(n for _, n in blocks) == total
        at = 0
        for r, (base, n) in enumerate(blocks):
            assert base == at and 0 <= n <= per
            at += n
            if n:
                assert fm.home_of(base, total, G) == r and fm.home_of(base + n - 1, total, G) == r
        assert np.array_equal(fm.home_of(np.arange(total), total, G),
                              np.repeat(np.arange(G), [n for _, n in blocks]))


def test_blocks_are_empty_past_the_last_page():
    # 5 pages on 8 ranks: one page each on ranks 0-4, nothing on 5-7 (base clamps to the total)
    assert [fm.block_of(r, 5, 8) for r in range(8)] == \
        [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 0), (5, 0), (5, 0)]
    # 9 pages on 4 ranks: per = 3, so rank 3 holds nothing
    assert [fm.block_of(r, 9, 4) for r in range(4)] == [(0, 3), (3, 3), (6, 3), (9, 0)]


def test_fetch_list_filter_on_hand_made_notices():
    nt = np.array([notice(3, 0, 1),            # gained for reading
                   notice(5, 0, 2, 1, 0),      # gained for writing
                   notice(6, 1, 2, 2, 0),      # upgrade 1 -> 2: no contents needed
                   notice(9, 2, 0, 0, 3),      # lost
                   notice(11, 1, 0),           # invalidated
                   notice(12, 1, 1, 4, 5),     # owner changed only
                   notice(20, 0, 1),
                   notice(21, 2, 1, 0, 0)],    # downgrade
                  np.uint64)
    assert fm.fetch_list(nt, 1).tolist() == [3, 20]
    assert fm.fetch_list(nt, 2).tolist() == [5]
    assert fm.fetch_list(nt, 3).tolist() == [3, 5, 20]
    assert fm.fetch_list(nt[:0], 3).tolist() == []
    assert fm.fetch_list(nt, 3).dtype == np.uint32
    # page-sorted notices give a strictly ascending list
    assert (np.diff(fm.fetch_list(nt, 3).astype(np.int64)) > 0).all()


def test_model_fetch_writes_only_the_named_pages():
    rng = np.random.default_rng(1)
    G, Z = 3, 10
    per = fm.per_of(Z, G)
    rep = [rng.integers(0, 256, (Z, 4096), dtype=np.uint8) for _ in range(G)]
    arenas = [{"current": rng.integers(0, 256, (Z, 4096), dtype=np.uint8),
               "twin": rng.integers(0, 256, (Z, 4096), dtype=np.uint8)} for _ in range(G)]
    req = [[0, 4, 9], [], [5]]
    dst = [None, None, [2]]
    out = fm.fetch(rep, req, dst, arenas, Z)
    for name in ("current", "twin"):
        assert np.array_equal(out[0][name][0], rep[0][0])
        assert np.array_equal(out[0][name][4], rep[1][4 - per])
        assert np.array_equal(out[0][name][9], rep[2][9 - 2 * per])
        assert np.array_equal(out[2][name][2], rep[1][5 - per])
        assert np.array_equal(out[1][name], arenas[1][name])
        keep = np.setdiff1d(np.arange(Z), [0, 4, 9])
        assert np.array_equal(out[0][name][keep], arenas[0][name][keep])
    assert fm.valid_request([0, 4, 9], None, Z, Z)
    assert not fm.valid_request([0, 4, 4], None, Z, Z)
    assert not fm.valid_request([4, 0], None, Z, Z)
    assert not fm.valid_request([0, Z], None, Z + 1, Z)      # destination == n_pages
    assert not fm.valid_request([0, Z], [0, 1], Z, Z)        # page == total_pages
    assert not fm.valid_request([0, 1], [0, Z], Z, Z)


def test_fetch_argument_checks():
    """gdsm_fetch refuses a NULL context or communicator at once (-EINVAL), whatever else is
    passed, like the other entry points."""
    from gallocy_amd import _lib
    lib = _lib.load()
    ids = (C.c_uint32 * 2)(0, 1)
    p = C.cast(ids, C.c_void_p)
    fake = C.cast(ids, C.c_void_p)  # never dereferenced: the NULL argument is refused first
    assert lib.gdsm_fetch(None, None, None, None, 0, 1, 2, 0) == -22
    assert lib.gdsm_fetch(None, fake, p, None, 2, 8, 2, 0) == -22      # no context
    assert lib.gdsm_fetch(fake, None, p, None, 2, 8, 2, 0) == -22      # no communicator
    assert lib.gdsm_fetch(None, None, None, None, 2, 8, 2, 0) == -22   # n without pages
    assert lib.gdsm_fetch(None, None, p, p, 2, 0, 7, 0xFF) == -22


def test_notices_fetch_list_argument_checks():
    from gallocy_amd import _lib
    lib = _lib.load()
    k = C.c_uint64(77)
    buf = (C.c_uint64 * 2)(0, 0)
    p = C.cast(buf, C.c_void_p)
    assert lib.gdsm_notices_fetch_list(None, None, 0, 3, None, 0, C.byref(k)) == -22
    assert lib.gdsm_notices_fetch_list(None, p, 2, 1, p, 2, C.byref(k)) == -22
    assert lib.gdsm_notices_fetch_list(None, p, 2, 0, p, 2, None) == -22
    assert k.value == 77  # nothing was written
