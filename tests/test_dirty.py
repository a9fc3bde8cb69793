"""CPU checks of the dirty scan (docs/SPEC.md §12): the numpy model tests/dirty_model.py against
the oracle's diff (its dirty set is the set of non-empty records; its bound is at least the diff
stream of the dirty list, on the pages built to strain it), and the immediate argument checks of
gdsm_dirty_scan, gdsm_dirty_scan_raw and gdsm_dirty_scan_workspace_bytes, which refuse before they
touch a context or a GPU."""
import ctypes as C

import numpy as np

from oracle import oracle
from tests import dirty_model as dm


def test_dirty_set_equals_the_nonempty_records():
    rng = np.random.default_rng(120)
    Z = 96
    a = rng.integers(0, 256, (Z, 4096), dtype=np.uint8)
    b = a.copy()
    written = rng.choice(Z, Z // 3, replace=False)
    for p in written:
        k = int(rng.integers(1, 40))
        at = rng.integers(0, 4096, k)
        b[p, at] ^= rng.integers(1, 256, k).astype(np.uint8)
    lists = {"none": None,
             "permutation": rng.permutation(Z).astype(np.uint32),
             "repeats": rng.integers(0, Z, 3 * Z).astype(np.uint32)}
    for kind, ids in lists.items():
        ro, _ = oracle.diff_pages(a, b, ids)
        nonempty = np.flatnonzero(np.diff(ro.astype(np.int64)) > 0)
        pages, pos, count, bound = dm.dirty_scan(a, b, ids)
        assert np.array_equal(pos, nonempty), kind
        lst = np.arange(Z) if ids is None else ids
        assert np.array_equal(pages, lst[nonempty]), kind
        assert count == len(nonempty) and bound >= int(ro[-1]), kind
    pages, _, count, _ = dm.dirty_scan(a, b)
    assert sorted(pages.tolist()) == sorted(written.tolist()) and count == len(written)


def adversarial_pages():
    """(name, a page, b page) for each pattern of the bound's derivation."""
    rng = np.random.default_rng(121)
    base = rng.integers(0, 256, 4096, dtype=np.uint8)
    out = []
    q = base.copy()
    q[0::2] ^= 0xFF
    out.append(("alternating bytes, whole page", q))
    q = base.copy()
    q[1600:1616:2] ^= 0x01
    out.append(("one chunk of alternating bytes", q))
    q = base.copy()
    q[777] ^= 0x80
    out.append(("one byte", q))
    out.append(("fully changed", base ^ np.uint8(0xFF)))
    q = base.copy()
    for lo, hi in ((10, 40), (47, 49), (63, 65), (100, 1000), (4090, 4096)):
        q[lo:hi] ^= 0x55
    out.append(("runs that cross chunk borders", q))
    return [(name, base, q) for name, q in out]


def test_bound_covers_the_diff_of_the_adversarial_pages():
    cases = adversarial_pages()
    a = np.stack([c[1] for c in cases])
    b = np.stack([c[2] for c in cases])
    for k, (name, _, _) in enumerate(cases):
        pages, pos, count, bound = dm.dirty_scan(a, b, np.array([k], np.uint32))
        ro, _ = oracle.diff_pages(a, b, pages)
        assert count == 1 and pages.tolist() == [k], name
        assert bound >= int(ro[-1]) > 0, (name, bound, int(ro[-1]))
    # the cap is reached exactly by the largest record there is
    _, _, _, bound = dm.dirty_scan(a, b, np.array([0], np.uint32))
    assert bound == 10244 == int(oracle.diff_pages(a, b, np.array([0], np.uint32))[0][-1])
    # one chunk: 8 runs of 1 byte = 4 + 32 + 8 against 4 + 48
    assert dm.dirty_scan(a, b, np.array([1], np.uint32))[3] == 52
    assert dm.dirty_scan(a, b, np.array([2], np.uint32))[3] == 52
    # all of them in one list, and the same for the other direction
    for x, y in ((a, b), (b, a)):
        pages, _, count, bound = dm.dirty_scan(x, y)
        ro, _ = oracle.diff_pages(x, y, pages)
        assert count == len(cases) and bound >= int(ro[-1])


def test_model_skips_ids_out_of_range():
    rng = np.random.default_rng(122)
    a = rng.integers(0, 256, (8, 4096), dtype=np.uint8)
    b = a.copy()
    b[[2, 5], 9] ^= 1
    pages, pos, count, bound = dm.dirty_scan(a, b, np.array([5, 8, 2, 1000, 5], np.uint32))
    assert pages.tolist() == [5, 2, 5] and pos.tolist() == [0, 2, 4]
    assert count == 3 and bound == 3 * 52


def test_dirty_scan_argument_checks():
    from gallocy_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    fake = p  # never dereferenced: every call below is refused on its arguments
    # no context, whatever else
    assert lib.gdsm_dirty_scan(None, 0, 1, None, 0, None, None, 0, None) == -22
    assert lib.gdsm_dirty_scan(None, 0, 1, None, 4, p, p, 4, p) == -22
    assert lib.gdsm_dirty_scan(None, 1, 1, p, 4, p, None, 4, p) == -22
    # the raw form: a NULL arena
    ws = lib.gdsm_dirty_scan_workspace_bytes(4)
    assert lib.gdsm_dirty_scan_raw(None, fake, None, 4, p, None, 4, p, p, ws, None) == -22
    assert lib.gdsm_dirty_scan_raw(fake, None, None, 4, p, None, 4, p, p, ws, None) == -22
    # a capacity with nowhere to write, a list longer than 2^32
    assert lib.gdsm_dirty_scan_raw(fake, fake, None, 4, None, None, 4, p, p, ws, None) == -22
    big = (1 << 32) + 1
    assert lib.gdsm_dirty_scan_raw(fake, fake, None, big, p, None, 4, p, p,
                                   lib.gdsm_dirty_scan_workspace_bytes(big), None) == -22
    # no workspace, one that is too small, one that is not 8-byte aligned
    assert lib.gdsm_dirty_scan_raw(fake, fake, None, 4, p, None, 4, p, None, ws, None) == -22
    assert lib.gdsm_dirty_scan_raw(fake, fake, None, 4, p, None, 4, p, p, ws - 1, None) == -22
    assert lib.gdsm_dirty_scan_raw(fake, fake, None, 4, p, None, 4, p, p.value + 4, ws,
                                   None) == -22
    assert list(buf) == [0] * 8


def test_workspace_is_at_most_a_byte_per_entry_plus_a_constant():
    from gallocy_amd import _lib
    lib = _lib.load()
    for n in (0, 1, 63, 64, 65, 70000, 1 << 20, 1 << 32):
        w = lib.gdsm_dirty_scan_workspace_bytes(n)
        assert 0 < w <= n + 128, n
    sizes = [lib.gdsm_dirty_scan_workspace_bytes(n) for n in (1, 64, 65, 4096, 4097)]
    assert sizes == sorted(sizes)
