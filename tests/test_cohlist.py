"""CPU checks of the page table by page list (docs/SPEC.md §15) on the numpy model
tests/cohlist_model.py over valid tables (oracle.coh_init folded with oracle.coherence): the
whole-array forms against the per-entry loop on random lists with repeats and ids out of range, the
properties the SPEC states of clean (idempotent, only bit 18 changes, the invariants, a fold input,
"owns dirty" empties and nothing is orphaned), lookup as the producer of gdsm_runs_split's masks,
and the C ABI: both symbols are exported and refuse a NULL context before they touch a GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from tests import cohlist_model as cm
from tests import split_model
from tests import sweep_model as sm

DIRTY = 1 << 18
ZERO = dict.fromkeys(cm.KEYS, 0)


def word(copyset, owner, state, dirty=0):
    return copyset | (owner << 8) | (state << 16) | (dirty << 18)


def folded_table(n_pages, n_nodes, seed, write_pct=30):
    st, fl = oracle.coh_init(n_pages, n_nodes)
    counts = np.random.default_rng(seed).integers(0, 10, n_pages).astype(np.uint64)
    ev = oracle.gen_events(counts, seed=seed + 1, n_nodes=n_nodes, write_pct=write_pct)
    rc, _ = oracle.coherence(st, fl, ev, n_nodes=n_nodes)
    assert rc == 0
    return st, fl


def valid(st):
    c, o, s = st & 0xFF, (st >> 8) & 0xFF, (st >> 16) & 3
    live = s != 0
    return bool((((c >> o) & 1) == 1)[live].all() and (c == 1 << o)[live & (s == 2)].all())


def random_list(rng, Z, n, base, repeats=True, out_of_range=True):
    ids = base + (rng.integers(0, Z, n) if repeats else rng.permutation(Z)[:n])
    ids = ids.astype(np.uint32)
    if out_of_range and n >= 4:
        ids[rng.integers(0, n)] = base + Z
        ids[rng.integers(0, n)] = 0xFFFFFFFF
        if base:
            ids[rng.integers(0, n)] = base - 1
    return ids


@pytest.mark.parametrize("n_nodes,seed", [(8, 1), (3, 2), (2, 3)])
def test_whole_array_forms_equal_the_loop(n_nodes, seed):
    Z = 1500
    st, fl = folded_table(Z, n_nodes, seed)
    st[7] = 0
    st[8] = 0x1FF | DIRTY                                       # INVALID with stray bits
    st[9] = word(3, 1, sm.SHARED, 1) | (0x1234 << 19)
    rng = np.random.default_rng(seed + 50)
    for node in range(n_nodes):
        for base, n in ((0, 2000), (777, 1), (1 << 20, 600)):
            ids = random_list(rng, Z, n, base)
            a, b = cm.clean(st, node, ids, base=base), cm.clean_vec(st, node, ids, base=base)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
            assert a[3] == b[3] and sum(a[1].values()) == n
            for shift, mask in ((0, 0xFF & ~(1 << node)), (8, 0xFF), (0, 0xFFFFFFFF)):
                x = cm.lookup(st, fl, ids, base=base, shift=shift, mask=mask)
                y = cm.lookup_vec(st, fl, ids, base=base, shift=shift, mask=mask)
                assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
        a, b = cm.clean(st, node, None, 1000), cm.clean_vec(st, node, None, 1000)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
        assert a[1]["cleaned"] > 0 and not a[3]
        assert np.array_equal(a[0][1000:], st[1000:])


def test_repeats_clean_once_and_the_first_occurrence_does():
    st = np.array([word(1, 0, 2, 1), word(3, 1, 1, 1), word(1, 0, 2, 0), 0], np.uint32)
    ids = np.array([0, 1, 0, 2, 3, 0, 9], np.uint32)
    new, stats, status, bad = cm.clean(st, 0, ids)
    assert status.tolist() == [0, 2, 1, 1, 3, 1, 4] and bad
    assert stats == {"cleaned": 1, "already": 3, "stale": 1, "skipped": 2}
    assert new.tolist() == [word(1, 0, 2, 0), st[1], st[2], 0]
    assert cm.status_multisets(ids, status)[0] == [0, 1, 1]


@pytest.mark.parametrize("n_nodes", [2, 8])
def test_clean_properties(n_nodes):
    Z = 800
    st, fl = folded_table(Z, n_nodes, seed=20 + n_nodes)
    st[5] |= 0x155 << 19
    rng = np.random.default_rng(30)
    for d in range(n_nodes):
        ids = random_list(rng, Z, 500, 0, out_of_range=False)
        new, stats, status, bad = cm.clean(st, d, ids)
        assert not bad and stats["cleaned"] > 0
        assert ((new ^ st) & ~np.uint32(DIRTY)).max() == 0           # only bit 18 changes
        changed = np.flatnonzero(new != st)
        assert len(changed) == stats["cleaned"] and set(changed) <= set(ids.tolist())
        assert (((st[changed] >> 8) & 0xFF) == d).all()
        assert valid(new) and new[5] >> 19 == st[5] >> 19
        # idempotent
        again, stats2, status2, _ = cm.clean(new, d, ids)
        assert np.array_equal(again, new) and stats2["cleaned"] == 0
        assert stats2["already"] == stats["cleaned"] + stats["already"]
        assert np.array_equal(status2 == cm.STALE, status == cm.STALE)
        # a fold input, and a later write sets the bit again
        f2 = fl.copy()
        ev = oracle.gen_events(np.full(Z, 2, np.uint64), seed=31, n_nodes=n_nodes, write_pct=100)
        rc, _ = oracle.coherence(again, f2, ev, n_nodes=n_nodes)
        assert rc == 0 and valid(again) and ((again >> 18) & 1).all()


@pytest.mark.parametrize("d", range(8))
def test_owns_dirty_empties_and_nothing_is_orphaned(d):
    Z, base = 1000, 4096
    st, _ = folded_table(Z, 8, seed=40)
    mask, value = 0xFF00 | DIRTY, d << 8 | DIRTY
    lst, count = sm.select(st, mask, value, base)
    heir = (d + 1) % 8
    assert count > 0 and sm.retire(st, d, heir)[1]["orphaned"] > 0
    new, stats, status, bad = cm.clean(st, d, lst, base=base)
    assert stats == {**ZERO, "cleaned": count} and not status.any() and not bad
    assert sm.select(new, mask, value, base)[1] == 0
    after = sm.retire(new, d, heir)[1]
    assert after["orphaned"] == 0 and after["moved"] == sm.retire(st, d, heir)[1]["moved"]
    # the other nodes' dirty pages are as they were
    for e in range(8):
        if e != d:
            assert np.array_equal(sm.select(new, mask, e << 8 | DIRTY)[0],
                                  sm.select(st, mask, e << 8 | DIRTY)[0])


def test_lookup_masks_feed_the_split_model():
    """A home (node 2) forwards writer 5's stream: dest = copyset without writer and home."""
    Z, G, writer, home = 400, 8, 5, 2
    st, fl = folded_table(Z, G, seed=60)
    rng = np.random.default_rng(61)
    ids = np.sort(rng.choice(Z, 150, replace=False)).astype(np.uint32) + 1000
    sizes = rng.choice((0, 12, 16, 40), len(ids))
    ro = np.zeros(len(ids) + 1, np.uint64)
    ro[1:] = np.cumsum(sizes)
    data = rng.integers(0, 256, int(ro[-1]), dtype=np.uint8)
    sel = 0xFF & ~(1 << writer) & ~(1 << home)
    dest, fo, bad = cm.lookup(st, fl, ids, base=1000, shift=0, mask=sel)
    assert not bad and np.array_equal(fo, fl[ids - 1000])
    w = st[ids - 1000]
    keep = np.uint32(0xFF ^ (1 << writer) ^ (1 << home))
    straight = np.where((w >> 16) & 3 != 0, w & keep, 0)
    assert np.array_equal(dest, straight.astype(np.uint32)) and dest.any()
    a = split_model.split(ro, data, ids, dest, 0, G)
    b = split_model.split(ro, data, ids, straight.astype(np.uint32), 0, G)
    assert a[0] == b[0] == 0 and np.array_equal(a[2], b[2])
    assert a[2][writer, 0] == a[2][home, 0] == 0 and a[2][:, 0].sum() > 0
    for d in range(G):
        assert all(np.array_equal(x, y) for x, y in zip(a[1][d], b[1][d]))
        holds = (((w >> d) & 1) == 1) & (((w >> 16) & 3) != 0) & (d not in (writer, home))
        assert np.array_equal(a[1][d][2], ids[holds])
    owners = cm.lookup(st, fl, ids, base=1000, shift=8, mask=0xFF)[0]
    assert np.array_equal(owners, (w >> 8) & 0xFF)
    assert np.array_equal(cm.lookup(st, fl, ids, base=1000)[0], w)


def test_symbols_are_exported_and_refuse_without_a_context():
    from gallocy_amd import _lib
    lib = _lib.load()
    assert "gdsm_coh_clean" in _lib.SIGNATURES and "gdsm_coh_lookup" in _lib.SIGNATURES
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.gdsm_coh_clean(None, 0, None, 0, 0, None, None, 0) == -22
    assert lib.gdsm_coh_clean(None, 0, p, 4, 0, p, p, 0) == -22
    assert lib.gdsm_coh_lookup(None, None, 0, 0, 0, 0, None, None) == -22
    assert lib.gdsm_coh_lookup(None, p, 4, 0, 0, 0xFF, p, p) == -22
    assert list(buf) == [0] * 8
