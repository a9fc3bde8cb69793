"""CPU checks of the page-table sweeps (docs/SPEC.md §14): the properties the SPEC states of
retire, on the numpy model tests/sweep_model.py over valid tables (oracle.coh_init folded with
oracle.coherence over oracle.gen_events) with a few hand-made words added; select against a numpy
one-liner; and the C ABI: both symbols are exported, and both refuse a NULL context before they
touch a GPU (a machine without one cannot make a context: gdsm_init gives -ENODEV there)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from tests import sweep_model as sm

EXCL, SHRD = sm.EXCLUSIVE << 16, sm.SHARED << 16
DIRTY = 1 << 18


def word(copyset, owner, state, dirty=0):
    return copyset | (owner << 8) | (state << 16) | (dirty << 18)


def folded_table(n_pages, n_nodes, seed, write_pct=25):
    """A valid table: the initial one after a random batch."""
    st, fl = oracle.coh_init(n_pages, n_nodes)
    counts = np.random.default_rng(seed).integers(0, 12, n_pages).astype(np.uint64)
    ev = oracle.gen_events(counts, seed=seed + 1, n_nodes=n_nodes, write_pct=write_pct)
    rc, _ = oracle.coherence(st, fl, ev, n_nodes=n_nodes)
    assert rc == 0
    return st, fl


def valid(st):
    """owner in copyset, and EXCLUSIVE => copyset == {owner}, on every page that is not INVALID."""
    for w in st.tolist():
        c, o, s, _ = sm.fields(w)
        if s == sm.INVALID:
            continue
        if not (c >> o) & 1:
            return False
        if s == sm.EXCLUSIVE and c != 1 << o:
            return False
    return True


CASES = [(n_nodes, x, heir, per_kind) for n_nodes in (2, 5, 8) for x in range(n_nodes)
         for heir in sorted({(x + 1) % n_nodes, (x + n_nodes - 1) % n_nodes})
         for per_kind in ("none", "home", "past")]


@pytest.mark.parametrize("n_nodes,x,heir,per_kind", CASES)
def test_retire_properties(n_nodes, x, heir, per_kind):
    Z = 200
    st, fl = folded_table(Z, n_nodes, seed=10 * n_nodes + x)
    # hand-made words: never initialised, SHARED with a lone owner (x and not x), x with the only
    # written copy, and bits above the §5 fields
    st[3] = 0
    st[4] = word(1 << x, x, sm.SHARED)
    st[5] = word(1 << heir, heir, sm.SHARED, 1)
    st[6] = word(1 << x, x, sm.EXCLUSIVE, 1)
    st[7] = word((1 << n_nodes) - 1, x, sm.SHARED) | (0x155 << 19)
    assert valid(st)
    # none: the heir everywhere; home: coh_init's own homes, x's block among them; past: the first
    # 100 pages at the last node's home, the rest at a home past the nodes
    base, per = {"none": (1000, 0), "home": (0, -(-Z // n_nodes)),
                 "past": (150 * n_nodes - 100, 150)}[per_kind]
    before, faults = st.copy(), fl.copy()
    new, stats, out = sm.retire(st, x, heir, base, per, 0, Z, n_nodes)
    assert np.array_equal(st, before) and np.array_equal(fl, faults)   # the model copies
    own = np.array([(w >> 8) & 0xFF == x and (w >> 16) & 3 for w in before.tolist()], bool)
    # moved pages are exactly those x owned; x is gone everywhere; the invariants hold
    assert np.array_equal(out & 0x7FFFFFFF, base + np.flatnonzero(own))
    assert stats["moved"] == int(own.sum()) > 0
    assert stats["held"] == int((((before >> x) & 1) & ((before >> 16) & 3 != 0)).sum())
    assert stats["orphaned"] == int((out >> 31).sum()) >= 1
    assert not (((new >> x) & 1) & ((new >> 16) & 3 != 0)).any()
    assert not ((((new >> 8) & 0xFF) == x) & ((new >> 16) & 3 != 0)).any()
    assert valid(new)
    assert new[3] == 0 and new[7] >> 19 == 0x155
    assert ((new ^ before)[~own & (((before >> x) & 1) == 0)] == 0).all()
    assert sm.fields(int(new[5])) == (1 << heir, heir, sm.SHARED, 1)   # a lone owner stays SHARED
    # the heirs: the surviving home, else the heir
    for p in np.flatnonzero(own):
        h = (base + p) // per if per else heir
        if h >= n_nodes or h == x:
            h = heir
        c, o, s, d = sm.fields(int(new[p]))
        assert o == h and d == (int(before[p]) >> 18) & 1, p
        assert s == (sm.EXCLUSIVE if c == 1 << h else sm.SHARED), p
    if per_kind == "home":   # some homes are x itself
        assert any((base + p) // per == x for p in np.flatnonzero(own))
    if per_kind == "past":   # and some lie past the nodes
        assert (base + Z - 1) // per >= n_nodes
    # idempotent
    again, stats2, out2 = sm.retire(new, x, heir, base, per, 0, Z, n_nodes)
    assert np.array_equal(again, new) and len(out2) == 0
    assert stats2 == {"held": 0, "moved": 0, "orphaned": 0}
    # retiring is not a ban: the table stays a fold input, and x may come back
    ev = oracle.gen_events(np.full(Z, 3, np.uint64), seed=77, n_nodes=n_nodes, write_pct=30)
    f2 = fl.copy()
    rc, _ = oracle.coherence(new, f2, ev, n_nodes=n_nodes)
    assert rc == 0 and valid(new)


def test_retire_sub_range_leaves_the_rest():
    st, _ = folded_table(300, 4, seed=5)
    new, stats, out = sm.retire(st, 2, 0, 0, 0, 101, 77, 4)
    assert np.array_equal(new[:101], st[:101]) and np.array_equal(new[178:], st[178:])
    assert ((out & 0x7FFFFFFF) >= 101).all() and ((out & 0x7FFFFFFF) < 178).all()
    whole, _, _ = sm.retire(st, 2, 0, 0, 0, 0, 300, 4)
    assert np.array_equal(new[101:178], whole[101:178])


def test_select_equals_numpy():
    st, _ = folded_table(500, 8, seed=9)
    for mask, value in ((1 << 3, 1 << 3), (0xFF00 | DIRTY, (5 << 8) | DIRTY), (3 << 16, EXCL),
                        (0, 0), (0xFF, 0x100)):
        pages, count = sm.select(st, mask, value, 4096, 11, 400)
        want = 4096 + 11 + np.flatnonzero((st[11:411] & mask) == value)
        assert np.array_equal(pages, want) and count == len(want)
    assert sm.select(st, 0, 0)[1] == 500 and sm.select(st, 0xFF, 0x100)[1] == 0


def test_whole_array_model_equals_the_loop():
    """retire_vec / select_vec, which the GPU tests use on tables of millions of pages."""
    for n_nodes, seed in ((8, 21), (3, 22)):
        st, _ = folded_table(3000, n_nodes, seed=seed)
        st[7] = 0
        st[8] = 0x1FF | DIRTY                       # INVALID with stray bits
        st[9] = word(0xFF >> (8 - n_nodes), 1, sm.SHARED, 1) | (0x1234 << 19)
        for x in range(n_nodes):
            for base, per, first, n in ((0, 0, 0, 3000), (500, -(-3500 // n_nodes), 1, 2998),
                                        (1700, 300, 33, 2001)):
                args = (st, x, (x + 1) % n_nodes, base, per, first, n, n_nodes)
                a_st, a_stats, a_out = sm.retire(*args)
                b_st, b_stats, b_out = sm.retire_vec(*args)
                assert a_stats == b_stats and a_stats["moved"] > 0
                assert np.array_equal(a_st, b_st) and np.array_equal(a_out, b_out)
        for mask, value in ((1 << 1, 1 << 1), (0xFF00 | DIRTY, (2 << 8) | DIRTY), (0, 0),
                            (0xFF, 0x100)):
            a = sm.select(st, mask, value, 77, 5, 2900)
            b = sm.select_vec(st, mask, value, 77, 5, 2900)
            assert a[1] == b[1] and np.array_equal(a[0], b[0])


def test_symbols_are_exported_and_refuse_without_a_context():
    from gallocy_amd import _lib
    lib = _lib.load()
    assert "gdsm_coh_retire" in _lib.SIGNATURES and "gdsm_coh_select" in _lib.SIGNATURES
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.gdsm_coh_retire(None, 0, 1, 0, 0, 0, 0, None, 0, None, 0) == -22
    assert lib.gdsm_coh_retire(None, 0, 1, 0, 0, 0, 4, p, 4, p, 1) == -22
    assert lib.gdsm_coh_select(None, 0, 0, 0, 0, 0, None, 0, None) == -22
    assert lib.gdsm_coh_select(None, 1, 1, 0, 0, 4, p, 4, p) == -22
    assert list(buf) == [0] * 8
    n = C.c_int(-1)
    lib.gdsm_device_count(C.byref(n))
    if n.value == 0:   # no context to sweep: the only way to one says -ENODEV
        h = C.c_void_p()
        assert lib.gdsm_init(C.byref(h), 0, 16, 0) == -19 and not h.value
