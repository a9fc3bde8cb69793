"""The inputs of tests/test_gpu_diff_long.py are what that file takes them for (CPU only): the
density classes lie inside their bands, the mixed class holds every kind of work unit, the hint
walk takes every pair, and the stream comparison rejects a flipped byte and a moved offset."""
import time

import numpy as np
import pytest

from oracle import oracle
from tests import diff_long_cases as dl


@pytest.fixture(scope="module")
def streams():
    """(class, n) -> (rec_off, data, page kinds) by the oracle, computed once."""
    cache = {}

    def get(cls, n, hot=()):
        if (cls, n, hot) not in cache:
            t, c = dl.pages(cls, n, hot=hot)
            ro, data = oracle.diff_pages(t, c)
            cache[cls, n, hot] = (ro, data, dl.page_kinds(cls, n, hot=hot))
        return cache[cls, n, hot]
    return get


def test_generation_is_deterministic():
    """The same arguments give the same pages, another seed other pages; a page's TWIN is its
    background page and clean pages are left alone."""
    n = dl.N_LENGTHS[0]
    t, c = dl.pages("X", n)
    assert t.shape == c.shape == (n, dl.PAGE) and t.dtype == c.dtype == np.uint8
    t2, c2 = dl.pages("X", n)
    assert np.array_equal(t, t2) and np.array_equal(c, c2)
    del t2, c2
    assert np.array_equal(t[dl.BG_PAGES:2 * dl.BG_PAGES], dl.background())
    clean = dl.page_kinds("X", n) == dl.KINDS.index("clean")
    assert clean.any() and np.array_equal(t[clean], c[clean])
    dirty = np.flatnonzero(~clean)
    assert (t[dirty] != c[dirty]).any(axis=1).all()
    # no two dirty pages one background period apart carry the same bytes
    far = dirty[np.isin(dirty + dl.BG_PAGES, dirty)]
    assert len(far) > 1000 and (c[far] != c[far + dl.BG_PAGES]).any(axis=1).all()
    assert not np.array_equal(c, dl.pages("X", n, seed=7)[1])


def test_kinds_are_what_they_say():
    """One page of each kind: its record size and dirty chunks, by the oracle."""
    m = dl.kind_masks()
    chunks = m.reshape(len(dl.KINDS), dl.BG_PAGES, 256, 16).any(axis=3).sum(axis=2)
    k = dl.KINDS.index
    assert (chunks[k("clean")] == 0).all() and (chunks[k("e64")] == 64).all()
    assert chunks[k("s")].max() <= 6 and chunks[k("m")].min() >= 10 and chunks[k("m")].max() <= 24
    assert chunks[k("k15")].min() >= 56 and chunks[k("k15")].max() == 68
    assert 0.2 < (chunks[k("k15")] > 64).mean() < 0.5  # both sides of the 64-chunk limit
    n = 5 * 16 + 5
    kinds = dl.page_kinds("X", n)
    t, c = dl.pages("X", n)
    ro, _ = oracle.diff_pages(t, c)
    sz = dl.record_sizes(ro)
    fixed = {"clean": 0, "e64": 4 + 64 * 4 + 64, "full": 4 + 4 + 4096, "alt": 4 + 2048 * 4 + 2048}
    for name, want in fixed.items():
        assert (sz[kinds == k(name)] == want).all(), name
    assert sz[-1] == 10244


@pytest.mark.parametrize("cls", ["S", "M", "D"])
def test_density_classes_lie_inside_their_bands(cls, streams):
    """total // n + 1 of each homogeneous class at the GPU tests' n lies in its band of the
    automatic table, at least 10 % away from 112 and 480; and steers the variant it is meant to."""
    n = dl.N_WALK
    ro, _, _ = streams(cls, n)
    hint = dl.hint_of(ro[-1], n)
    lo, hi = dl.BANDS[cls]
    assert lo <= hint <= hi, (cls, hint)
    assert dl.expected_variant(hint) == {"S": 5, "M": 1, "D": 7}[cls]
    # the thresholds themselves
    assert [dl.expected_variant(h) for h in (0, 1, 112, 113, 480, 481)] == [5, 5, 5, 1, 1, 7]
    assert dl.BANDS["S"][1] * 1.1 <= 112 and dl.BANDS["M"][0] >= 113 * 1.1
    assert dl.BANDS["M"][1] * 1.1 <= 480 and dl.BANDS["D"][0] >= 481 * 1.1


@pytest.mark.parametrize("n,hot", [(dl.N_WALK, ()), (dl.N_REUSE, dl.HOT_REUSE)])
def test_mixed_class_holds_every_kind_of_unit(n, hot, streams):
    """Class X: of its aligned 16-page units at least 15 % each fit the LDS buffer, spill without
    late pages, and have late pages; of its 64-page units at least 15 % each fit and have late
    pages. The largest records fall on the first and the last page of units, the last page's is
    10 244 B, and the hint it leaves is a dense one."""
    t0 = time.perf_counter()
    ro, _, kinds = streams("X", n, hot)
    print(f"X n={n}: oracle {time.perf_counter() - t0:.2f} s,"
          f" {int(ro[-1]) // n} B/page,"
          f" 16-page units {['%.2f' % f for f in dl.unit_kinds(ro, 16)]},"
          f" 64-page units {['%.2f' % f for f in dl.unit_kinds(ro, 64)]}")
    assert min(dl.unit_kinds(ro, 16)) >= 0.15
    fits64, _, late64 = dl.unit_kinds(ro, 64)
    assert fits64 >= 0.15 and late64 >= 0.15
    sz = dl.record_sizes(ro)
    assert sz[-1] == 10244
    big = np.flatnonzero(sz == 10244)
    for unit in (16, 64):
        assert (big % unit == 0).sum() >= 10 and (big % unit == unit - 1).sum() >= 10
    assert dl.expected_variant(dl.hint_of(ro[-1], n)) == 7
    # units mix kinds: the block grid is shifted against the units
    per_unit = [len(set(kinds[u:u + 16])) for u in range(0, n - 16, 16)]
    assert np.mean(np.array(per_unit) > 1) > 0.3
    for a, b in hot:
        assert set(kinds[a:b]) <= {dl.KINDS.index(x) for x in dl.HOT}
        assert dl.unit_kinds(ro[a:b + 1] - ro[a], 16)[0] == 0  # every hot unit spills


def test_reuse_shape_reaches_the_second_use_of_a_spill_slot():
    n = dl.N_REUSE
    assert n == 82309
    wgs16 = ((n + 15) // 16 + 3) // 4
    assert wgs16 - dl.SPILL_WGS == 7  # tickets 1280 .. 1286 take slots 0 .. 6 again
    assert dl.HOT_REUSE == ((0, 7 * 64), (dl.SPILL_WGS * 64, n))
    assert ((n + 63) // 64 + 3) // 4 < dl.SPILL_WGS  # 64-page units: no reuse at this size
    for m in (dl.N_WALK,) + dl.N_LENGTHS:
        assert m > dl.DIFF_SHORT
    assert dl.N_WALK % 64 == 13 and (dl.N_WALK // 16) % 4 == 0 and (dl.N_WALK // 64) % 4 == 0
    assert dl.N_LENGTHS[0] == dl.DIFF_SHORT + 1 and dl.N_LENGTHS[1] % 256 == 0


def test_hint_walk_takes_every_pair():
    w = dl.HINT_WALK
    assert len(w) == 17
    assert {(a, b) for a, b in zip(w, w[1:])} == {(a, b) for a in dl.CLASSES for b in dl.CLASSES}


def test_raw_variant_rule():
    n = dl.N_WALK
    assert [dl.raw_variant(c, n) for c in (1, 128 * n, 128 * n + 1, 384 * n, 384 * n + 1)] == \
        [4, 4, 2, 2, 1]


def test_comparison_rejects_a_flipped_byte_and_a_moved_offset(streams):
    n = dl.N_WALK
    ro, data, _ = streams("X", n)
    assert dl.first_stream_difference(ro, data, ro, data) is None
    dl.assert_stream_equal(ro, np.concatenate([data, np.full(64, 0xA5, np.uint8)]), ro, data)
    # a late page: its unit's records pass the LDS buffer and the spill slot before it
    sz = dl.record_sizes(ro)
    u = next(u for u in range(0, n - 16, 16)
             if sz[u:u + 16].sum() > dl.LDS_BUF + dl.SPILL_SLOT and sz[u + 15] >= 4104)
    i = u + 15
    bad = data.copy()
    at = int(ro[i]) + int(sz[i]) - 5  # a payload byte
    bad[at] ^= 0x40
    why = dl.first_stream_difference(ro, bad, ro, data)
    assert why is not None and f"record {i} " in why and f"stream byte {at}" in why
    with pytest.raises(AssertionError, match=f"record {i} "):
        dl.assert_stream_equal(ro, bad, ro, data, "flipped")
    moved = ro.copy()
    moved[i + 1] += 4
    why = dl.first_stream_difference(moved, data, ro, data)
    assert why is not None and f"rec_off[{i + 1}]" in why and f"record {i} " in why
    with pytest.raises(AssertionError, match=f"record {i} "):
        dl.assert_stream_equal(moved, data, ro, data)
    assert dl.first_stream_difference(ro[:-1], data, ro, data) is not None
    assert dl.first_stream_difference(ro, data[:-1], ro, data) is not None
