"""Numpy restatement of docs/SPEC.md §15 (gdsm_coh_clean, gdsm_coh_lookup), written from the SPEC
text as one plain loop over the list's entries and independent of the kernels. Where a page is
listed more than once the loop takes the entries in list order, so the first occurrence cleans; the
device leaves open which occurrence does, so a test of repeats compares the statuses per page as
multisets (status_multisets)."""
from __future__ import annotations

import numpy as np

INVALID, SHARED, EXCLUSIVE = 0, 1, 2
CLEANED, ALREADY, STALE, SKIPPED, OUT_OF_RANGE = 0, 1, 2, 3, 4
DIRTY = 1 << 18
KEYS = ("cleaned", "already", "stale", "skipped")


def _pages(ids, n, base, n_pages):
    """(table page per entry as int64, -1 where the id is out of range)."""
    if ids is None:
        assert n <= n_pages
        return np.arange(n, dtype=np.int64)
    g = np.asarray(ids, np.uint32)[:n].astype(np.int64)
    p = g - base
    p[(g < base) | (p >= n_pages)] = -1
    return p


def clean(state, node: int, ids=None, n=None, base: int = 0):
    """gdsm_coh_clean over the list `ids` (global pages; None: table pages 0 .. n-1).
    -> (the new state array, {"cleaned", "already", "stale", "skipped"}, status uint8[n], bad: an id
    was out of range). The input is left as it is."""
    words = np.array(state, np.uint32).tolist()
    n = (len(words) if ids is None else len(ids)) if n is None else n
    pages = _pages(ids, n, base, len(words)).tolist()
    status = np.zeros(n, np.uint8)
    counts = [0, 0, 0, 0]
    bad = False
    for i, p in enumerate(pages):
        if p < 0:
            st, bad = OUT_OF_RANGE, True
        else:
            w = words[p]
            o, s, d = (w >> 8) & 0xFF, (w >> 16) & 3, (w >> 18) & 1
            if s == INVALID:
                st = SKIPPED
            elif o != node:
                st = STALE
            elif d == 0:
                st = ALREADY
            else:
                st = CLEANED
                words[p] = w & ~DIRTY
        status[i] = st
        counts[min(st, SKIPPED)] += 1
    return np.array(words, np.uint32), dict(zip(KEYS, counts)), status, bad


def clean_vec(state, node: int, ids=None, n=None, base: int = 0):
    """clean() on whole arrays, for long lists; tests/test_cohlist.py holds it to the loop."""
    new = np.array(state, np.uint32)
    n = (len(new) if ids is None else len(ids)) if n is None else n
    p = _pages(ids, n, base, len(new))
    inside = p >= 0
    w = np.where(inside, new[np.where(inside, p, 0)], 0).astype(np.int64)
    o, s, d = (w >> 8) & 0xFF, (w >> 16) & 3, (w >> 18) & 1
    status = np.where(~inside, OUT_OF_RANGE,
                      np.where(s == INVALID, SKIPPED,
                               np.where(o != node, STALE,
                                        np.where(d == 0, ALREADY, CLEANED)))).astype(np.uint8)
    # of the entries of one page that would clean it, the first in list order does
    at = np.flatnonzero(status == CLEANED)
    _, first = np.unique(p[at], return_index=True)
    later = np.ones(len(at), bool)
    later[first] = False
    status[at[later]] = ALREADY
    new[p[at[first]]] &= np.uint32(~DIRTY & 0xFFFFFFFF)
    counts = [int((status == k).sum()) for k in (CLEANED, ALREADY, STALE)]
    counts.append(int((status >= SKIPPED).sum()))
    return new, dict(zip(KEYS, counts)), status, bool((~inside).any())


def lookup(state, faults, ids=None, n=None, base: int = 0, shift: int = 0, mask: int = 0xFFFFFFFF):
    """gdsm_coh_lookup -> (out uint32[n], faults_out uint32[n], bad)."""
    words = np.asarray(state, np.uint32).tolist()
    fl = np.asarray(faults, np.uint32).tolist()
    n = (len(words) if ids is None else len(ids)) if n is None else n
    out, fo = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    bad = False
    for i, p in enumerate(_pages(ids, n, base, len(words)).tolist()):
        if p < 0:
            bad = True
            continue
        w = words[p]
        out[i] = 0 if (w >> 16) & 3 == INVALID else (w >> shift) & mask
        fo[i] = fl[p]
    return out, fo, bad


def lookup_vec(state, faults, ids=None, n=None, base: int = 0, shift: int = 0,
               mask: int = 0xFFFFFFFF):
    """lookup() on whole arrays."""
    st, fl = np.asarray(state, np.uint32), np.asarray(faults, np.uint32)
    n = (len(st) if ids is None else len(ids)) if n is None else n
    p = _pages(ids, n, base, len(st))
    inside = p >= 0
    q = np.where(inside, p, 0)
    w = st[q].astype(np.int64)
    live = inside & (((w >> 16) & 3) != INVALID)
    out = np.where(live, (w >> shift) & mask, 0).astype(np.uint32)
    return out, np.where(inside, fl[q], 0).astype(np.uint32), bool((~inside).any())


def status_multisets(ids, status):
    """{page id: the sorted statuses of its entries}."""
    m: dict = {}
    for g, s in zip(np.asarray(ids).tolist(), np.asarray(status).tolist()):
        m.setdefault(g, []).append(s)
    return {g: sorted(v) for g, v in m.items()}
