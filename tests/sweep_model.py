"""Numpy restatement of docs/SPEC.md §14 (gdsm_coh_retire, gdsm_coh_select), written from the SPEC
text as one plain loop over the pages and independent of the kernels."""
from __future__ import annotations

import numpy as np

INVALID, SHARED, EXCLUSIVE = 0, 1, 2


def fields(w: int):
    """(copyset, owner, state, dirty) of a §5 state word."""
    return w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 3, (w >> 18) & 1


def retire(state, x: int, heir: int, base: int = 0, per: int = 0, first: int = 0, n=None,
           n_nodes: int = 8):
    """retire(x) over table pages [first, first + n) of `state` (uint32[n_pages]).
    -> (the new state array, {"held", "moved", "orphaned"}, moved_out as uint32: (base + p) |
    orphaned << 31 per moved page, ascending). The input is left as it is; bits 19-31 of a word are
    kept."""
    new = np.array(state, np.uint32)
    n = len(new) - first if n is None else n
    words = new.tolist()
    held = moved = orphaned = 0
    out = []
    for p in range(first, first + n):
        w = words[p]
        c, o, s, d = fields(w)
        if s == INVALID:
            continue
        c1 = c & ~(1 << x)
        if c != c1:
            held += 1
        if o != x:
            words[p] = (w & ~0xFF) | c1
            continue
        h = (base + p) // per if per else heir
        if h >= n_nodes or h == x:
            h = heir
        c2 = c1 | (1 << h)
        s2 = EXCLUSIVE if c2 == (1 << h) else SHARED
        orphan = s == EXCLUSIVE and d == 1
        moved += 1
        orphaned += orphan
        out.append((base + p) | (int(orphan) << 31))
        words[p] = (w & ~0x3FFFF) | c2 | (h << 8) | (s2 << 16) | (d << 18)
    return (np.array(words, np.uint32), {"held": held, "moved": moved, "orphaned": orphaned},
            np.array(out, np.uint32))


def select(state, mask: int, value: int, base: int = 0, first: int = 0, n=None):
    """-> (uint32 pages base + p of the table pages p of [first, first + n) with
    (word & mask) == value, ascending; their count)."""
    words = np.asarray(state, np.uint32).tolist()
    n = len(words) - first if n is None else n
    out = []
    for p in range(first, first + n):
        if (words[p] & mask) == value:
            out.append(base + p)
    return np.array(out, np.uint32), len(out)


def retire_vec(state, x: int, heir: int, base: int = 0, per: int = 0, first: int = 0, n=None,
               n_nodes: int = 8):
    """retire() on whole arrays, for tables too long for the loop; tests/test_sweep.py holds it to
    the loop's results."""
    new = np.array(state, np.uint32)
    n = len(new) - first if n is None else n
    w = new[first:first + n].astype(np.int64)
    c, o, s, d = w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 3, (w >> 18) & 1
    live = s != INVALID
    c1 = c & ~(1 << x)
    held = live & (c != c1)
    moved = live & (o == x)
    h = np.full(n, heir, np.int64)
    if per:
        h = (base + first + np.arange(n, dtype=np.int64)) // per
        h[(h >= n_nodes) | (h == x)] = heir
    c2 = c1 | (1 << h)
    s2 = np.where(c2 == (1 << h), EXCLUSIVE, SHARED)
    orphan = moved & (s == EXCLUSIVE) & (d == 1)
    gone = (w & ~0x3FFFF) | c2 | (h << 8) | (s2 << 16) | (d << 18)
    kept = (w & ~0xFF) | c1
    new[first:first + n] = np.where(live, np.where(moved, gone, kept), w).astype(np.uint32)
    at = np.flatnonzero(moved)
    out = ((base + first + at) | (orphan[at].astype(np.int64) << 31)).astype(np.uint32)
    stats = {"held": int(held.sum()), "moved": int(moved.sum()), "orphaned": int(orphan.sum())}
    return new, stats, out


def select_vec(state, mask: int, value: int, base: int = 0, first: int = 0, n=None):
    """select() on whole arrays."""
    st = np.asarray(state, np.uint32)
    n = len(st) - first if n is None else n
    at = np.flatnonzero((st[first:first + n] & np.uint32(mask)) == value)
    return (base + first + at).astype(np.uint32), len(at)
