"""numpy model of gdsm_runs_split (docs/SPEC.md §13): one diff stream into one per destination.

A stream is (rec_off uint64[n + 1], data uint8[>= rec_off[n]]). The model gives the call's verdict
(0, -EINVAL, -ENOSPC), the G complete outputs, the counts, and what a device buffer of a given
capacity holds afterwards (the guarded writes of the raw form)."""
from __future__ import annotations

import numpy as np

EINVAL, ENOSPC = -22, -28
DROP_EMPTY = 1
MAX_NODES = 8
ERR_IDS, ERR_STREAM = 8, 16


def immediate(n, G, dest_given, per, flags, out_ptrs=(), in_ptrs=()):
    """The refusals made on the arguments alone: 0 or -EINVAL. out_ptrs: per output (rec_off, data)
    addresses; in_ptrs: the input's (rec_off, data)."""
    if not 1 <= G <= MAX_NODES:
        return EINVAL
    if bool(dest_given) == (per != 0):
        return EINVAL
    if flags & ~DROP_EMPTY:
        return EINVAL
    if n > 1 << 32:
        return EINVAL
    seen_ro, seen_data = set(in_ptrs[:1]), set(in_ptrs[1:2])
    for ro, data in out_ptrs:
        if ro in seen_ro or (data and data in seen_data):
            return EINVAL
        seen_ro.add(ro)
        seen_data.add(data)
    return 0


def offsets_malformed(rec_off, cap):
    ro = np.asarray(rec_off, np.uint64)
    if ro[0] != 0 or (ro & np.uint64(3)).any():
        return True
    if (ro[1:] < ro[:-1]).any():
        return True
    return int(ro[-1]) > cap


def destinations(n, sizes, ids, dest, per, G, flags):
    """(mask uint32[n] of the destinations each record goes to, page uint32[n] written for it,
    bad: a mask bit >= G or a home >= G somewhere)."""
    ids = np.arange(n, dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32)[:n]
    if dest is not None:
        mask = np.asarray(dest, np.uint32)[:n].copy()
        bad = bool((mask >> np.uint32(G)).any())
        page = ids.copy()
    else:
        home = ids.astype(np.uint64) // np.uint64(per)
        bad = bool((home >= G).any())
        mask = (np.uint32(1) << (home & np.uint64(7)).astype(np.uint32)).astype(np.uint32)
        page = (ids.astype(np.uint64) - home * np.uint64(per)).astype(np.uint32)
    if flags & DROP_EMPTY:
        mask[sizes == 0] = 0
    return mask, page, bad


def empty_outputs(G):
    return [(np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint32))
            for _ in range(G)]


def split(rec_off, data, ids=None, dest=None, per=0, G=1, flags=0, cap=None):
    """(err bits, outs, counts): outs[d] = (rec_off uint64[c_d + 1], data uint8[b_d], ids
    uint32[c_d]), counts uint64[G, 2] = {records, bytes}. err != 0 (ERR_STREAM / ERR_IDS): the input
    is refused, the outputs are empty and the counts 0."""
    ro = np.asarray(rec_off, np.uint64)
    data = np.asarray(data, np.uint8)
    n = len(ro) - 1
    cap = len(data) if cap is None else cap
    err = 0
    if offsets_malformed(ro, cap):
        err |= ERR_STREAM
        sizes = np.zeros(n, np.uint64)  # nothing is read through malformed offsets
    else:
        sizes = np.diff(ro)
    mask, page, bad = destinations(n, sizes, ids, dest, per, G, flags)
    if bad:
        err |= ERR_IDS
    if err:
        return err, empty_outputs(G), np.zeros((G, 2), np.uint64)
    outs, counts = [], np.zeros((G, 2), np.uint64)
    for d in range(G):
        sel = np.flatnonzero((mask >> np.uint32(d)) & np.uint32(1))
        o = np.zeros(len(sel) + 1, np.uint64)
        o[1:] = np.cumsum(sizes[sel])
        parts = [data[int(ro[i]):int(ro[i + 1])] for i in sel]
        buf = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        outs.append((o, buf.astype(np.uint8), page[sel]))
        counts[d] = (len(sel), int(o[-1]))
    return 0, outs, counts


def verdict(err, counts, out_caps, out_n_caps):
    """The context form's return value."""
    if err:
        return EINVAL
    for d in range(len(counts)):
        if counts[d, 0] > out_n_caps[d] or counts[d, 1] > out_caps[d]:
            return ENOSPC
    return 0


def written(out, cap, n_cap):
    """What the guarded writes leave of one complete output in buffers of the given capacities:
    (rec_off entries [0, k), data bytes [0, m), ids [0, q))."""
    o, buf, ids = out
    k = min(len(o), n_cap + 1)
    m = min(len(buf), cap & ~3)
    q = min(len(ids), n_cap)
    return o[:k], buf[:m], ids[:q]
