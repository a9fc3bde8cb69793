"""Numpy restatement of docs/SPEC.md §9 (gdsm_fetch, gdsm_notices_fetch_list), written from the
SPEC text and independent of the kernels: the block home mapping, what a fetch leaves in the
requesters' arenas, and which of a node's notices name a page it has to fetch."""
from __future__ import annotations

import numpy as np

PAGE = 4096


def per_of(total_pages: int, G: int) -> int:
    return -(-total_pages // G)


def home_of(page, total_pages: int, G: int):
    """Home rank of a global page (scalar or array): page // ceil(total_pages / G)."""
    return np.asarray(page) // per_of(total_pages, G)


def block_of(rank: int, total_pages: int, G: int):
    """(base, pages) of rank's home block; empty blocks when total_pages < G."""
    per = per_of(total_pages, G)
    base = min(total_pages, rank * per)
    return base, min(total_pages, (rank + 1) * per) - base


def valid_request(pages, dst_ids, total_pages: int, n_pages: int) -> bool:
    """A request list gdsm_fetch accepts: strictly ascending, < total_pages, destinations < n_pages."""
    p = np.asarray(pages, np.int64)
    d = p if dst_ids is None else np.asarray(dst_ids, np.int64)
    return bool((np.diff(p) > 0).all() and (p < total_pages).all() and (d < n_pages).all()
                and (p >= 0).all() and (d >= 0).all())


def fetch(replica_blocks, requests, dst_ids, arenas, total_pages: int):
    """The arenas after a fetch.
    replica_blocks[r]: the source arena of rank r, (>= block, 4096) uint8, page p of the block at
    p - base; requests[r]: rank r's ascending global page ids; dst_ids[r]: its destinations or None;
    arenas[r]: {name: (n_pages, 4096) uint8} of the arenas the call names. Returns new arrays;
    pages not named keep their contents."""
    G = len(replica_blocks)
    per = per_of(total_pages, G)
    out = []
    for r in range(G):
        req = np.asarray(requests[r], np.int64)
        dst = req if dst_ids[r] is None else np.asarray(dst_ids[r], np.int64)
        new = {k: v.copy() for k, v in arenas[r].items()}
        for p, d in zip(req, dst):
            h = int(p) // per
            src = replica_blocks[h][int(p) - h * per]
            for v in new.values():
                v[d] = src
        out.append(new)
    return out


def fetch_list(notices, want: int) -> np.ndarray:
    """Pages (u32, in notice order) of the notices whose access before is 0 and whose access after
    is 1 (want bit 0) or 2 (want bit 1). SPEC §5b packing: page | before << 32 | after << 34."""
    x = np.asarray(notices, np.uint64)
    before = (x >> np.uint64(32)) & np.uint64(3)
    after = (x >> np.uint64(34)) & np.uint64(3)
    keep = (before == 0) & ((((want & 1) != 0) & (after == 1)) | (((want & 2) != 0) & (after == 2)))
    return (x[keep] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
