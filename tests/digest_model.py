"""Numpy restatement of docs/SPEC.md §10 (the page digest) and §11 (gdsm_fetch_changed), written
from the SPEC text and independent of the kernels: the keys, the two NH rows of a page, and what a
conditional fetch leaves behind (the arenas through tests/fetch_model.fetch, plus the `changed`
flags and the four `stats` counts)."""
from __future__ import annotations

import numpy as np

from tests import fetch_model as fm

PAGE = 4096
WORDS = PAGE // 4
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1


def mix64(z: int) -> int:
    """SPEC §6 (python integers)."""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


# K[j] = mix64(j + 1) >> 32, j in [0, 1028): two Toeplitz-shifted rows of 1024 keys
KEYS = np.array([mix64(j + 1) >> 32 for j in range(WORDS + 4)], np.uint64)


def digests(pages) -> np.ndarray:
    """(n, 2) uint64: (S0, S1) of each 4096-byte page of `pages` ((n, 4096) uint8)."""
    p = np.ascontiguousarray(pages, np.uint8).reshape(-1, PAGE)
    x = p.view("<u4").astype(np.uint64)          # (n, 1024) little-endian words
    out = np.empty((len(p), 2), np.uint64)
    mask = np.uint64(M32)
    for t in (0, 1):
        k = KEYS[4 * t:4 * t + WORDS]
        a = (x[:, 0::2] + k[0::2]) & mask        # both < 2^32: the product wraps mod 2^64,
        b = (x[:, 1::2] + k[1::2]) & mask        # which is what the sum wants
        with np.errstate(over="ignore"):
            out[:, t] = (a * b).sum(axis=1, dtype=np.uint64)
    return out


def digest_scalar(page) -> tuple:
    """(S0, S1) of one page with python integers, term by term as §10 writes it."""
    b = bytes(np.ascontiguousarray(page, np.uint8).reshape(PAGE))
    x = [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(WORDS)]
    K = [mix64(j + 1) >> 32 for j in range(WORDS + 4)]
    s = []
    for t in (0, 1):
        acc = 0
        for i in range(WORDS // 2):
            acc += ((x[2 * i] + K[2 * i + 4 * t]) & M32) * ((x[2 * i + 1] + K[2 * i + 1 + 4 * t]) & M32)
        s.append(acc & M64)
    return tuple(s)


def digests_differ(mine, home) -> np.ndarray:
    """Per pair of pages: their digests differ. Pairs equal byte for byte are not digested (equal
    pages have equal digests), so a long list of mostly unchanged pages stays cheap."""
    out = np.zeros(len(mine), bool)
    ne = np.flatnonzero((mine != home).any(axis=1))
    out[ne] = (digests(mine[ne]) != digests(home[ne])).any(axis=1)
    return out


def first_arena(names) -> str:
    """The arena whose copy the requester offers: CURRENT when it is named, else TWIN."""
    return "current" if "current" in names else "twin"


def pairs(replica_blocks, requests, dst_ids, arenas, total_pages: int):
    """Per rank (mine, home, local): for every entry of its list the requester's copy (arena A at
    dst(i)) and the home copy, (n, 4096) uint8 each, and whether the entry is homed at the rank."""
    G = len(replica_blocks)
    per = fm.per_of(total_pages, G)
    out = []
    for r in range(G):
        req = np.asarray(requests[r], np.int64)
        dst = req if dst_ids[r] is None else np.asarray(dst_ids[r], np.int64)
        a = arenas[r][first_arena(arenas[r].keys())]
        h = req // per
        home = np.empty((len(req), PAGE), np.uint8)
        for k in np.unique(h):
            sel = h == k
            home[sel] = replica_blocks[int(k)][req[sel] - int(k) * per]
        out.append((a[dst].reshape(-1, PAGE), home, h == r))
    return out


def fetch_changed(replica_blocks, requests, dst_ids, arenas, total_pages: int):
    """The model of gdsm_fetch_changed. Arguments as fetch_model.fetch (arenas[r] holds exactly the
    arenas the call names). Returns (arenas after, changed[r] uint32 per entry, stats[r] = [remote
    transferred, remote skipped, local differing, local equal]). A remote entry is judged by its
    digest, a local one byte for byte; the arenas are gdsm_fetch's."""
    changed, stats = [], []
    for mine, home, local in pairs(replica_blocks, requests, dst_ids, arenas, total_pages):
        by_bytes = (mine != home).any(axis=1)
        by_digest = digests_differ(mine, home)
        ch = np.where(local, by_bytes, by_digest)
        changed.append(ch.astype(np.uint32))
        stats.append([int((ch & ~local).sum()), int((~ch & ~local).sum()),
                      int((ch & local).sum()), int((~ch & local).sum())])
    return fm.fetch(replica_blocks, requests, dst_ids, arenas, total_pages), changed, stats
