"""A seeded corpus of structured Needleman-Wunsch pairs whose optimal paths run far from the
entries the GPU trace guesses for its strips (gdsm_nw.hip, phase A), and a census that counts, on
the CPU, which of the trace's branches every pair reaches. Helper module, checked on the CPU by
tests/test_nw_corpus.py and fed to the device by tests/test_gpu_nw.py. Numpy only: nothing here is
computed by the device library.

Pairs (corpus()): M, M1..M3 are random blocks over the family's alphabet, Z(k) a run of one byte
outside it, X(k) fresh random bytes over it; |M| = 1500, |Mi| = 700, k = 600.
    head_a        Z(k)+M | M          the path ends with k up-moves in column 0, over two strips
    head_b        M | Z(k)+M          a k-long left run on row 0 with three strips
    tail_a        M+Z(k) | M          a run of up-moves at column n2
    tail_b        M | M+Z(k)          a k-long left run on row n1, through ~10 recomputed regions
    shift+        X(k)+M | M+X(k)     the path runs k columns off every guess, one way
    shift-        M+X(k) | X(k)+M     and the other
    bulge         M1+M2+X(300)+M3 | M1+X(300)+M2+M3   300 off the guess in the middle strips only
    bulge_mirror  the same with a and b exchanged
    allsame_tall / allsame_wide / allsame_sq   'A' * (1500 | 700), (700 | 1500), (1100 | 1100)
    disjoint      1 * 1300 | 2 * 900  no match anywhere
    periodic      bytes(range(7)) * 200 | bytes(range(1, 7)) * 220
The whole family is built once over an alphabet of 200 ("name") and once over an alphabet of 3
("name/3"); the last five do not depend on the alphabet and are the same bytes in both.

Census (census()): a plain DP direction matrix with the reference's tie-break (1 diag if
dg >= max(lf, up), else 2 left if lf >= up, else 3 up; column 0 is up, row 0 is left), then the
trace's phases A and B over 512-row strips, exactly as trace_spec in scripts/dev/nw_ckpt_model.py
walks them: every strip from its guessed entry, then in order from the last strip each strip's
real entry, walked again on a mismatch until it meets the first walk.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

SEED = 0x4E57C0
STRIP = 512
LEN_M, LEN_MI, K, K_BULGE = 1500, 700, 600, 300
ALPHABETS = (200, 3)
Z_BYTE = 250  # outside both alphabets


def _family(alphabet, rng):
    def X(n):
        return bytes(rng.integers(0, alphabet, n, dtype=np.uint8))

    M, M1, M2, M3 = X(LEN_M), X(LEN_MI), X(LEN_MI), X(LEN_MI)
    Z = bytes([Z_BYTE]) * K
    bulge = (M1 + M2 + X(K_BULGE) + M3, M1 + X(K_BULGE) + M2 + M3)
    return {
        "head_a": (Z + M, M),
        "head_b": (M, Z + M),
        "tail_a": (M + Z, M),
        "tail_b": (M, M + Z),
        "shift+": (X(K) + M, M + X(K)),
        "shift-": (M + X(K), X(K) + M),
        "bulge": bulge,
        "bulge_mirror": bulge[::-1],
        "allsame_tall": (b"A" * 1500, b"A" * 700),
        "allsame_wide": (b"A" * 700, b"A" * 1500),
        "allsame_sq": (b"A" * 1100, b"A" * 1100),
        "disjoint": (b"\x01" * 1300, b"\x02" * 900),
        "periodic": (bytes(range(7)) * 200, bytes(range(1, 7)) * 220),
    }


@functools.lru_cache(maxsize=None)
def corpus():
    """{name: (a, b)} bytes, in a fixed order."""
    rng = np.random.default_rng(SEED)
    out = {}
    for alphabet in ALPHABETS:
        suffix = "" if alphabet == ALPHABETS[0] else f"/{alphabet}"
        for name, pair in _family(alphabet, rng).items():
            out[name + suffix] = pair
    assert all(len(s) < 2500 for p in out.values() for s in p)
    return out


# ---------------------------------------------------------------------------- census
def directions(a: bytes, b: bytes) -> np.ndarray:
    """D[y][x] in {1 diag, 2 left, 3 up} for the reference's recurrence (match +1, mismatch 0,
    gap -1) and tie-break; D[0][0] = 0. One np.maximum.accumulate per row: with G[x] = H[y][x] + x,
    G[x] = max(max(dg, up)[x] + x, G[x-1])."""
    av, bv = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    n1, n2 = len(av), len(bv)
    D = np.empty((n1 + 1, n2 + 1), np.uint8)
    D[0, :] = 2
    D[:, 0] = 3
    D[0, 0] = 0
    xs = np.arange(n2 + 1, dtype=np.int64)
    prev = -xs
    for y in range(1, n1 + 1):
        dg = prev[:-1] + (bv == av[y - 1])
        up = prev[1:] - 1
        g = np.concatenate(([-y], np.maximum(dg, up) + xs[1:]))
        row = np.maximum.accumulate(g) - xs
        lf = row[:-1] - 1
        D[y, 1:] = np.where(dg >= np.maximum(lf, up), 1, np.where(lf >= up, 2, 3))
        prev = row
    return D


def _row_exit(v):
    lo, typ = v
    return lo - (typ == 1)


@dataclass
class Census:
    out1: bytes
    out2: bytes
    strips: int            # S
    rewalked: int          # strips walked again in phase B
    merged_first_row: int  # re-walks that met the first walk on their first row
    merged_later: int      # re-walks that met it on a later row
    reached_top: int       # re-walks that left the strip's top row without meeting it
    col0_rows: int         # rows taken at column 0 inside re-walks
    max_deviation: int     # largest |real entry - guess| over the strips below the last
    row0_entry: int        # the column at which the path enters DP row 0


def _walk(D, s, y, x, rec, spec=None, spec_hi=None):
    """trace_spec's walk_strip over the direction matrix. -> (where the walk ended: "first",
    "later" or "top"; rows taken at column 0)."""
    top, y_first, col0 = STRIP * s + 1, y, 0
    while y >= top:
        if spec is not None and spec[y][0] <= x <= spec_hi:
            rec[y] = spec[y]
            return ("first" if y == y_first else "later"), col0
        code = 3 if x == 0 else int(D[y, x])
        if code == 2:
            x -= 1
            continue
        col0 += x == 0
        rec[y] = (x, code)
        if spec is not None:
            spec_hi = _row_exit(spec[y])
        y -= 1
        x -= code == 1
    return "top", col0


def census(a: bytes, b: bytes) -> Census:
    n1, n2 = len(a), len(b)
    D = directions(a, b)
    S = (n1 + STRIP - 1) // STRIP
    rec, guess = {}, {}
    ends = {"first": 0, "later": 0, "top": 0}
    col0 = dev = 0
    for s in range(S - 1, -1, -1):  # phase A
        ye = min(STRIP * (s + 1), n1)
        guess[s] = n2 if s == S - 1 else (ye * n2 + n1 // 2) // n1
        _walk(D, s, ye, guess[s], rec)
    spec = dict(rec)
    for s in range(S - 2, -1, -1):  # phase B
        xe = _row_exit(rec[STRIP * (s + 1) + 1])
        dev = max(dev, abs(xe - guess[s]))
        if xe != guess[s]:
            end, c0 = _walk(D, s, STRIP * (s + 1), xe, rec, spec, guess[s])
            ends[end] += 1
            col0 += c0
    # phase C: row y's entry column is the exit of row y + 1 (n2 for row n1)
    hi = [_row_exit(rec[y + 1]) if y < n1 else n2 for y in range(n1 + 1)]
    o1, o2 = bytearray(b"-" * hi[0]), bytearray(b[:hi[0]])
    for y in range(1, n1 + 1):
        lo, typ = rec[y]
        o1.append(a[y - 1])
        o2.append(b[lo - 1] if typ == 1 else 0x2D)
        o1 += b"-" * (hi[y] - lo)
        o2 += b[lo:hi[y]]
    return Census(bytes(o1), bytes(o2), S, sum(ends.values()), ends["first"], ends["later"],
                  ends["top"], col0, dev, hi[0])


@functools.lru_cache(maxsize=None)
def censuses():
    """{name: Census} of the whole corpus."""
    return {name: census(a, b) for name, (a, b) in corpus().items()}
