"""Inputs for the long-list diff tests (tests/test_gpu_diff_long.py): page sets of a chosen stream
density, the automatic geometry table they are meant to steer, and a stream comparison that
names the first differing record. Pure numpy, deterministic by seed; checked on the CPU by
tests/test_diff_long_cases.py.

Every set is built from a 2048-page random background: TWIN page i is background page i % 2048,
CURRENT page i is that page changed as its kind says. A kind is a pool of 2048 changed pages (one
per background page); two of a dirty page's changed bytes then take values that depend on i, so
that no two pages of a list carry the same record.

Kinds (a page's dirty 16-B chunks and the bytes changed inside them):
  clean  no byte changed
  s      1-6 dirty chunks, ~3 bytes each, a quarter of the pages clean: ~45 B of stream per page
  m      10-24 dirty chunks, ~4 bytes each: ~280 B per page
  e64    64 one-byte runs in 64 different chunks (324 B: the most chunks the diff kernel buffers)
  k15    56-68 dirty chunks, half their bytes changed: ~1.5 KB per page; the pages with more than
         64 dirty chunks are re-read by the kernel whatever the room in its buffers
  full   every byte changed: one run, a 4104-B record
  alt    every other byte changed: 2048 runs, a 10 244-B record (the largest there is)

Classes: S, M and D are all s, all m and all k15. X is mixed: blocks of 16 consecutive pages of
one kind each, the block grid shifted by 5 pages (so that 16- and 64-page work units hold two to
five blocks and the largest records fall on the first and the last page of units), the blocks'
kinds drawn per region of 8 blocks, a region being quiet (clean / e64) or busy (every kind); the
list's last page is alt. `hot` ranges of X hold only k15, full and alt blocks.
"""
from __future__ import annotations

import functools

import numpy as np

PAGE = 4096
BG_PAGES = 2048
KINDS = ("clean", "s", "m", "e64", "k15", "full", "alt")
CLASSES = ("S", "M", "D", "X")

# The automatic long-list geometry (gallocy_amd/csrc/gdsm_pages.hip, launch_diff_impl): lists of
# more than DIFF_SHORT pages, by the hint = stream bytes // pages + 1 the context learned last.
DIFF_SHORT = 32768
DENSE64, DENSE16 = 112, 480
LDS_BUF, SPILL_SLOT = 8192, 24576
SPILL_WGS = 1280
FORM_GRID, FORM_SOLO, FORM_CHAIN_PAGE, FORM_CHAIN_WAVE = 0, 1, 2, 3
# class -> the band its hint lies in, 10 % away from the thresholds
BANDS = {"S": (1, int(DENSE64 / 1.1)), "M": (int(np.ceil((DENSE64 + 1) * 1.1)), int(DENSE16 / 1.1)),
         "D": (int(np.ceil((DENSE16 + 1) * 1.1)), 10245)}


def hint_of(total, n: int) -> int:
    """The hint gdsm_runs_total leaves after a stream of `total` bytes for n > DIFF_SHORT pages
    (None: nothing learned yet)."""
    return 0 if total is None else int(total) // n + 1


def expected_variant(hint: int) -> int:
    """The variant a context's long-list diff takes under `hint`."""
    if hint == 0 or hint <= DENSE64:
        return 5
    return 1 if hint <= DENSE16 else 7


def raw_variant(cap: int, n: int) -> int:
    """... and a raw caller's, whose workspace has no spill pool: by its capacity per page."""
    return 4 if cap <= 128 * n else 2 if cap <= 384 * n else 1


# A walk over the classes that starts with no hint and takes every ordered pair (class that set
# the hint, class being diffed) once: 17 diffs.
HINT_WALK = "SSMMDDXXSDSXMXDMS"


@functools.lru_cache(maxsize=None)
def background(seed: int = 2026) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (BG_PAGES, PAGE), dtype=np.uint8)


def _chunk_masks(rng, lo: int, hi: int, density: float, clean_frac: float = 0.0) -> np.ndarray:
    """bool[BG_PAGES, 256, 16]: per page lo..hi dirty chunks at random places, each of their
    bytes changed with probability `density`, at least one per dirty chunk."""
    cnt = rng.integers(lo, hi + 1, BG_PAGES)
    cnt[rng.random(BG_PAGES) < clean_frac] = 0
    rank = rng.random((BG_PAGES, 256)).argsort(axis=1).argsort(axis=1)
    sel = rank < cnt[:, None]
    bits = rng.random((BG_PAGES, 256, 16)) < density
    forced = rng.integers(0, 16, (BG_PAGES, 256))
    np.put_along_axis(bits, forced[:, :, None], True, axis=2)
    return bits & sel[:, :, None]


@functools.lru_cache(maxsize=None)
def kind_masks(seed: int = 2026) -> np.ndarray:
    """bool[len(KINDS), BG_PAGES, PAGE]: the bytes each kind changes in each background page."""
    rng = np.random.default_rng(seed + 1)
    m = np.zeros((len(KINDS), BG_PAGES, 256, 16), bool)
    m[KINDS.index("s")] = _chunk_masks(rng, 1, 6, 0.15, clean_frac=0.25)
    m[KINDS.index("m")] = _chunk_masks(rng, 10, 24, 0.25)
    one = np.zeros((BG_PAGES, 256, 16), bool)
    rank = rng.random((BG_PAGES, 256)).argsort(axis=1).argsort(axis=1)
    pos = rng.integers(1, 15, (BG_PAGES, 256))  # never a chunk's edge: the runs stay apart
    np.put_along_axis(one, pos[:, :, None], True, axis=2)
    m[KINDS.index("e64")] = one & (rank < 64)[:, :, None]
    m[KINDS.index("k15")] = _chunk_masks(rng, 56, 68, 0.5)
    m[KINDS.index("full")] = True
    m[KINDS.index("alt")][:, :, 0::2] = True
    return m.reshape(len(KINDS), BG_PAGES, PAGE)


@functools.lru_cache(maxsize=None)
def _pool(seed: int = 2026):
    """(pool uint8[len(KINDS) * BG_PAGES, PAGE], p0, p1): the changed pages of every kind, and per
    pool page the places of its first and last changed byte (0 for a clean page)."""
    bg, m = background(seed), kind_masks(seed)
    delta = np.random.default_rng(seed + 2).integers(1, 256, (BG_PAGES, PAGE), dtype=np.uint8)
    pool = np.where(m, bg[None] ^ delta[None], bg[None]).reshape(-1, PAGE)
    flat = m.reshape(-1, PAGE)
    p0 = flat.argmax(axis=1)
    p1 = PAGE - 1 - flat[:, ::-1].argmax(axis=1)
    p1[~flat.any(axis=1)] = 0
    return pool, p0, p1, flat.any(axis=1)


QUIET = {"clean": 0.85, "e64": 0.15}
BUSY = {"clean": 0.10, "e64": 0.20, "k15": 0.35, "full": 0.20, "alt": 0.15}
HOT = {"k15": 0.5, "full": 0.25, "alt": 0.25}
X_SHIFT, X_BLOCK, X_REGION, X_QUIET = 5, 16, 8, 0.4


def _draw(rng, dist: dict, size: int) -> np.ndarray:
    names = list(dist)
    k = rng.choice(len(names), size=size, p=[dist[x] for x in names])
    return np.array([KINDS.index(x) for x in names])[k]


def page_kinds(cls: str, n: int, seed: int = 2026, hot=()) -> np.ndarray:
    """uint8[n]: the kind (index into KINDS) of every page of a class."""
    if cls in ("S", "M", "D"):
        return np.full(n, KINDS.index({"S": "s", "M": "m", "D": "k15"}[cls]), np.uint8)
    assert cls == "X"
    rng = np.random.default_rng(seed + 3)
    blocks = (n + X_BLOCK - 1) // X_BLOCK + 1  # block b: pages [16 b - 11, 16 b + 5)
    quiet = np.repeat(rng.random(blocks // X_REGION + 1) < X_QUIET, X_REGION)[:blocks]
    kind = np.where(quiet, _draw(rng, QUIET, blocks), _draw(rng, BUSY, blocks))
    hot_kind = _draw(rng, HOT, blocks)
    per_page = np.repeat(kind, X_BLOCK)[X_BLOCK - X_SHIFT:][:n]
    hot_page = np.repeat(hot_kind, X_BLOCK)[X_BLOCK - X_SHIFT:][:n]
    for a, b in hot:
        per_page[a:b] = hot_page[a:b]
    per_page[n - 1] = KINDS.index("alt")
    return per_page.astype(np.uint8)


def pages(cls: str, n: int, seed: int = 2026, hot=()):
    """(twin, current), uint8[n, PAGE] each, of class `cls`."""
    pool, p0, p1, dirty = _pool(seed)
    i = np.arange(n)
    twin = background(seed)[i % BG_PAGES]
    src = page_kinds(cls, n, seed, hot).astype(np.int64) * BG_PAGES + i % BG_PAGES
    cur = pool[src]
    # two changed bytes of every dirty page take a value of the page's own (never the twin's)
    d = np.flatnonzero(dirty[src])
    cur[d, p1[src[d]]] = twin[d, p1[src[d]]] ^ (1 + (d // 255) % 255).astype(np.uint8)
    cur[d, p0[src[d]]] = twin[d, p0[src[d]]] ^ (1 + d % 255).astype(np.uint8)
    return twin, cur


def record_sizes(rec_off) -> np.ndarray:
    return np.diff(np.asarray(rec_off, np.uint64)).astype(np.int64)


def unit_kinds(rec_off, unit: int):
    """Fractions of the aligned `unit`-page units of a stream whose records (fit the LDS buffer,
    spill without late pages, have late pages)."""
    sz = record_sizes(rec_off)
    sums = np.add.reduceat(sz, np.arange(0, len(sz), unit))
    fits = sums <= LDS_BUF
    late = sums > LDS_BUF + SPILL_SLOT
    return fits.mean(), (~fits & ~late).mean(), late.mean()


def first_stream_difference(got_off, got_data, want_off, want_data):
    """None when the stream (got_off, got_data) equals (want_off, want_data): rec_off equal and
    the data equal up to rec_off[n]. Otherwise a sentence naming the first differing record."""
    got_off, want_off = np.asarray(got_off, np.uint64), np.asarray(want_off, np.uint64)
    if got_off.shape != want_off.shape:
        return f"{len(got_off) - 1} records, expected {len(want_off) - 1}"
    bad = np.flatnonzero(got_off != want_off)
    if len(bad):
        i = int(bad[0])
        return (f"rec_off[{i}] = {int(got_off[i])}, expected {int(want_off[i])}: record "
                f"{max(i - 1, 0)} is the first that differs")
    total = int(want_off[-1])
    if len(got_data) < total or len(want_data) < total:
        return f"data holds {min(len(got_data), len(want_data))} bytes, rec_off[n] = {total}"
    ne = np.flatnonzero(np.asarray(got_data[:total]) != np.asarray(want_data[:total]))
    if len(ne):
        b = int(ne[0])
        i = int(np.searchsorted(want_off, b, side="right")) - 1
        return (f"record {i} differs at its byte {b - int(want_off[i])} (stream byte {b}): "
                f"{int(got_data[b])}, expected {int(want_data[b])}")
    return None


def assert_stream_equal(got_off, got_data, want_off, want_data, what=""):
    why = first_stream_difference(got_off, got_data, want_off, want_data)
    assert why is None, f"{what}: {why}" if what else why


# ---- the shapes of the GPU tests
N_WALK = 33037          # 516 64-page units + 13 pages, 2064 16-page units + 13
N_LENGTHS = (32769, 33024)
N_REUSE = 4 * 16 * SPILL_WGS + 6 * 64 + 5  # 82 309: six workgroups and 5 pages past the reuse
HOT_REUSE = ((0, 448), (4 * 16 * SPILL_WGS, N_REUSE))
N_IDS_CTX, N_IDS_LIST = 2048, 262144 + 300


def gpu_cases():
    """Every (class, n, hot) whose oracle stream the GPU tests compare with."""
    out = [(c, N_WALK, ()) for c in CLASSES]
    out += [("X", n, ()) for n in N_LENGTHS]
    out.append(("X", N_REUSE, HOT_REUSE))
    return out
