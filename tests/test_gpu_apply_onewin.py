"""The long-list apply (gdsm_tune "apply_variant" 0, the default, and 8, the flat form with its
tasks in a scattered order, named) on streams built around a staging window's edges: tasks whose
64 records fill a window exactly, by 4 B too much and twice over (for a 4 KiB and a 5 KiB
window); partial runs of every length at every alignment; a long run among word runs; malformed
records and stream offsets out of order between good records. REPLICA is compared byte for byte
with the C oracle's apply of the same stream, record by record (SPEC §4: a malformed record
writes nothing, every other record is applied, -EINVAL at sync); it starts from bytes that equal
neither TWIN nor CURRENT, so a byte outside the runs that is touched shows."""
import functools

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import _lib
from gallocy_amd.gdsm import GdsmError, HostRuns, Runs
from oracle import oracle

pytestmark = pytest.mark.gpu

VARIANTS = (0, 8)
WINDOWS = (4096, 5120)  # the staging window, and the largest that keeps six workgroups per CU
LONG = 16384            # lists above this take the flat forms
MAX_RECORD = 10244      # GDSM_MAX_RECORD: 2048 one-byte runs


def _rec(runs):
    """The record (SPEC §3) of `runs`, a list of (offset, payload bytes)."""
    hdr = np.array([len(runs)] + [o | (len(b) << 16) for o, b in runs], "<u4").tobytes()
    pay = b"".join(b for _, b in runs)
    return hdr + pay + b"\0" * (-len(pay) % 4)


def _words(rng, k, length=8):
    """k runs of `length` bytes at distinct 16-B slots of a page, sorted."""
    slots = np.sort(rng.choice(256, k, replace=False))
    return [(int(s) * 16, rng.integers(1, 256, length, dtype=np.uint8).tobytes()) for s in slots]


def _task_of(rng, total):
    """64 well-formed records of word runs whose sizes add up to `total` bytes exactly."""
    k, rem = divmod(total - 64 * 4, 12)  # an 8-B run takes 12 B of its record, a 12-B run 16
    assert rem % 4 == 0 and k >= 64
    recs = []
    for i in range(64):
        runs = _words(rng, k // 64 + (1 if i < k % 64 else 0))
        if i < rem // 4:
            runs[0] = (runs[0][0], runs[0][1] + b"\x5a\xa5\x3c\xc3")
        recs.append(_rec(runs))
    assert sum(len(r) for r in recs) == total
    return recs


def _stream(recs):
    ro = np.zeros(len(recs) + 1, np.uint64)
    ro[1:] = np.cumsum([len(r) for r in recs])
    return ro, np.frombuffer(b"".join(recs), np.uint8).copy()


def _oracle_apply(rep, ro, data, ids=None):
    """REPLICA after the oracle applied the stream record by record, and how many records it
    refused."""
    want, bad = rep.copy(), 0
    for i in range(len(ro) - 1):
        if ro[i + 1] != ro[i]:
            page = i if ids is None else int(ids[i])
            bad += oracle.apply(want, ro[i:i + 2], data, ids=np.array([page], np.uint32)) != 0
    return want, bad


def _filled(rng, special, n=LONG + 1, runs_per_record=5):
    """n records of word runs, with the records of `special` ({first record: list}) in place."""
    recs = [_rec(_words(rng, runs_per_record)) for _ in range(n)]
    for at, lst in special.items():
        assert at + len(lst) <= n
        recs[at:at + len(lst)] = lst
    return recs


def _case(recs, seed, ro=None):
    rng = np.random.default_rng(seed)
    ro2, data = _stream(recs)
    ro = ro2 if ro is None else ro
    rep = rng.integers(0, 256, (len(recs), 4096), dtype=np.uint8)
    want, bad = _oracle_apply(rep, ro, data)
    return rep, ro, data, want, bad, None


@functools.lru_cache(maxsize=None)
def _plain(n, permuted):
    tw, cu = oracle.gen_pages(n, seed=2026, mode=0, ppm=10000)
    ids = np.random.default_rng(n).permutation(n).astype(np.uint32) if permuted else None
    ro, data = oracle.diff_pages(tw, cu) if ids is None else oracle.diff_pages(tw[ids], cu[ids])
    rep = tw ^ 0x5A  # clean bytes: TWIN == CURRENT != REPLICA
    want, bad = _oracle_apply(rep, ro, data, ids)
    assert bad == 0 and np.array_equal(want, np.where(tw != cu, cu, rep))
    return rep, ro, data, want, bad, ids


@functools.lru_cache(maxsize=None)
def _window_edges():
    rng = np.random.default_rng(41)
    special, at = {}, 64  # every special task starts on a task boundary (64 records)
    for w in WINDOWS:
        for total in (w, w + 4, 2 * w + 4):
            special[at] = _task_of(rng, total)
            at += 128
    dense = _rec([(0, rng.integers(0, 256, 4096, dtype=np.uint8).tobytes())])
    assert len(dense) == 4104
    special[at + 20] = [dense]
    largest = _rec([(2 * i, bytes([1 + i % 255])) for i in range(2048)])
    assert len(largest) == MAX_RECORD
    special[at + 128 + 31] = [largest]
    special[at + 256] = [b""] * 64
    return _case(_filled(rng, special), 42)


@functools.lru_cache(maxsize=None)
def _partial_runs():
    rng = np.random.default_rng(43)

    def run(off, length):
        return off, rng.integers(1, 256, length, dtype=np.uint8).tobytes()

    # every length 1..17 at every start offset mod 16, one run per 64-B slot, 64 runs per record:
    # consecutive records of 64 partial runs fill whole batches with them
    shapes = [(s, length) for length in range(1, 18) for s in range(16)]
    recs = []
    for r0 in range(0, len(shapes), 64):
        recs.append(_rec([run(64 * i + s, length) for i, (s, length) in enumerate(shapes[r0:r0 + 64])]))
    # 130 runs of 3 B straddling nothing, two per 32 B: more than 65 partial runs in one batch
    recs.append(_rec([run(32 * i + 5, 3) for i in range(65)] + [run(2100 + 16 * i, 7) for i in range(65)]))
    # runs ending on the page's last byte
    for length in (1, 7, 8, 9, 16, 17, 33):
        recs.append(_rec([run(8, 8), run(4096 - length, length)]))
    # two runs inside one 16-B chunk, three, and a chunk shared by the end of one run and the
    # start of the next
    recs.append(_rec([run(17, 3), run(22, 5), run(160, 1), run(162, 1), run(164, 12), run(200, 10),
                      run(212, 30)]))
    # 8 B at offset 4 (not a whole half), at 8 (one), 4 B at 4, 16 B at 8 (two halves of two chunks)
    recs.append(_rec([run(4, 8), run(40, 8), run(68, 4), run(136, 16), run(4084, 8)]))
    special = {64 * 3 + 7: recs[:3], 64 * 9: recs[3:], 64 * 200 + 60: recs}
    return _case(_filled(rng, special), 44)


@functools.lru_cache(maxsize=None)
def _long_among_words():
    rng = np.random.default_rng(45)
    special = {}
    for t, length in enumerate((33, 48, 49, 1000, 4000)):
        for off in (0, 7, 16):
            runs = _words(rng, 6)
            runs = [r for r in runs if r[0] < 16] + \
                   [(24 + off, rng.integers(1, 256, length, dtype=np.uint8).tobytes())] + \
                   [r for r in runs if r[0] >= 24 + off + length + 16]
            special[64 * (5 + 7 * t) + 3 + 11 * (off % 5)] = [_rec(_words(rng, 3)), _rec(runs)]
    # a batch of long runs only, and one where every run spans three chunks
    special[64 * 100] = [_rec([(512 * i + 3, rng.integers(1, 256, 300, dtype=np.uint8).tobytes())
                               for i in range(8)])]
    special[64 * 101 + 9] = [_rec([(64 * i + 15, rng.integers(1, 256, 18, dtype=np.uint8).tobytes())
                                   for i in range(64)])]
    return _case(_filled(rng, special), 46)


@functools.lru_cache(maxsize=None)
def _malformed():
    rng = np.random.default_rng(47)
    # 88-B records: 46 of them fill a 4 KiB window and 58 a 5 KiB one, so the records below sit
    # on either window's boundaries, inside a window and on a task boundary
    recs = _filled(rng, {}, n=LONG + 64, runs_per_record=7)
    assert all(len(r) == 88 for r in recs)

    def w32(r):
        return np.frombuffer(r, "<u4").copy()

    kinds = ("unsorted", "past", "size", "nr0", "nrbig")
    spots = [64 * t + lane for t in (2, 40, 130) for lane in (0, 13, 45, 46, 57, 58, 63)]
    for k, at in enumerate(spots):
        w = w32(recs[at])
        kind = kinds[k % len(kinds)]
        if kind == "unsorted":
            w[1], w[2] = w[2], w[1]
        elif kind == "past":
            w[7] = 4090 | (8 << 16)
        elif kind == "size":
            w[3] = (w[3] & 0xFFFF) | (12 << 16)
        elif kind == "nr0":
            w[0] = 0
        else:
            w[0] = 2049
        recs[at] = w.tobytes()
    ro, _ = _stream(recs)
    # offsets out of order: record i ends before it starts; record i + 1 then starts in the
    # last payload bytes of record i - 1 (set to 0xFF: a run count past 2048)
    for at in (64 * 60 + 45, 64 * 61 + 57, 64 * 62 + 63, 64 * 64 + 20):
        recs[at - 1] = recs[at - 1][:-8] + b"\xff" * 8
        ro[at + 1] = ro[at] - np.uint64(8)
    rep, ro, data, want, bad, ids = _case(recs, 48, ro=ro)
    assert bad == len(spots) + 2 * 4
    return rep, ro, data, want, bad, ids


def _apply_and_compare(variant, case):
    rep, ro, data, want, bad, ids = case
    n = len(rep)
    assert len(ro) - 1 == n and n > LONG
    L = _lib.load()
    assert L.gdsm_tune(b"apply_variant", variant) == 0
    try:
        with ga.Context(n) as c:
            c.upload("replica", rep)
            r = Runs.from_host(c, HostRuns(ro, data))
            c.apply(r, "replica", None if ids is None else c.ids(ids))
            if bad:
                with pytest.raises(GdsmError) as ei:
                    c.sync()
                assert ei.value.errno == 22
            else:
                c.sync()
            got = c.download("replica")
            diffp = np.flatnonzero((got != want).any(axis=1))
            assert len(diffp) == 0, diffp[:10]
    finally:
        L.gdsm_tune(b"apply_variant", 0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("permuted", (False, True))
@pytest.mark.parametrize("n", (LONG + 1, LONG + 64))
def test_plain_long_list(n, permuted, variant):
    """Uniform 1 % word writes, the smallest long list (a last task of one record) and one of
    whole tasks, by position and through a permuted page list."""
    _apply_and_compare(variant, _plain(n, permuted))


@pytest.mark.parametrize("variant", VARIANTS)
def test_window_edges(variant):
    """Tasks of exactly one window, one window + 4 B and two windows + 4 B (4 and 5 KiB
    windows), a fully rewritten page and a GDSM_MAX_RECORD record among sparse ones, a task of 64
    empty records."""
    _apply_and_compare(variant, _window_edges())


@pytest.mark.parametrize("variant", VARIANTS)
def test_partial_runs(variant):
    """Runs of 1..17 B at every offset mod 16, runs ending on the page's last byte, several runs
    in one 16-B chunk, 8 B at offset 4, batches of partial runs only."""
    _apply_and_compare(variant, _partial_runs())


@pytest.mark.parametrize("variant", VARIANTS)
def test_long_run_among_word_runs(variant):
    """Batches with a run of more than two chunks among word runs: the chunk map spreads the
    chunks over the wave."""
    _apply_and_compare(variant, _long_among_words())


@pytest.mark.parametrize("variant", VARIANTS)
def test_malformed_between_good(variant):
    """Unsorted runs, a run past the page, a size that does not add up, a run count of 0 or past
    2048, and stream offsets out of order, on window and task boundaries: only the oracle's
    well-formed records are written, and the sync reports -EINVAL."""
    _apply_and_compare(variant, _malformed())
