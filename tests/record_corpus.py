"""A seeded corpus of SPEC §3 records, canonical ones and malformed mutants of them, and the lists
the GPU validation tests feed to the device (tests/test_gpu_record_validation.py). Helper module,
checked on the CPU by tests/test_record_corpus.py.

Base records come from oracle.diff_pages of seeded twin/current pages, so they are canonical. Every
mutant is one record (uint8) with a class name. What apply makes of a record, the verdict (0 or
-22) and the resulting page, is oracle.apply's answer on a one-record stream over a copy of the
page's initial contents; nothing here is computed by the device library.

Safety of the lists (check_safety): a validator that wrongly accepts a mutant must produce a wrong
byte, never an access outside an allocation:
  * reach(rec) = 4 + 4 * min(nruns, 2048) + the sum of the `len` fields of those headers that lie
    inside the record is the farthest a validator or a payload read can get from the record's
    start; no record's start + reach passes the end of the list's data (zero padding, or valid
    tail records where the data may not be padded);
  * every page a corpus record targets is followed by GUARD_PAGES pages that no record of the list
    targets (a header can name at most 0xFFFF + 0xFFFF = 131070 B past the page start);
  * rec_off starts at 0, never decreases, is 4-aligned; page ids are in range and unique.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import oracle

PAGE = 4096
MAX_RUNS = 2048
GUARD_PAGES = 32
SEED = 0x5EC04
RUN_COUNTS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 500, 2047, 2048)

# class names
BASE = "base"
LEN0 = "len0"
PAST_4097 = "past_end_4097"
PAST_4095_2 = "past_end_off4095_len2"
REACH_FFFF = "off_ffff_len_ffff"
SWAPPED = "swapped"
OVERLAP1 = "overlap_one_byte"
ABUTTING = "abutting"
NRUNS_0 = "nruns_0"
NRUNS_2049 = "nruns_2049"
NRUNS_80000000 = "nruns_80000000"
NRUNS_FFFFFFFF = "nruns_ffffffff"
NRUNS_SIZE4 = "nruns_headers_end_at_size_plus_4"
SIZE_PLUS4 = "size_plus_4"
SIZE_MINUS4 = "size_minus_4"
LEN1_SAME = "len_plus_1_same_roundup"
LEN1_CHANGES = "len_plus_1_roundup_changes"
OVER_12292_1 = "oversized_12292_nruns_1"
OVER_16384_1 = "oversized_16384_nruns_1"
OVER_12292_2048 = "oversized_12292_nruns_2048"
OVER_16384_2048 = "oversized_16384_nruns_2048"

ACCEPTED_CLASSES = (BASE, ABUTTING, LEN1_SAME)
REFUSED_CLASSES = (LEN0, PAST_4097, PAST_4095_2, REACH_FFFF, SWAPPED, OVERLAP1, NRUNS_0, NRUNS_2049,
                   NRUNS_80000000, NRUNS_FFFFFFFF, NRUNS_SIZE4, SIZE_PLUS4, SIZE_MINUS4,
                   LEN1_CHANGES, OVER_12292_1, OVER_16384_1, OVER_12292_2048, OVER_16384_2048)
LAST = "last"


@dataclass
class Entry:
    """One corpus record: `init` is its page before the apply, `page` after it (the oracle's)."""
    cls: str
    base: str
    note: str
    rec: np.ndarray
    init: np.ndarray
    verdict: int
    page: np.ndarray

    @property
    def accepted(self) -> bool:
        return self.verdict == 0

    @property
    def name(self) -> str:
        return f"{self.cls}[{self.base}{',' + self.note if self.note else ''}]"


# ---------------------------------------------------------------------------- records
def words(rec) -> np.ndarray:
    return np.frombuffer(np.ascontiguousarray(rec, np.uint8).tobytes(), "<u4")


def parse(rec):
    """(off, len, payload) of a well-formed record: int64 arrays and the unpadded payload."""
    w = words(rec)
    nr = int(w[0])
    hdr = w[1:1 + nr].astype(np.int64)
    off, ln = hdr & 0xFFFF, hdr >> 16
    p = 4 + 4 * nr
    return off, ln, np.asarray(rec[p:p + int(ln.sum())], np.uint8).copy()


def build(off, ln, pay, nruns=None) -> np.ndarray:
    """The record with these headers and this payload, as given: nothing is checked."""
    hdr = (np.asarray(off, np.int64) | (np.asarray(ln, np.int64) << 16)).astype("<u4")
    head = np.array([len(hdr) if nruns is None else nruns], "<u4").tobytes() + hdr.tobytes()
    pay = np.asarray(pay, np.uint8).tobytes()
    return np.frombuffer(head + pay + b"\0" * (-len(pay) % 4), np.uint8).copy()


def with_header(rec, r, off, ln) -> np.ndarray:
    """rec with header r replaced; every other byte, the payload included, stays."""
    out = np.array(rec, np.uint8)
    out[4 + 4 * r:8 + 4 * r] = np.frombuffer(np.array([off | (ln << 16)], "<u4").tobytes(), np.uint8)
    return out


def with_nruns(rec, nruns) -> np.ndarray:
    out = np.array(rec, np.uint8)
    out[:4] = np.frombuffer(np.array([nruns], "<u4").tobytes(), np.uint8)
    return out


def reach(rec) -> int:
    """The farthest byte, from the record's start, that a validator trusting `nruns` (bounded by
    2048) and every header inside the record could read."""
    size = len(rec)
    if size < 4:
        return size
    w = words(rec)
    m = min(int(w[0]), MAX_RUNS)
    inside = min(m, size // 4 - 1)
    return max(size, 4 + 4 * m + int((w[1:1 + inside] >> 16).sum(dtype=np.uint64)))


def overhang(rec) -> int:
    return reach(rec) - len(rec)


def _layout(k, rng):
    """k runs with at least one unchanged byte between neighbours."""
    max_len = 1 if k > 1000 else max(1, min(24, (PAGE - k) // k - 1))
    ln = rng.integers(1, max_len + 1, k)
    free = PAGE - int(ln.sum()) - (k - 1)
    assert free >= 0
    gaps = rng.multinomial(free, np.full(k + 1, 1.0 / (k + 1)))
    gaps[1:k] += 1
    off = np.cumsum(gaps[:k]) + np.concatenate([[0], np.cumsum(ln)[:-1]])
    return [(int(o), int(l)) for o, l in zip(off, ln)]


def _pages(runs, rng):
    twin = rng.integers(1, 256, PAGE, dtype=np.uint8)  # no zero byte: a stray zero store shows
    cur = twin.copy()
    for o, l in runs:
        cur[o:o + l] ^= rng.integers(1, 256, l, dtype=np.uint8)
    return twin, cur


@functools.lru_cache(maxsize=None)
def bases():
    """{name: (twin, current, record)}; the record is oracle.diff_pages' of the two pages."""
    rng = np.random.default_rng(SEED)
    shapes = {f"runs{k}": _layout(k, rng) for k in RUN_COUNTS}
    shapes["whole"] = [(0, PAGE)]
    shapes["long_odd_a"] = [(1, 999), (1003, 17), (1031, 2001), (3333, 763)]
    shapes["long_odd_b"] = [(4096 - 601, 601)]
    shapes["long_odd_c"] = [(7, 33), (41, 1), (43, 4053)]
    shapes["long_odd_d"] = [(15, 17), (33, 31), (65, 63), (129, 127), (257, 255), (513, 1023)]
    out = {}
    for name, runs in shapes.items():
        twin, cur = _pages(runs, rng)
        ro, data = oracle.diff_pages(twin[None], cur[None])
        rec = data[:int(ro[1])].copy()
        assert int(words(rec)[0]) == len(runs)
        out[name] = (twin, cur, rec)
    assert len(out["runs2048"][2]) == 10244 and len(out["whole"][2]) == 4104
    return out


def _runs_of(name) -> int:
    return int(words(bases()[name][2])[0])


def _for_run(r, least=1):
    """The bases run r is taken from: the one with the fewest runs that has it, and three large
    ones, so that r is met both as the record's last run and in the middle of a step."""
    names = sorted((n for n in bases() if n.startswith("runs")), key=_runs_of)
    have = [n for n in names if _runs_of(n) > r and _runs_of(n) >= least]
    return list(dict.fromkeys(have[:1] + [n for n in ("runs129", "runs500", "runs2048") if n in have]))


_LAST_BASES = ("runs1", "runs2", "runs16", "runs17", "runs33", "runs64", "runs65", "runs2047",
               "whole", "long_odd_a", "long_odd_d")


def _targets(rs, least=1):
    """[(base name, run index, note)] for run indices rs (LAST = every base's last run)."""
    out = []
    for r in rs:
        if r == LAST:
            out += [(n, _runs_of(n) - 1, "last") for n in _LAST_BASES if _runs_of(n) >= least]
        else:
            out += [(n, r, f"r{r}") for n in _for_run(r, least)]
    return out


def _mutants():
    """[(class, base name, note, record)]"""
    rng = np.random.default_rng(SEED + 1)
    B = bases()
    out = []

    def add(cls, name, note, rec):
        assert len(rec) % 4 == 0
        out.append((cls, name, note, np.ascontiguousarray(rec, np.uint8)))

    # a run of length 0 (its payload bytes taken out: the length is the only defect)
    for name, r, note in _targets((0, 15, 16, 17, 63, 64, 65, LAST)):
        off, ln, pay = parse(B[name][2])
        p0 = int(ln[:r].sum())
        pay = np.concatenate([pay[:p0], pay[p0 + int(ln[r]):]])
        ln[r] = 0
        add(LEN0, name, note, build(off, ln, pay))
    # a run past the page end
    for name in _LAST_BASES:
        off, ln, pay = parse(B[name][2])
        more = PAGE + 1 - int(off[-1] + ln[-1])
        l2 = ln.copy()
        l2[-1] += more
        add(PAST_4097, name, "", build(off, l2, np.concatenate([pay, rng.integers(1, 256, more, dtype=np.uint8)])))
        if len(off) == 1 or off[-2] + ln[-2] <= PAGE - 1:
            o3, l3 = off.copy(), ln.copy()
            o3[-1], l3[-1] = PAGE - 1, 2
            p3 = np.concatenate([pay[:int(ln[:-1].sum())], rng.integers(1, 256, 2, dtype=np.uint8)])
            add(PAST_4095_2, name, "", build(o3, l3, p3))
    for name, r, note in _targets((0, 16, 64, LAST)):
        add(REACH_FFFF, name, note, with_header(B[name][2], r, 0xFFFF, 0xFFFF))  # the size stays
    # unsorted: headers r-1 and r swapped (the size stays consistent)
    for name, r, note in _targets((1, 16, 17, 64, 65, LAST), least=2):
        off, ln, pay = parse(B[name][2])
        off[[r - 1, r]], ln[[r - 1, r]] = off[[r, r - 1]], ln[[r, r - 1]]
        add(SWAPPED, name, note, build(off, ln, pay))
    # run r starts one byte inside run r-1 / exactly at its end (lengths, payload and size stay)
    for name, r, note in _targets((1, 16, 64, 128, LAST), least=2):
        off, ln, pay = parse(B[name][2])
        end = int(off[r - 1] + ln[r - 1])
        add(OVERLAP1, name, note, with_header(B[name][2], r, end - 1, int(ln[r])))
        add(ABUTTING, name, note, with_header(B[name][2], r, end, int(ln[r])))
    # nruns
    for name in ("runs1", "runs2", "runs17", "runs65", "runs500", "runs2047", "runs2048", "whole",
                 "long_odd_a"):
        rec = B[name][2]
        for cls, v in ((NRUNS_0, 0), (NRUNS_2049, 2049), (NRUNS_80000000, 0x80000000),
                       (NRUNS_FFFFFFFF, 0xFFFFFFFF)):
            add(cls, name, "", with_nruns(rec, v))
        if len(rec) // 4 <= MAX_RUNS:  # 4 + 4 * nruns == size + 4, nruns itself in range
            add(NRUNS_SIZE4, name, "", with_nruns(rec, len(rec) // 4))
    # the size against the headers
    for name in ("runs1", "runs2", "runs16", "runs17", "runs64", "runs65", "runs129", "runs2048",
                 "whole", "long_odd_c"):
        rec = B[name][2]
        add(SIZE_PLUS4, name, "", np.concatenate([rec, np.zeros(4, np.uint8)]))
        add(SIZE_MINUS4, name, "", rec[:-4])
    # one run a byte longer, header only: with the same round-up the size still matches and the
    # payload of every later run shifts by a byte; otherwise the size no longer matches
    for name, r, note in _targets((0, 16, 64, LAST)):
        off, ln, pay = parse(B[name][2])
        nxt = int(off[r + 1]) if r + 1 < len(off) else PAGE
        if off[r] + ln[r] + 1 > nxt:
            continue
        same = int(ln.sum()) % 4 != 0
        add(LEN1_SAME if same else LEN1_CHANGES, name, note,
            with_header(B[name][2], r, int(off[r]), int(ln[r]) + 1))
    return out


def _oversized():
    for size, c1, c2048 in ((12292, OVER_12292_1, OVER_12292_2048), (16384, OVER_16384_1, OVER_16384_2048)):
        one = np.zeros(size, np.uint8)
        one[:8] = np.frombuffer(np.array([1, 100 | (8 << 16)], "<u4").tobytes(), np.uint8)
        many = np.zeros(size, np.uint8)
        hdr = np.array([MAX_RUNS] + [2 * i | (1 << 16) for i in range(MAX_RUNS)], "<u4")
        many[:4 + 4 * MAX_RUNS] = np.frombuffer(hdr.tobytes(), np.uint8)
        yield c1, one
        yield c2048, many


def verdict_and_page(rec, init):
    """oracle.apply of the one-record stream `rec` over a copy of `init`."""
    page = np.array(init, np.uint8).reshape(1, PAGE)
    rc = oracle.apply(page, np.array([0, len(rec)], np.uint64), rec)
    return int(rc), page[0]


@functools.lru_cache(maxsize=None)
def corpus():
    """Every base record and every mutant, as a tuple of Entry."""
    rng = np.random.default_rng(SEED + 2)
    out = []

    def entry(cls, base, note, rec, init):
        rc, page = verdict_and_page(rec, init)
        assert rc in (0, -22)
        out.append(Entry(cls, base, note, rec, init, rc, page))

    for name, (twin, cur, rec) in bases().items():
        entry(BASE, name, "", rec, twin)
    for cls, name, note, rec in _mutants():
        entry(cls, name, note, rec, bases()[name][0])
    for cls, rec in _oversized():
        entry(cls, "none", "", rec, rng.integers(1, 256, PAGE, dtype=np.uint8))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ordered():
    """The corpus in list order: a small refused record right after every record that is larger
    than a staging window (4104 B, 10244 B), the rest as built."""
    c = list(corpus())
    small = [e for e in c if not e.accepted and len(e.rec) <= 64]
    big = [e for e in c if e.accepted and len(e.rec) in (4104, 10244)]
    assert len(small) >= len(big) >= 2
    after = {id(b): s for b, s in zip(big, small)}
    moved = {id(s) for s in after.values()}
    out = []
    for e in c:
        if id(e) in moved:
            continue
        out.append(e)
        if id(e) in after:
            out.append(after[id(e)])
    assert len(out) == len(c)
    return tuple(out)


# ---------------------------------------------------------------------------- fillers
EMPTY = np.zeros(0, np.uint8)


def filler_word(rng) -> np.ndarray:
    """A small valid word edit."""
    return build([int(rng.integers(0, PAGE // 8)) * 8], [8], rng.integers(1, 256, 8, dtype=np.uint8))


def filler_sized(rng, size) -> np.ndarray:
    """A valid record of `size` bytes (16 <= size <= 4104, a multiple of 4): one run."""
    ln = size - 8
    return build([int(rng.integers(0, PAGE - ln + 1))], [ln], rng.integers(1, 256, ln, dtype=np.uint8))


def filler_big(rng) -> np.ndarray:
    """The largest canonical record: 2048 one-byte runs, 10244 B."""
    return build(np.arange(0, PAGE, 2), np.ones(MAX_RUNS, np.int64), rng.integers(1, 256, MAX_RUNS, dtype=np.uint8))


# ---------------------------------------------------------------------------- lists
class RecordList:
    """One device list. items: Entry (a corpus record) or a uint8 array (a valid filler record).
    The k-th corpus record targets page 33 k, followed by its guard pages; fillers take the pages
    after the corpus region, one each. pad: zero bytes after the stream as far as every record's
    reach needs; without it (a wire frame's data cannot be padded) the items themselves must
    provide the room (see with_tail)."""

    def __init__(self, items, pad=True):
        self.items = list(items)
        self.n = len(self.items)
        recs = [it.rec if isinstance(it, Entry) else np.asarray(it, np.uint8) for it in self.items]
        self.rec_off = np.zeros(self.n + 1, np.uint64)
        self.rec_off[1:] = np.cumsum([len(r) for r in recs])
        self.total = int(self.rec_off[-1])
        self.slots = []    # (list index, page, Entry)
        self.fillers = []  # (list index, page)
        n_corpus = sum(isinstance(it, Entry) for it in self.items)
        self.corpus_pages = (GUARD_PAGES + 1) * n_corpus
        self.ids = np.zeros(self.n, np.uint32)
        for i, it in enumerate(self.items):
            if isinstance(it, Entry):
                self.ids[i] = (GUARD_PAGES + 1) * len(self.slots)
                self.slots.append((i, int(self.ids[i]), it))
            else:
                self.ids[i] = self.corpus_pages + len(self.fillers)
                self.fillers.append((i, int(self.ids[i])))
        self.n_pages = self.corpus_pages + len(self.fillers) + 1  # (the last page: never listed)
        self.need = max([self.total] + [int(self.rec_off[i]) + reach(r) for i, r in enumerate(recs)])
        self.data = np.zeros(self.need if pad else self.total, np.uint8)
        self.data[:self.total] = np.concatenate(recs) if recs else EMPTY
        self.refused = any(not e.accepted for _, _, e in self.slots)

    def stream(self):
        """(rec_off, data) with the padding: a stream whose capacity is the padded length."""
        return self.rec_off, self.data

    def arena(self, seed):
        """(initial arena, arena the oracle expects after the apply), n_pages x 4096 each: seeded
        non-zero bytes, every corpus page its record's initial contents."""
        rng = np.random.default_rng(seed)
        init = rng.integers(1, 256, (self.n_pages, PAGE), dtype=np.uint8)
        for _, page, e in self.slots:
            init[page] = e.init
        want = init.copy()
        for _, page, e in self.slots:
            want[page] = e.page
        if self.fillers:
            idx = [i for i, _ in self.fillers]
            recs = [np.asarray(self.items[i], np.uint8) for i in idx]
            ro = np.zeros(len(recs) + 1, np.uint64)
            ro[1:] = np.cumsum([len(r) for r in recs])
            data = np.concatenate(recs)
            rc = oracle.apply(want, ro, data, ids=np.array([p for _, p in self.fillers], np.uint32))
            assert rc == 0, "a filler record must be valid"
        return init, want


def check_safety(lst: RecordList, alloc=None):
    """Asserts the three rules of this module's docstring for a list; alloc = the bytes of the
    device data allocation (default: the list's padded data)."""
    alloc = len(lst.data) if alloc is None else alloc
    ro = lst.rec_off.astype(np.int64)
    assert ro[0] == 0 and (np.diff(ro) >= 0).all() and not (ro & 3).any()
    assert len(np.unique(lst.ids)) == lst.n and (lst.ids < lst.n_pages).all()
    for i, it in enumerate(lst.items):
        rec = it.rec if isinstance(it, Entry) else it
        assert int(ro[i]) + reach(rec) <= alloc, (i, reach(rec))
    targeted = np.zeros(lst.n_pages + GUARD_PAGES, bool)
    targeted[lst.ids] = True
    for _, page, _ in lst.slots:
        assert page + GUARD_PAGES < lst.n_pages
        assert not targeted[page + 1:page + 1 + GUARD_PAGES].any(), page


def with_tail(items, rng):
    """items followed by as many largest valid records as keep every record's reach inside the
    stream itself: for lists whose data cannot be zero-padded (the data of a wire frame)."""
    items = list(items)
    while True:
        lst = RecordList(items, pad=False)
        if lst.need <= lst.total:
            return lst
        items += [filler_big(rng) for _ in range((lst.need - lst.total + 10243) // 10244)]


WIRE_OVERHANG = 1 << 17  # records that reach farther are left out of wire frames


def wire_subset(entries):
    """The entries a wire frame can hold safely: a frame's data ends the device buffer, so what a
    record could reach must be covered by the valid records behind it (with_tail)."""
    return [e for e in entries if overhang(e.rec) <= WIRE_OVERHANG]


def tiny_list() -> RecordList:
    """The corpus as one list (at most 4096 records)."""
    return RecordList(ordered())


def short_list(n=5000) -> RecordList:
    """The corpus padded with empty filler records to n records (4097..16384)."""
    c = list(ordered())
    return RecordList(c + [EMPTY] * (n - len(c)))


LONG_FRONTS = (0, 1, 63)
LONG_N = 16384 + 64 + 7


def long_items(entries, rng, fronts=LONG_FRONTS, n=LONG_N):
    """The entries once per front f, each copy starting at a list index that is f modulo 64 with at
    least f filler records before it, then fillers up to n records (> 16384, not a multiple of 64).
    Fillers are empty, small word edits or a few hundred bytes, in seeded random order, so that the
    staged windows break at different corpus records in every copy."""
    def filler():
        k = int(rng.integers(0, 8))
        return EMPTY if k < 2 else filler_word(rng) if k < 7 else filler_sized(rng, 4 * int(rng.integers(16, 200)))

    items, starts = [], []
    for f in fronts:
        items += [filler() for _ in range(f)]
        while len(items) % 64 != f:
            items.append(filler())
        starts.append(len(items))
        items += list(entries)
    assert len(items) < n
    items += [filler() for _ in range(n - len(items))]
    return items, starts


@functools.lru_cache(maxsize=None)
def long_list() -> RecordList:
    items, starts = long_items(ordered(), np.random.default_rng(SEED + 3))
    lst = RecordList(items)
    lst.starts = starts
    return lst


def windows(rec_off, per_task, win):
    """The staging of apply_kernel / apply_flat_kernel restated: [(first, end, staged)] over list
    indices; staged False = the record alone exceeds the window (read from global memory)."""
    ro = [int(x) for x in rec_off]
    n = len(ro) - 1
    out = []
    for a in range(0, n, per_task):
        cnt = min(per_task, n - a)
        j = 0
        while j < cnt:
            k = j
            while k < cnt and ro[a + k + 1] - ro[a + j] <= win:
                k += 1
            if k == j:
                out.append((a + j, a + j + 1, False))
                j += 1
            else:
                out.append((a + j, a + k, True))
                j = k
    return out
