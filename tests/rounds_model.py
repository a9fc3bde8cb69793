"""Host model of gdsm_rounds' page-data side (include/gdsm.h, "DSM rounds on the device"), in plain
numpy and the C oracle's diff, independent of the kernels: what every round leaves in TWIN,
CURRENT and REPLICA and the stream it writes. Also the trace generators the GPU test replays
(tests/test_gpu_rounds_data.py; tests/test_rounds_model.py checks the generators and the model on
the CPU) and the helper that issues a trace's first k rounds on the device.

A trace: the initial TWIN / CURRENT / REPLICA images (n_pages x 4096 u8), a source byte buffer, and
per round the list entries `ids` (pages of TWIN / CURRENT) and `home` (pages of REPLICA) and the
round's writes as descriptors (dst byte offset in CURRENT, src byte offset in the source buffer,
bytes). A round, in order: the descriptors are laid onto CURRENT; the listed pages are diffed
(TWIN against CURRENT) into the round's stream; the changed bytes of entry i go to page home[i] of
REPLICA; TWIN := CURRENT for the listed pages."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from oracle import oracle

PAGE = 4096
MAX_RECORD = 10244      # include/gdsm.h GDSM_MAX_RECORD
MAX_ROUND_PAGES = 2048  # include/gdsm.h: pages per round


@dataclass
class Round:
    ids: np.ndarray                       # u32: pages of TWIN / CURRENT
    home: np.ndarray                      # u32: entry i's page of REPLICA
    desc: List[Tuple[int, int, int]]      # (dst byte offset in CURRENT, src offset, bytes)


@dataclass
class Trace:
    name: str
    twin: np.ndarray
    cur: np.ndarray
    rep: np.ndarray
    src: np.ndarray
    rounds: List[Round] = field(default_factory=list)

    @property
    def n_pages(self) -> int:
        return self.twin.shape[0]


@dataclass
class State:
    """The arenas after a round and that round's stream."""
    twin: np.ndarray
    cur: np.ndarray
    rep: np.ndarray
    rec_off: np.ndarray
    data: np.ndarray


def replay(trace: Trace, k: Optional[int] = None) -> Iterator[State]:
    """Replays rounds 0..k-1 (all by default), yielding after each round the arenas (the live
    arrays, valid until the next step: copy what has to last) and that round's stream."""
    twin, cur, rep = trace.twin.copy(), trace.cur.copy(), trace.rep.copy()
    flat = cur.reshape(-1)
    for rd in trace.rounds[:len(trace.rounds) if k is None else k]:
        for dst, so, nb in rd.desc:                                   # 1: the round's writes
            flat[dst:dst + nb] = trace.src[so:so + nb]
        ids = np.asarray(rd.ids, np.int64)
        if len(ids):
            rec_off, data = oracle.diff_pages(twin, cur, rd.ids)      # 2: the round's stream
        else:
            rec_off, data = np.zeros(1, np.uint64), np.zeros(0, np.uint8)  # 5: an empty round
        for i, p in enumerate(ids):                                   # 3: the home apply
            m = twin[p] != cur[p]
            rep[int(rd.home[i])][m] = cur[p][m]
        twin[ids] = cur[ids]                                          # 4: the re-twin
        yield State(twin, cur, rep, rec_off, data)


def model(trace: Trace, k: int) -> State:
    """TWIN, CURRENT, REPLICA after round k - 1 and that round's (rec_off, data), 1 <= k."""
    assert 1 <= k <= len(trace.rounds)
    st = None
    for st in replay(trace, k):
        pass
    return State(st.twin.copy(), st.cur.copy(), st.rep.copy(), st.rec_off, st.data)


# ---------------------------------------------------------------------------- trace generators
def shifted_perm(rng, n: int) -> np.ndarray:
    """A permutation of 0..n-1 without fixed points (one cycle through a random order), n >= 2."""
    order = rng.permutation(n)
    perm = np.empty(n, np.int64)
    perm[order] = np.roll(order, -1)
    return perm


class TraceBuilder:
    """Builds a trace round by round. write() makes one descriptor whose source bytes are the
    destination's bytes at that point of the trace with the masked bytes XOR-ed by non-zero
    values, so a byte changes exactly where the mask says."""

    def __init__(self, name: str, twin, cur, rep, seed: int):
        self.rng = np.random.default_rng(seed)
        self.t = Trace(name, np.array(twin, np.uint8), np.array(cur, np.uint8),
                       np.array(rep, np.uint8), np.zeros(0, np.uint8))
        self.now = self.t.cur.copy().reshape(-1)  # CURRENT as the writes so far leave it
        self.src: List[np.ndarray] = []
        self.src_len = 0
        self.desc: List[Tuple[int, int, int]] = []

    @classmethod
    def fresh(cls, name: str, n_pages: int, seed: int, dirty: Sequence[int] = ()):
        """Random TWIN, CURRENT = TWIN but for sparse changes on the `dirty` pages, and an
        unrelated random REPLICA (so a home apply that stores more than the changed bytes shows)."""
        rng = np.random.default_rng(seed ^ 0x5EED)
        twin = rng.integers(0, 256, (n_pages, PAGE), dtype=np.uint8)
        cur = twin.copy()
        for p in dirty:
            m = rng.random(PAGE) < 0.01
            m[rng.integers(0, PAGE)] = True
            cur[p, m] ^= rng.integers(1, 256, int(m.sum()), dtype=np.uint8)
        rep = rng.integers(0, 256, (n_pages, PAGE), dtype=np.uint8)
        return cls(name, twin, cur, rep, seed)

    def write(self, dst: int, nbytes: int, mask=None, pad: bool = False):
        """One descriptor of `nbytes` at byte `dst` of CURRENT; mask: bool[nbytes] or the byte
        positions to change (None: none, the source equals the destination). pad: 8 B of filler
        before the source, so sources are not all 16-B aligned with their destinations."""
        assert dst % 8 == 0 and nbytes % 8 == 0
        m = np.zeros(nbytes, bool)
        if mask is not None:
            mk = np.asarray(mask)
            if mk.dtype == bool:
                m[:] = mk
            else:
                m[mk] = True
        x = np.where(m, self.rng.integers(1, 256, nbytes, dtype=np.uint8), 0).astype(np.uint8)
        new = self.now[dst:dst + nbytes] ^ x
        if pad:
            self.src.append(np.full(8, 0xA5, np.uint8))
            self.src_len += 8
        self.desc.append((dst, self.src_len, nbytes))
        self.src.append(new)
        self.src_len += nbytes
        self.now[dst:dst + nbytes] = new

    def release(self, ids, home):
        self.t.rounds.append(Round(np.array(ids, np.uint32).reshape(-1),
                                   np.array(home, np.uint32).reshape(-1), self.desc))
        self.desc = []

    def build(self) -> Trace:
        assert not self.desc
        self.t.src = np.concatenate(self.src) if self.src else np.zeros(8, np.uint8)
        return self.t


EDGES_PAGES = 24


def edges_home(p):
    """The edges trace's home page of view page p: a permutation without fixed points."""
    return (np.asarray(p, np.int64) * 7 + 5) % EDGES_PAGES


def edges_trace() -> Trace:
    """24 pages, 8 rounds of at most 6 pages: the edge cases of the fused row writes, of the
    diff's chunk / quarter / page edges and of the release's empty and clean entries."""
    P = PAGE
    b = TraceBuilder.fresh("edges", EDGES_PAGES, seed=101, dirty=(4, 20, 22, 23))
    H = edges_home
    # round 0: empty
    b.release([], [])
    # round 1
    #   page 3: released, no descriptor, no change; page 4: dirty before the call, no descriptor;
    #   pages 22 and 23: dirty before the call and never released
    b.write(9 * P + 512, 64)                                 # page 9: bytes equal to TWIN
    b.write(10 * P + 256, 0)                                 # page 10: bytes = 0,
    b.write(10 * P + 5 * 16 + 8, 8, [0, 3, 7], pad=True)     #   an upper half only,
    b.write(10 * P + 7 * 16, 8, [1, 2])                      #   a lower half only
    b.write(15 * P + 20 * 16 + 8, 16, [6, 7, 8, 9])          # page 15: upper half -> lower half
    for q, ln in ((0, 24), (1000, 48), (2040, 16), (4000, 96)):  # page 20 (dirty before): four
        b.write(20 * P + q, ln, b.rng.random(ln) < 0.5, pad=q == 1000)
    ids = [3, 9, 4, 10, 15, 20]
    b.release(ids, H(ids))
    # round 2: one descriptor over three released pages; page 11: runs across the quarter edges
    # (chunks 63/64, 127/128, 191/192) and the page's first and last bytes
    n3 = 24 + P + 40
    b.write(5 * P + P - 24, n3, b.rng.random(n3) < 0.3, pad=True)
    b.write(11 * P, 8, [0])
    for ch in (64, 128, 192):
        b.write(11 * P + ch * 16 - 8, 16, [6, 7, 8, 9])
    b.write(11 * P + P - 8, 8, [7])
    ids = [11, 7, 5, 6]
    b.release(ids, H(ids))
    # round 3: empty
    b.release([], [])
    # round 4: every byte of page 12; alternating bytes of page 13 (a record of GDSM_MAX_RECORD
    # bytes); view pages 1 and 2 with disjoint bytes to ONE home page
    b.write(12 * P, P, np.ones(P, bool))
    b.write(13 * P, P, np.arange(P) % 2 == 0, pad=True)
    b.write(1 * P, 2048, b.rng.random(2048) < 0.2)
    b.write(2 * P + 2048, 2048, b.rng.random(2048) < 0.2)
    ids = [12, 13, 1, 2]
    b.release(ids, [H(12), H(13), H(1), H(1)])
    # round 5: pages of rounds 1 and 4 again, in another order (another workgroup each)
    b.write(13 * P, P, np.arange(P) % 2 == 1)
    b.write(12 * P + 1024, 2048, b.rng.random(2048) < 0.4, pad=True)
    b.write(4 * P + 8, 8, [4])
    b.write(20 * P + 1000, 48, b.rng.random(48) < 0.5)
    ids = [20, 13, 9, 12, 4, 3]
    b.release(ids, H(ids))
    # round 6: pages of rounds 1 and 2 again
    for p in (10, 15, 11, 6):
        for q in sorted(b.rng.choice(P // 64, 3, replace=False)):
            b.write(p * P + int(q) * 64 + 8, 48, b.rng.random(48) < 0.1)
    ids = [6, 5, 10, 7, 15, 11]
    b.release(ids, H(ids))
    # round 7: empty
    b.release([], [])
    return b.build()


HANDOFF_PAGES, HANDOFF_IDS, HANDOFF_HOME = 8, (2, 5, 7), (6, 0, 3)


def handoff_trace(rounds: int = 300) -> Trace:
    """The same three pages and home pages released `rounds` times, the list rotated by one every
    round (so another workgroup releases each page). Round r writes the 8-B word next to round
    r - 1's and rewrites some bytes of that one (one 16-B descriptor): a stale TWIN read ships
    bytes that did not change in the round, a stale CURRENT or REPLICA read loses earlier ones."""
    b = TraceBuilder.fresh("hand-off", HANDOFF_PAGES, seed=202)
    for r in range(rounds):
        for j, p in enumerate(HANDOFF_IDS):
            w = r + 64 * j  # page j's word of this round: the pages work in different quarters
            new = b.rng.random(8) < 0.6
            new[b.rng.integers(0, 8)] = True
            if r == 0:
                b.write(p * PAGE + 8 * w, 8, new)
            else:
                old = np.zeros(8, bool)
                old[b.rng.integers(0, 8, 2)] = True
                b.write(p * PAGE + 8 * (w - 1), 16, np.concatenate([old, new]), pad=r % 3 == 0)
        k = r % 3
        b.release(np.roll(HANDOFF_IDS, -k), np.roll(HANDOFF_HOME, -k))
    return b.build()


def page_mask(rng, kind: int) -> np.ndarray:
    """The byte densities of test_gpu_pages._mixed_density_pages: clean, 0.3 %, 40 %, every byte,
    alternating bytes."""
    if kind == 1:
        return rng.random(PAGE) < 0.003
    if kind == 2:
        return rng.random(PAGE) < 0.4
    if kind == 3:
        return np.ones(PAGE, bool)
    if kind == 4:
        return np.arange(PAGE) % 2 == int(rng.integers(0, 2))
    return np.zeros(PAGE, bool)


def random_round(b: TraceBuilder, rng, ids, home):
    """One round releasing `ids` to `home`: each listed page gets 0-3 disjoint descriptors (or,
    for some pages changed in every or every other byte, one over the whole page) whose changed
    bytes follow page_mask."""
    for p in ids:
        kind = int(rng.integers(0, 5))
        m = page_mask(b.rng, kind)
        nd = int(rng.integers(0, 4))
        if nd and kind >= 3 and rng.random() < 0.5:
            b.write(int(p) * PAGE, PAGE, m, pad=bool(rng.integers(0, 2)))  # the whole page
            continue
        cuts = np.sort(rng.choice(PAGE // 8 + 1, 2 * nd, replace=False)) * 8
        for a, e in zip(cuts[0::2], cuts[1::2]):
            b.write(int(p) * PAGE + int(a), int(e - a), m[a:e], pad=bool(rng.integers(0, 2)))
    b.release(ids, home)


def sizes_trace(name: str, n_pages: int, sizes: Sequence[int], seed: int) -> Trace:
    """Rounds of sizes[r] distinct random pages (random_round); the home pages are a
    fixed-point-free permutation of the ids; one page in 16 is dirty before the first round."""
    rng = np.random.default_rng(seed)
    b = TraceBuilder.fresh(name, n_pages, seed,
                           dirty=rng.choice(n_pages, n_pages // 16, replace=False))
    perm = shifted_perm(rng, n_pages)
    for n in sizes:
        ids = rng.choice(n_pages, n, replace=False)
        random_round(b, rng, ids, perm[ids])
    return b.build()


SMALL_SIZES = (1, 32, 0, 17, 31, 2)
LARGE_SIZES = (1, 33, 0, 257, 32, 2048, 5, 256)


def sizes_small_trace() -> Trace:
    return sizes_trace("sizes-small", 64, SMALL_SIZES, seed=303)


def sizes_large_trace() -> Trace:
    return sizes_trace("sizes-large", 4096, LARGE_SIZES, seed=404)


# ------------------------------------------------------------------------ the API contract
def contract_violations(trace: Trace) -> List[str]:
    """Where a trace leaves gdsm_rounds' contract (empty: inside it): 8-B aligned descriptors,
    writes only on pages their round releases, no overlap within a round, each page listed at
    most once per round, at most 2048 pages per round, ids and home pages inside the arenas."""
    bad = []
    n = trace.n_pages
    for r, rd in enumerate(trace.rounds):
        ids = np.asarray(rd.ids, np.int64)
        if len(ids) != len(rd.home):
            bad.append(f"round {r}: {len(ids)} ids, {len(rd.home)} home pages")
        if len(ids) > MAX_ROUND_PAGES:
            bad.append(f"round {r}: {len(ids)} pages")
        if len(np.unique(ids)) != len(ids):
            bad.append(f"round {r}: a page listed twice")
        if (ids >= n).any() or (np.asarray(rd.home, np.int64) >= n).any():
            bad.append(f"round {r}: a page outside the arenas")
        words = np.zeros(n * PAGE // 8, np.int32)
        for dst, so, nb in rd.desc:
            if dst % 8 or so % 8 or nb % 8:
                bad.append(f"round {r}: descriptor {(dst, so, nb)} not 8-B aligned")
            if dst < 0 or dst + nb > n * PAGE or so < 0 or so + nb > len(trace.src):
                bad.append(f"round {r}: descriptor {(dst, so, nb)} out of range")
                continue
            words[dst // 8:(dst + nb) // 8] += 1
        if (words > 1).any():
            bad.append(f"round {r}: overlapping descriptors")
        pages = np.unique(np.flatnonzero(words) // (PAGE // 8))
        if not np.isin(pages, ids).all():
            bad.append(f"round {r}: a write outside the released pages")
    return bad


# ------------------------------------------------------------------------------ the device
@dataclass
class DeviceRun:
    twin: np.ndarray
    cur: np.ndarray
    rep: np.ndarray
    n: int               # runs.n after the call
    rec_off: np.ndarray  # n + 1
    data: np.ndarray     # rec_off[n] bytes


def device_arrays(data_ctx, trace: Trace, k: int, src_buf=None):
    """The first k rounds as gdsm_rounds takes them: (d_ids, d_home, id_off, d_desc, desc_off,
    d_src) with the descriptors as absolute addresses (CURRENT's arena + dst, the uploaded source
    buffer + off)."""
    rounds = trace.rounds[:k]
    ids = np.concatenate([r.ids for r in rounds] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    home = np.concatenate([r.home for r in rounds] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    id_off = np.zeros(k + 1, np.int64)
    id_off[1:] = np.cumsum([len(r.ids) for r in rounds])
    desc_off = np.zeros(k + 1, np.int64)
    desc_off[1:] = np.cumsum([len(r.desc) for r in rounds])
    d_src = src_buf or data_ctx.buffer(max(8, trace.src.nbytes)).upload(trace.src)
    base = data_ctx.arena_ptr("current")
    desc = np.array([d for r in rounds for d in r.desc], np.uint64).reshape(-1, 3)
    desc[:, 0] += np.uint64(base)
    desc[:, 1] += np.uint64(d_src.ptr)
    d_ids = data_ctx.buffer(max(4, ids.nbytes)).upload(ids)
    d_home = data_ctx.buffer(max(4, home.nbytes)).upload(home)
    d_desc = data_ctx.buffer(max(24, desc.nbytes)).upload(desc)
    return d_ids, d_home, id_off, d_desc, desc_off, d_src


def issue_rounds(data_ctx, pt_ctx, trace: Trace, k: int, runs, events: Sequence = ()):
    """gdsm_rounds of the trace's first k rounds on the two contexts (not synchronised), with
    `events` (one host u64 array per round; none: an all-empty event side). Returns the call's
    return code and the device buffers it reads (keep them until the sync); totals are [7]."""
    from gallocy_amd.gdsm import lib
    arr = device_arrays(data_ctx, trace, k)
    d_ids, d_home, id_off, d_desc, desc_off, _ = arr
    ev_off = np.zeros(k + 1, np.int64)
    ev = np.zeros(0, np.uint64)
    if len(events):
        assert len(events) == k
        ev = np.concatenate(list(events)).astype(np.uint64)
        ev_off[1:] = np.cumsum([len(e) for e in events])
    d_ev = pt_ctx.buffer(max(8, ev.nbytes))
    if len(ev):
        d_ev.upload(ev)
    d_tot = pt_ctx.buffer(80 * max(1, k))
    rc = lib().gdsm_rounds(data_ctx.handle, pt_ctx.handle, k, d_ev.ptr, ev_off.ctypes.data,
                           d_tot.ptr, d_ids.ptr, d_home.ptr, id_off.ctypes.data, d_desc.ptr,
                           desc_off.ctypes.data, C.byref(runs.s))
    return rc, (*arr, d_ev, d_tot)


def max_round(trace: Trace, k: int) -> int:
    return max([len(r.ids) for r in trace.rounds[:k]] + [0])


def download_run(data_ctx, runs) -> DeviceRun:
    h = runs.to_host()
    n = int(runs.n)
    return DeviceRun(data_ctx.download("twin"), data_ctx.download("current"),
                     data_ctx.download("replica"), n, h.rec_off[:n + 1], h.data)


def run_prefix(trace: Trace, k: int) -> DeviceRun:
    """The trace's first k rounds in one gdsm_rounds call on fresh contexts (the page-table side
    gets empty rounds); the three arenas and the stream the call leaves."""
    import gallocy_amd as ga
    from gallocy_amd.gdsm import check
    m = max(1, max_round(trace, k))
    with ga.Context(trace.n_pages) as data, ga.Context(4, arenas=()) as pt:
        pt.coh_init(2)
        data.upload("twin", trace.twin)
        data.upload("current", trace.cur)
        data.upload("replica", trace.rep)
        runs = ga.Runs(data, m, cap=m * MAX_RECORD)
        rc, _keep = issue_rounds(data, pt, trace, k, runs)
        check(rc, "gdsm_rounds")
        data.sync()
        pt.sync()
        out = download_run(data, runs)
        runs.free()
        return out
