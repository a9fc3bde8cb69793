"""gdsm_runs_split on the GPU (docs/SPEC.md §13) against the numpy model tests/split_model.py,
exactly (rec_off, data, ids, counts), every output in a canary-filled buffer of exactly the
capacity the call is told: record counts around the wave and the 256-record tile and past the
tile scan's first step, record sizes from empty to the largest, every alignment of a destination
against the source, both forms, the flag, the capacity guards, the refusals, the raw entry point,
and the chains split -> apply, split -> merge and scan -> diff -> split -> exchange."""
import ctypes as C
import errno
import threading

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import exchange
from gallocy_amd._lib import GdsmRuns
from gallocy_amd.gdsm import GdsmError, lib
from oracle import oracle
from tests import split_model as sm

pytestmark = pytest.mark.gpu

T = 256            # records per tile of the kernels (gdsm_launch.h kSplitTile)
CANARY32 = 0xDEADBEEF
CANARY64 = 0xDEADBEEFDEADBEEF
CANARY8 = 0xC3
CANARY_ALL = 0xFFFFFFFFFFFFFFFF  # a torch tensor filled with -1
PAD = 8            # canary entries behind every rec_off / ids output
PAD_BYTES = 64     # canary bytes behind every data output
SIZES = (0, 12, 16, 20, 4104, 10244)


def run_ranks(G, fn):
    """fn(rank) on G threads; re-raises the first failure."""
    errs = [None] * G

    def body(r):
        try:
            fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e
    th = [threading.Thread(target=body, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    for e in errs:
        if e is not None:
            raise e


@pytest.fixture(scope="module")
def ctx():
    c = ga.Context(16)
    yield c
    c.close()


def stream(sizes, seed=0):
    ro = np.zeros(len(sizes) + 1, np.uint64)
    ro[1:] = np.cumsum(np.asarray(sizes, np.uint64))
    data = np.random.default_rng(seed).integers(0, 256, int(ro[-1]), dtype=np.uint8)
    return ro, data


def mixed_sizes(rng, n, small=False):
    if small:
        return rng.choice(SIZES[:4], n)
    return rng.choice(SIZES, n, p=[0.2, 0.3, 0.2, 0.2, 0.05, 0.05])


class Dev:
    """The input stream and G canary-filled outputs on the device, and the checks of what a call
    left in them."""

    def __init__(self, ctx, ro, data, ids, dest, G, caps, ncaps, in_cap=None, want_ids=True):
        self.ctx, self.G, self.caps, self.ncaps = ctx, G, list(caps), list(ncaps)
        n = len(ro) - 1
        self.bufs = []
        self.in_cap = len(data) if in_cap is None else in_cap
        self.d_ro = self._buf(np.asarray(ro, np.uint64))
        self.d_data = self._buf(data if len(data) else np.zeros(16, np.uint8))
        self.d_ids = self._buf(np.asarray(ids, np.uint32)) if ids is not None and n else None
        self.d_dest = self._buf(np.asarray(dest, np.uint32) if n else np.zeros(1, np.uint32)) \
            if dest is not None else None
        self.inp = GdsmRuns(n=n, rec_off=self.d_ro.ptr, data=self.d_data.ptr, cap=self.in_cap,
                            n_cap=n)
        self.o_ro = [self._buf(np.full(ncaps[d] + 1 + PAD, CANARY64, np.uint64)) for d in range(G)]
        self.o_data = [self._buf(np.full(caps[d] + PAD_BYTES, CANARY8, np.uint8)) for d in range(G)]
        self.o_ids = [self._buf(np.full(ncaps[d] + PAD, CANARY32, np.uint32)) if want_ids else None
                      for d in range(G)]
        self.outs = (GdsmRuns * G)(*[GdsmRuns(n=77, rec_off=self.o_ro[d].ptr,
                                              data=self.o_data[d].ptr, cap=caps[d], n_cap=ncaps[d])
                                     for d in range(G)])
        self.idp = (C.c_void_p * G)(*[ctx._ptr(b) for b in self.o_ids])

    def _buf(self, arr):
        arr = np.ascontiguousarray(arr)
        b = self.ctx.buffer(max(16, arr.nbytes)).upload(arr)
        self.bufs.append(b)
        return b

    def call(self, per=0, flags=0):
        counts = np.full((self.G, 2), 0x5A5A5A5A, np.uint64)
        rc = lib().gdsm_runs_split(self.ctx.handle, C.byref(self.inp), self.ctx._ptr(self.d_ids),
                                   self.ctx._ptr(self.d_dest), per, self.G, self.outs, self.idp,
                                   counts.ctypes.data_as(C.POINTER(C.c_uint64)), flags)
        return rc, counts

    def check_buffers(self, outs, tag=""):
        """Every output buffer holds the guarded part of the model's output and canaries behind it;
        `outs` None: a refused input, only rec_off[0] = 0 was written."""
        for d in range(self.G):
            if outs is None:
                o, buf, ids = np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint32)
            else:
                o, buf, ids = sm.written(outs[d], self.caps[d], self.ncaps[d])
            want = np.full(self.ncaps[d] + 1 + PAD, CANARY64, np.uint64)
            want[:len(o)] = o
            got = self.o_ro[d].download(np.uint64, len(want))
            assert np.array_equal(got, want), (tag, d, "rec_off")
            want = np.full(self.caps[d] + PAD_BYTES, CANARY8, np.uint8)
            want[:len(buf)] = buf
            got = self.o_data[d].download(np.uint8, len(want))
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (tag, d, "data", bad[:8].tolist(), len(buf))
            if self.o_ids[d] is not None:
                want = np.full(self.ncaps[d] + PAD, CANARY32, np.uint32)
                want[:len(ids)] = ids
                got = self.o_ids[d].download(np.uint32, len(want))
                assert np.array_equal(got, want), (tag, d, "ids")

    def free(self):
        for b in self.bufs:
            b.free()


def check(ctx, ro, data, ids, dest, per, G, flags=0, tag="", want_ids=True):
    """One call with every capacity exactly what the model says is needed."""
    err, outs, counts = sm.split(ro, data, ids, dest, per, G, flags)
    assert err == 0, tag
    caps = [int(counts[d, 1]) for d in range(G)]
    ncaps = [int(counts[d, 0]) for d in range(G)]
    dev = Dev(ctx, ro, data, ids, dest, G, caps, ncaps, want_ids=want_ids)
    try:
        rc, got = dev.call(per, flags)
        assert rc == 0, (tag, rc)
        assert np.array_equal(got, counts), (tag, got.tolist(), counts.tolist())
        assert [dev.outs[d].n for d in range(G)] == ncaps, tag
        dev.check_buffers(outs, tag)
    finally:
        dev.free()
    return outs, counts


def masks(rng, n, G):
    return {"zero": np.zeros(n, np.uint32),
            "all": np.full(n, (1 << G) - 1, np.uint32),
            "one bit": (np.uint32(1) << rng.integers(0, G, n).astype(np.uint32)).astype(np.uint32),
            "random": rng.integers(0, 1 << G, n).astype(np.uint32)}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 4 * T + 3])
def test_split_equals_model(ctx, n):
    rng = np.random.default_rng(1000 + n)
    ro, data = stream(mixed_sizes(rng, n), seed=n)
    page_ids = np.sort(rng.choice(4 * n + 8, n, replace=False)).astype(np.uint32)
    k = 0
    for G in (1, 2, 8):
        for kind, dest in masks(rng, n, G).items():
            k += 1
            check(ctx, ro, data, page_ids if k % 3 else None, dest, 0, G, flags=k & 1,
                  tag=(G, kind), want_ids=k % 5 != 0)
        # home form: an uneven last block; ascending, unsorted and no ids
        per = -(-(4 * n + 8) // G) + (1 if G > 1 else 0)
        check(ctx, ro, data, page_ids, None, per, G, flags=0, tag=(G, "home ascending"))
        check(ctx, ro, data, rng.permutation(page_ids), None, per, G, flags=1,
              tag=(G, "home unsorted"))
        check(ctx, ro, data, None, None, -(-max(n, 1) // G), G, flags=0, tag=(G, "home no ids"))


def test_long_list_of_small_records(ctx):
    """274 tiles: the scan of the tile sums takes two steps of 256."""
    n = 70001
    rng = np.random.default_rng(151)
    ro, data = stream(mixed_sizes(rng, n, small=True), seed=151)
    _, counts = check(ctx, ro, data, None, rng.integers(0, 256, n).astype(np.uint32), 0, 8,
                      flags=1, tag="masks")
    assert 0.3 * n < int(counts[:, 0].min()) and int(counts[:, 0].max()) < 0.45 * n
    ids = rng.integers(0, 1000, n).astype(np.uint32)
    check(ctx, ro, data, ids, None, 334, 3, tag="homes")


def test_a_tile_of_the_largest_records_between_tiles_of_empties(ctx):
    sizes = [0] * T + [10244] * T + [0] * T
    ro, data = stream(sizes, seed=152)
    n = len(sizes)
    for flags in (0, 1):
        check(ctx, ro, data, None, np.full(n, 3, np.uint32), 0, 2, flags, tag=("all", flags))
        check(ctx, ro, data, None, None, 300, 3, flags, tag=("home", flags))
    # one large record next to a thousand small ones
    sizes = [12] * 1000 + [10244] + [12] * 1000
    ro, data = stream(sizes, seed=153)
    rng = np.random.default_rng(153)
    check(ctx, ro, data, None, rng.integers(0, 4, len(sizes)).astype(np.uint32), 0, 2)


def test_records_longer_than_a_span(ctx):
    """Records are opaque, so one may be longer than the copy's 16 KiB span: a 40 KiB record among
    small ones is copied by several workgroups, its middle span holding nothing else; and a stream
    that is one 100 KiB record."""
    rng = np.random.default_rng(155)
    sizes = [12] * 300 + [40960] + [20] * 300 + [16384, 16388] + [12] * 50
    ro, data = stream(sizes, seed=155)
    n = len(sizes)
    dest = rng.integers(1, 8, n).astype(np.uint32)
    dest[300] = 5
    check(ctx, ro, data, None, dest, 0, 3, tag="masks")
    check(ctx, ro, data, None, None, 250, 3, tag="homes")
    ro, data = stream([102400], seed=156)
    check(ctx, ro, data, None, np.array([3], np.uint32), 0, 2, tag="one record")


@pytest.mark.parametrize("shift", [0, 4, 8, 12])
def test_every_alignment_of_destination_against_source(ctx, shift):
    """Destination 1 gets `shift` bytes the others do not, so its offset against the source (and
    that of the 16 KiB input spans' edges in it) starts at `shift` mod 16; the sizes move every
    destination through all four residues."""
    rng = np.random.default_rng(160 + shift)
    sizes = np.concatenate([[shift], rng.choice([12, 16, 20, 36, 4104], 3000,
                                                p=[0.3, 0.25, 0.25, 0.15, 0.05])])
    ro, data = stream(sizes, seed=shift)
    n = len(sizes)
    dest = rng.integers(1, 8, n).astype(np.uint32)
    dest[0] = 2
    outs, _ = check(ctx, ro, data, None, dest, 0, 3, tag=shift)
    # the offsets of the records' copies against their sources cover every residue everywhere
    for d in range(3):
        sel = np.flatnonzero((dest >> d) & 1)
        rel = (outs[d][0][:-1].astype(np.int64) - ro[sel].astype(np.int64)) % 16
        assert set(rel.tolist()) == {0, 4, 8, 12}, d
    # all to one destination: source and destination aligned alike from the second record on
    check(ctx, ro, data, None, np.ones(n, np.uint32), 0, 1, tag=(shift, "copy"))


def real_stream(seed, Z, frac=0.5):
    rng = np.random.default_rng(seed)
    twin = rng.integers(0, 256, (Z, 4096), dtype=np.uint8)
    cur = twin.copy()
    for p in rng.choice(Z, int(Z * frac), replace=False):
        k = int(rng.integers(1, 80))
        cur[p, rng.integers(0, 4096, k)] ^= rng.integers(1, 256, k).astype(np.uint8)
    cur[3] ^= 0xFF
    cur[7, 0::2] ^= 0xFF  # the largest record
    return twin, cur


def test_a_real_diff_stream(ctx):
    twin, cur = real_stream(170, 300)
    ids = np.sort(np.random.default_rng(171).choice(300, 280, replace=False)).astype(np.uint32)
    ro, data = oracle.diff_pages(twin, cur, ids)
    rng = np.random.default_rng(172)
    check(ctx, ro, data, ids, rng.integers(0, 16, len(ids)).astype(np.uint32), 0, 4, flags=1)
    check(ctx, ro, data, ids, None, 100, 3)


def short_case():
    rng = np.random.default_rng(180)
    n = 700
    ro, data = stream(mixed_sizes(rng, n), seed=180)
    dest = rng.integers(1, 8, n).astype(np.uint32)
    err, outs, counts = sm.split(ro, data, None, dest, 0, 3)
    return ro, data, dest, outs, counts


@pytest.mark.parametrize("short", ["one record", "one dword", "six bytes"])
def test_capacity_short_gives_enospc_and_guarded_writes(ctx, short):
    ro, data, dest, outs, counts = short_case()
    caps = [int(counts[d, 1]) for d in range(3)]
    ncaps = [int(counts[d, 0]) for d in range(3)]
    if short == "one record":
        ncaps[1] -= 1
    elif short == "one dword":
        caps[2] -= 4
    else:
        caps[0] -= 6
    dev = Dev(ctx, ro, data, None, dest, 3, caps, ncaps)
    try:
        rc, got = dev.call()
        assert rc == -errno.ENOSPC == sm.verdict(0, counts, caps, ncaps)
        assert np.array_equal(got, counts)
        assert [dev.outs[d].n for d in range(3)] == [0, 0, 0]
        dev.check_buffers(outs, short)
    finally:
        dev.free()


def malformed_cases():
    ro, data = stream([12, 16, 0, 20, 4104], seed=190)
    ok_mask = np.array([1, 2, 3, 1, 2], np.uint32)
    ids = np.array([5, 2, 9, 11, 3], np.uint32)

    def with_ro(i, v):
        r = ro.copy()
        r[i] = v
        return r
    return [
        ("not from 0", with_ro(0, 4), ok_mask, 0, sm.ERR_STREAM),
        ("decreasing", with_ro(2, 8), ok_mask, 0, sm.ERR_STREAM),
        ("not 4-aligned", with_ro(3, 30), ok_mask, 0, sm.ERR_STREAM),
        ("past the capacity", with_ro(5, len(data) + 4), ok_mask, 0, sm.ERR_STREAM),
        ("mask bit >= G", ro, np.array([1, 2, 4, 1, 2], np.uint32), 0, sm.ERR_IDS),
        ("home >= G", ro, None, 5, sm.ERR_IDS),
        ("both", with_ro(0, 4), np.array([1, 8, 3, 1, 2], np.uint32), 0,
         sm.ERR_STREAM | sm.ERR_IDS),
    ], data, ids


def test_refusals_write_no_data(ctx):
    cases, data, ids = malformed_cases()
    for name, ro, dest, per, bits in cases:
        err, _, counts = sm.split(ro, data, ids, dest, per, 2)
        assert err == bits, name
        dev = Dev(ctx, ro, data, ids, dest, 2, [8192, 8192], [8, 8])
        try:
            rc, got = dev.call(per)
            assert rc == -errno.EINVAL, name
            assert not got.any() and [dev.outs[d].n for d in range(2)] == [0, 0], name
            dev.check_buffers(None, name)
            # the refusal was this call's own: nothing is left for gdsm_sync
            assert lib().gdsm_sync(ctx.handle) == 0, name
        finally:
            dev.free()


def test_an_earlier_error_bit_stays_for_sync(ctx):
    """An id out of range in an unsynchronised gdsm_digest leaves an error bit; the split that
    follows is judged on its own checks and gdsm_sync still reports the bit."""
    ro, data = stream([12, 16, 20], seed=191)
    dig = ctx.buffer(32)
    bad = ctx.ids(np.array([3, 1000], np.uint32))
    try:
        assert lib().gdsm_digest(ctx.handle, ga.CURRENT, bad.ptr, 2, dig.ptr) == 0
        check(ctx, ro, data, None, np.array([1, 3, 2], np.uint32), 0, 2)
        assert lib().gdsm_sync(ctx.handle) == -errno.EINVAL
        assert lib().gdsm_sync(ctx.handle) == 0
    finally:
        dig.free()
        bad.free()


def test_recording_context_gets_ebusy(ctx):
    ro, data = stream([12, 16, 20], seed=192)
    dev = Dev(ctx, ro, data, None, np.array([1, 1, 1], np.uint32), 1, [64], [4])
    dig = ctx.buffer(16)
    try:
        ctx.capture_begin()
        try:
            ctx.digest("current", n=1, out=dig)
            rc, _ = dev.call()
        finally:
            ctx.capture_end().destroy()
        assert rc == -errno.EBUSY
        got = dev.o_ro[0].download(np.uint64, 4 + 1 + PAD)
        assert (got == CANARY64).all()
    finally:
        dig.free()
        dev.free()


def test_raw_on_torch_tensors():
    import torch
    rng = np.random.default_rng(200)
    n, G = 3 * T + 17, 3
    ro, data = stream(mixed_sizes(rng, n), seed=200)
    ids = rng.permutation(n).astype(np.uint32)
    dest = rng.integers(0, 1 << G, n).astype(np.uint32)
    lb = lib()
    stream_ptr = torch.cuda.current_stream().cuda_stream

    def dev(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()

    t_ro = dev(ro, np.int64)
    # the input's data 4 bytes into its tensor: a source that is only dword aligned
    t_data = torch.zeros(len(data) + 16, dtype=torch.uint8, device="cuda")
    t_data[4:4 + len(data)] = torch.from_numpy(data).cuda()
    t_ids = dev(ids, np.int32)
    bad_dest = dest.copy()
    bad_dest[n // 2] |= 1 << G
    bad_ro = ro.copy()
    bad_ro[7] += 2
    per = -(-n // G)
    # (name, masks or None, per, flags, offsets, the err bits expected, capacities cut short)
    cases = [("mask", dest, 0, 0, ro, 0, None),
             ("home, short", None, per, 1, ro, 0, (5, 40)),
             ("malformed", dest, 0, 0, bad_ro, sm.ERR_STREAM, None),
             ("mask bit >= G", bad_dest, 0, 0, ro, sm.ERR_IDS, None),
             ("home >= G", None, per - 2, 0, ro, sm.ERR_IDS, None),
             ("both", bad_dest, 0, 1, bad_ro, sm.ERR_STREAM | sm.ERR_IDS, None)]
    for name, m_dest, per, flags, m_ro, bits, short in cases:
        t_ro = dev(m_ro, np.int64)
        t_dest = dev(m_dest, np.int32) if m_dest is not None else None
        p_dest = t_dest.data_ptr() if t_dest is not None else None
        err, outs, counts = sm.split(m_ro, data, ids, m_dest, per, G, flags)
        assert err == bits, name
        if err:  # (buffers sized as for the well-formed call)
            _, outs, counts = sm.split(ro, data, ids, dest if m_dest is not None else None,
                                       0 if m_dest is not None else -(-n // G), G, flags)
        drop_rec, drop_bytes = short or (0, 0)
        caps = [int(counts[d, 1]) for d in range(G)]
        ncaps = [int(counts[d, 0]) for d in range(G)]
        if drop_rec:
            ncaps[1] -= drop_rec
            caps[2] -= drop_bytes
        o_ro = [torch.full((ncaps[d] + 1 + PAD,), -1, dtype=torch.int64, device="cuda")
                for d in range(G)]
        # every output's data 8 bytes into its tensor
        o_data = [torch.full((caps[d] + 8 + PAD_BYTES,), CANARY8, dtype=torch.uint8, device="cuda")
                  for d in range(G)]
        o_ids = [torch.full((ncaps[d] + PAD,), -1, dtype=torch.int32, device="cuda")
                 for d in range(G)]
        t_counts = torch.full((2 * G,), -1, dtype=torch.int64, device="cuda")
        t_err = torch.zeros(1, dtype=torch.int32, device="cuda")
        need = lb.gdsm_runs_split_workspace_bytes(n, G)
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        args = (t_ro.data_ptr(), t_data.data_ptr() + 4, len(data), t_ids.data_ptr(), p_dest, per,
                n, G, (C.c_void_p * G)(*[t.data_ptr() for t in o_ro]),
                (C.c_void_p * G)(*[t.data_ptr() + 8 for t in o_data]),
                (C.c_uint64 * G)(*caps), (C.c_uint64 * G)(*ncaps),
                (C.c_void_p * G)(*[t.data_ptr() for t in o_ids]), t_counts.data_ptr(),
                t_err.data_ptr(), flags)
        assert lb.gdsm_runs_split_raw(*args, ws.data_ptr(), need - 1, stream_ptr) == -22
        assert lb.gdsm_runs_split_raw(*args, None, need, stream_ptr) == -22
        assert lb.gdsm_runs_split_raw(*args, ws.data_ptr(), need, stream_ptr) == 0
        torch.cuda.synchronize()
        assert int(t_err.cpu()[0]) == err, name
        if err:
            counts = np.zeros((G, 2), np.uint64)
        assert t_counts.cpu().numpy().view(np.uint64).reshape(G, 2).tolist() == counts.tolist(), name
        for d in range(G):
            o, buf, pg = sm.written(outs[d], caps[d], ncaps[d]) if not err else \
                (np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint32))
            got = o_ro[d].cpu().numpy().view(np.uint64)
            assert np.array_equal(got[:len(o)], o) and (got[len(o):] == np.uint64(CANARY_ALL)).all(), (name, d)
            got = o_data[d].cpu().numpy()
            assert (got[:8] == CANARY8).all() and (got[8 + len(buf):] == CANARY8).all(), (name, d)
            assert np.array_equal(got[8:8 + len(buf)], buf), (name, d)
            got = o_ids[d].cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:len(pg)], pg) and (got[len(pg):] == 0xFFFFFFFF).all(), (name, d)
    assert np.array_equal(t_data.cpu().numpy()[4:4 + len(data)], data)


def test_split_by_home_then_apply_equals_apply():
    Z, G = 300, 4
    per = -(-Z // G)
    twin, cur = real_stream(210, Z)
    ids = np.flatnonzero((twin != cur).any(axis=1)).astype(np.uint32)
    with ga.Context(Z) as c:
        c.upload("twin", twin)
        c.upload("current", cur)
        c.upload("replica", twin)
        d_ids = c.ids(ids)
        runs = c.diff(d_ids, n=len(ids))
        c.apply(runs, "replica", d_ids)
        c.sync()
        full = c.download("replica")
        assert np.array_equal(full, cur)
        res = c.runs_split(runs, ids=d_ids, per=per, G=G)
        assert int(res.counts[:, 0].sum()) == len(ids)
        for d in range(G):
            lo, hi = d * per, min(Z, (d + 1) * per)
            assert res.runs[d].n == int(((ids >= lo) & (ids < hi)).sum())
            c.upload("replica", twin[lo:hi])
            c.apply(res.runs[d], "replica", res.ids[d])
            c.sync()
            assert np.array_equal(c.download("replica", 0, hi - lo), full[lo:hi]), d
        res.free()
        runs.free()


def test_split_by_mask_then_merge_returns_the_input():
    Z, G = 200, 8
    twin, cur = real_stream(220, Z)
    ids = np.flatnonzero((twin != cur).any(axis=1)).astype(np.uint32)
    rng = np.random.default_rng(221)
    with ga.Context(Z) as c:
        c.upload("twin", twin)
        c.upload("current", cur)
        d_ids = c.ids(ids)
        runs = c.diff(d_ids, n=len(ids))
        want = runs.to_host()
        dest = c.ids((np.uint32(1) << rng.integers(0, G, len(ids)).astype(np.uint32)))
        res = c.runs_split(runs, ids=d_ids, dest=dest, G=G)
        assert int(res.counts[:, 0].sum()) == len(ids)
        assert int(res.counts[:, 1].sum()) == int(want.rec_off[-1])
        m = c.merge(res.runs, ids=res.ids, out_ids=d_ids)
        m.runs.s.n = len(ids)
        got = m.runs.to_host()
        assert np.array_equal(got.rec_off, want.rec_off) and np.array_equal(got.data, want.data)
        assert m.stats == {"overlap_bytes": 0, "conflict_bytes": 0}
        m.free()
        m.runs.free()
        res.free()
        runs.free()
    # the wrapper reports what a short output needs
    with ga.Context(8) as c:
        ro, data = stream([12, 16, 20], seed=222)
        runs = ga.Runs.from_host(c, ga.HostRuns(ro, data))
        small = ga.Runs(c, 2, 64)
        with pytest.raises(GdsmError) as e:
            c.runs_split(runs, dest=c.ids(np.ones(3, np.uint32)), G=1, outs=[(small, None)])
        assert e.value.errno == errno.ENOSPC and e.value.counts.tolist() == [[3, 48]]
        assert small.n == 0


def test_sparse_release_end_to_end_on_the_loopback_communicator():
    """4 ranks, 750 global pages (homes of 188, 188, 188 and 186): every rank writes its own
    sparse set of global pages; scan -> diff of the list -> split by home -> exchange."""
    G, total = 4, 750
    per = -(-total // G)
    rng = np.random.default_rng(230)
    base = rng.integers(0, 256, (total, 4096), dtype=np.uint8)
    owner = rng.integers(0, 6, total)  # ranks 0..3 write theirs, 4 and 5: nobody writes the page
    expect = base.copy()
    curs = []
    for r in range(G):
        cur = base.copy()
        for p in np.flatnonzero(owner == r)[::3]:
            k = int(rng.integers(1, 50))
            cur[p, rng.integers(0, 4096, k)] ^= rng.integers(1, 256, k).astype(np.uint8)
            expect[p] = cur[p]
        curs.append(cur)
    ctxs = [ga.Context(total) for _ in range(G)]
    for r, c in enumerate(ctxs):
        c.upload("twin", base)
        c.upload("current", curs[r])
        lo, hi = r * per, min(total, (r + 1) * per)
        c.upload("replica", base[lo:hi])
    comms = exchange.Comm.loopback(ctxs)
    try:
        def rank(r):
            c = ctxs[r]
            dl = c.dirty_scan()
            count, bound = dl.count, dl.bound
            assert count == int((curs[r] != base).any(axis=1).sum()) > 10
            runs = ga.Runs(c, count, cap=bound)
            c.diff(dl.pages, n=count, out=runs)
            res = exchange.split_by_home(c, runs, dl.pages, total, G)
            assert int(res.counts[:, 0].sum()) == count
            recv = [ga.Runs(c, per, cap=per * 1024) for _ in range(G)]
            rids = [c.buffer(4 * per) for _ in range(G)]
            exchange.exchange_runs(c, comms[r], res.runs, [b.ptr for b in res.ids], recv,
                                   [b.ptr for b in rids])
            c.sync()
        run_ranks(G, rank)
        for r, c in enumerate(ctxs):
            lo, hi = r * per, min(total, (r + 1) * per)
            got = c.download("replica", 0, hi - lo)
            assert np.array_equal(got, expect[lo:hi]), r
            untouched = np.flatnonzero((expect[lo:hi] == base[lo:hi]).all(axis=1))
            assert len(untouched) > 100 and np.array_equal(got[untouched], base[lo:hi][untouched])
    finally:
        for cm in comms:
            cm.close()
        for c in ctxs:
            c.close()
