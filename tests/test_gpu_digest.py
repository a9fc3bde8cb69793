"""gdsm_digest on the GPU (docs/SPEC.md §10) against the numpy model tests/digest_model.py, bit for
bit: list lengths around the launch geometry, no list / a permutation / a list with repeats, each
arena, pages of all zero, all 0xFF, random and differing in the last byte only; the raw entry point
on a torch tensor; an id out of range; the profiling stage."""
import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd.gdsm import GdsmError, lib
from tests import digest_model as dm

pytestmark = pytest.mark.gpu

Z = 300
ARENAS = ("twin", "current", "replica")


def make_pages(seed):
    """Z pages: 0 all zero, 1 all 0xFF, the rest random; page 3 is page 2 but for byte 4095."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (Z, 4096), dtype=np.uint8)
    p[0] = 0
    p[1] = 0xFF
    p[3] = p[2]
    p[3, 4095] ^= 0x80
    return p


@pytest.fixture(scope="module")
def shard():
    """One context with its own contents per arena and the model's digests of every page."""
    host = {a: make_pages(40 + k) for k, a in enumerate(ARENAS)}
    ctx = ga.Context(Z)
    for a in ARENAS:
        ctx.upload(a, host[a])
    want = {a: dm.digests(host[a]) for a in ARENAS}
    yield ctx, want
    ctx.close()


def read(ctx, buf, n):
    ctx.sync()
    return buf.download(np.uint64, 2 * n).reshape(n, 2)


@pytest.mark.parametrize("n", [0, 1, 3, 64, 257])
def test_digest_equals_model(shard, n):
    ctx, want = shard
    rng = np.random.default_rng(n)
    lists = {"none": None,
             "permutation": rng.permutation(Z)[:n].astype(np.uint32),
             "repeats": rng.integers(0, max(1, min(Z, n // 2 + 1)), n).astype(np.uint32)}
    out = ctx.buffer(16 * max(n, 1))
    for arena in ARENAS:
        for kind, ids in lists.items():
            out.upload(np.full(2 * max(n, 1), 0xA5A5A5A5A5A5A5A5, np.uint64))
            buf = ctx.ids(ids) if ids is not None and n else None
            ctx.digest(arena, buf, n=n, out=out)
            got = read(ctx, out, max(n, 1))
            exp = want[arena][:n] if ids is None else want[arena][ids]
            assert np.array_equal(got[:n], exp), (arena, kind)
            if n == 0:  # a no-op: nothing written
                assert got[0, 0] == 0xA5A5A5A5A5A5A5A5
            if buf is not None:
                buf.free()
    out.free()


def test_digest_fixed_vectors_and_last_byte(shard):
    ctx, want = shard
    got = read(ctx, ctx.digest("current", n=4), 4)
    assert [hex(int(x)) for x in got[0]] == ["0x6397fb63bb6eafd", "0xb3d0051bf22bf1ec"]
    assert [hex(int(x)) for x in got[1]] == ["0x6397dbced7578a1", "0xb3d00323a05cee0f"]
    assert got[2, 0] != got[3, 0] and got[2, 1] != got[3, 1]
    assert np.array_equal(got, want["current"][:4])


def test_digest_whole_arena_without_arguments(shard):
    ctx, want = shard
    assert np.array_equal(read(ctx, ctx.digest("replica"), Z), want["replica"])


def test_digest_raw_on_a_torch_tensor():
    import torch
    host = make_pages(50)
    ids = np.array([7, 0, 299, 7, 3], np.int32)
    t = torch.from_numpy(host).cuda()
    d_ids = torch.from_numpy(ids).cuda()
    out = torch.zeros(2 * Z, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib().gdsm_digest_raw(t.data_ptr(), None, Z, out.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    want = dm.digests(host)
    assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(Z, 2), want)
    assert lib().gdsm_digest_raw(t.data_ptr(), d_ids.data_ptr(), len(ids), out.data_ptr(),
                                 stream) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64).reshape(Z, 2)
    assert np.array_equal(got[:len(ids)], want[ids])
    assert np.array_equal(got[len(ids):], want[len(ids):])  # nothing past the list


def test_digest_id_out_of_range(shard):
    ctx, want = shard
    ids = np.array([5, Z, 9, 2], np.uint32)
    buf = ctx.ids(ids)
    out = ctx.digest("twin", buf)
    with pytest.raises(GdsmError) as ei:
        ctx.sync()
    assert ei.value.errno == 22
    got = out.download(np.uint64, 8).reshape(4, 2)
    assert got[1].tolist() == [0, 0]
    assert np.array_equal(got[[0, 2, 3]], want["twin"][[5, 9, 2]])
    ctx.sync()  # the error was reported once
    lb = lib()
    assert lb.gdsm_digest(ctx.handle, 3, None, 1, out.ptr) == -22
    assert lb.gdsm_digest(ctx.handle, -1, None, 1, out.ptr) == -22
    assert lb.gdsm_digest(ctx.handle, 1, None, 1, None) == -22
    assert lb.gdsm_digest(ctx.handle, 1, None, 0, None) == 0
    with ga.Context(4, arenas=("current",)) as one:
        assert lb.gdsm_digest(one.handle, ga.REPLICA, None, 1, out.ptr) == -22
    buf.free()
    out.free()


def test_digest_profiling_stage(shard):
    ctx, _ = shard
    assert ga.Context.PROF_STAGES[-1] == "digest"
    ctx.prof_enable(True)
    try:
        out = ctx.digest("current", n=Z)
        prof = ctx.prof_read()
    finally:
        ctx.prof_enable(False)
    ms, launches = prof["digest"]
    assert launches == 1 and ms > 0
    assert all(v[1] == 0 for k, v in prof.items() if k != "digest")
    out.free()


def test_digest_records_into_a_graph(shard):
    """No workspace and no host synchronisation: the call can be recorded and replayed."""
    ctx, want = shard
    out = ctx.buffer(16 * Z)
    ctx.capture_begin()
    try:
        ctx.digest("current", n=Z, out=out)
    finally:
        g = ctx.capture_end()
    out.upload(np.zeros(2 * Z, np.uint64))
    g.launch(ctx)
    assert np.array_equal(read(ctx, out, Z), want["current"])
    g.destroy()
    out.free()
