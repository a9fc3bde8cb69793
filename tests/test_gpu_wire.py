"""GPU diff wire format (gdsm_wire_encode / decode / apply, docs/SPEC.md §7) against the oracle
restatement (oracle/wire.py): the command text is byte-identical, decode returns the stream, the
follower apply reproduces CURRENT, and every malformed text is refused with nothing applied."""
import base64
import ctypes as C

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import _lib
from gallocy_amd.gdsm import GdsmError, HostRuns, Runs
from oracle import oracle, wire

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with ga.Context(4096) as c:
        yield c


def _setup(ctx, seed, ppm=10000, mode=0):
    n = ctx.n_pages
    ctx.gen_pages(seed=seed, mode=mode, ppm=ppm)
    ctx.sync()
    return oracle.gen_pages(n, seed=seed, mode=mode, ppm=ppm)


def test_encode_matches_oracle_all_pages(ctx):
    twin, cur = _setup(ctx, 11)
    runs = ctx.diff()
    text = ctx.wire_encode(runs)
    ro, data = oracle.diff_pages(twin, cur)
    assert text == wire.encode(np.arange(ctx.n_pages, dtype=np.uint32), ro, data)
    runs.free()


@pytest.mark.parametrize("count", [1, 3, 1001])
def test_encode_listed_pages_and_apply(ctx, count):
    twin, cur = _setup(ctx, 20 + count, ppm=50000, mode=1)
    rng = np.random.default_rng(count)
    ids = np.sort(rng.choice(ctx.n_pages, count, replace=False)).astype(np.uint32)
    dids = ctx.ids(ids)
    runs = ctx.diff(dids)
    text = ctx.wire_encode(runs, dids)
    ro, data = oracle.diff_pages(twin, cur, ids=ids)
    assert text == wire.encode(ids, ro, data)
    # follower: replica holds the twin; try_apply the committed command
    ctx.upload("replica", twin)
    assert ctx.wire_apply(text) == count
    want = twin.copy()
    want[ids] = cur[ids]
    assert np.array_equal(ctx.download("replica"), want)
    # decode hands back the same stream
    i2, r2 = ctx.wire_decode(text, count, max(16, len(data)))
    h = r2.to_host()
    assert np.array_equal(h.rec_off, ro) and np.array_equal(h.data, data)
    assert np.array_equal(i2.download(np.uint32, count), ids)
    for x in (i2, r2, runs, dids):
        x.free()


def test_rejected_texts_apply_nothing(ctx):
    twin, cur = _setup(ctx, 31)
    ids = np.arange(0, 64, dtype=np.uint32)
    ro, data = oracle.diff_pages(twin, cur, ids=ids)
    good = wire.encode(ids, ro, data)
    f = base64.b64decode(good[6:])
    big = ids.copy()
    big[5] = ctx.n_pages  # outside the arena, checksum valid
    cases = [good[:-4], b"GDSM2" + good[5:], good[:100] + b"!" + good[101:],
             wire.PREFIX + base64.b64encode(f[:200] + bytes([f[200] ^ 0x10]) + f[201:]),
             wire.encode(big, ro, data), good[:6] + good[10:]]
    ctx.upload("replica", twin)
    for t in cases:
        with pytest.raises(GdsmError):
            ctx.wire_apply(t)
    assert np.array_equal(ctx.download("replica"), twin)
    assert ctx.wire_apply(good) == 64
    assert np.array_equal(ctx.download("replica")[:64], cur[:64])


# ---- text shapes: every branch of b64_decode_kernel / wire_check_kernel on a one-page context ----
@pytest.fixture(scope="module")
def one():
    with ga.Context(1, arenas=("replica",)) as c:
        yield c


def _shape_stream(n, m, seed):
    """n records, the first m of them 16-B word edits, the rest empty; ids are n distinct pages of
    a larger space (decode does not bound them; apply is only given n <= 1)."""
    rng = np.random.default_rng(seed)
    recs = [np.frombuffer(np.array([1, 8 * int(rng.integers(0, 512)) | (8 << 16)], "<u4").tobytes()
                          + rng.integers(1, 256, 8, dtype=np.uint8).tobytes(), np.uint8)
            for _ in range(m)]
    ro = np.zeros(n + 1, np.uint64)
    ro[1:m + 1] = 16 * np.arange(1, m + 1)
    ro[m + 1:] = 16 * m
    data = np.concatenate(recs) if recs else np.zeros(0, np.uint8)
    ids = (np.arange(n, dtype=np.uint32) * 7) if n > 1 else np.zeros(n, np.uint32)
    return ids, ro, data


SHAPES = [(0, 0), (1, 1), (1, 0), (2, 1), (2, 2), (3, 1), (3, 3), (4, 2), (5, 5), (6, 1), (7, 2), (8, 8)]


def test_shapes_cover_every_text_form():
    """The (records, non-empty records) pairs below give n = 0, odd and even n, frame lengths that
    are 0, 1 and 2 modulo 3 (no '=', '==', '='), and bodies that are and are not whole 16-character
    pieces."""
    F = [wire.frame_bytes(n, 16 * m) for n, m in SHAPES]
    T = [4 * ((f + 2) // 3) for f in F]
    assert {f % 3 for f in F} == {0, 1, 2}
    assert {t % 16 == 0 for t in T} == {True, False}
    assert {n % 2 for n, _ in SHAPES if n} == {0, 1} and (0, 0) in SHAPES
    for (n, m), f, t in zip(SHAPES, F, T):
        text = wire.encode(*_shape_stream(n, m, n))
        assert len(text) == 6 + t and text.count(b"=") == (0, 2, 1)[f % 3]


@pytest.mark.parametrize("n,m", SHAPES)
def test_text_shapes_encode_decode_apply(one, n, m):
    ids, ro, data = _shape_stream(n, m, n)
    text = wire.encode(ids, ro, data)
    runs = Runs.from_host(one, HostRuns(ro, data))
    dids = one.ids(ids)
    assert one.wire_encode(runs, dids) == text
    i2, r2 = one.wire_decode(text, n, max(16, len(data)))
    assert r2.n == n
    h = r2.to_host()
    assert np.array_equal(h.rec_off, ro) and np.array_equal(h.data, data)
    assert np.array_equal(i2.download(np.uint32, n), ids)
    if n <= 1:
        page = np.random.default_rng(5).integers(1, 256, (1, 4096), dtype=np.uint8)
        want = page.copy()
        assert oracle.apply(want, ro, data, ids=ids) == 0
        one.upload("replica", page)
        assert one.wire_apply(text) == n
        assert np.array_equal(one.download("replica"), want)
    for x in (i2, r2, runs, dids):
        x.free()


@pytest.mark.parametrize("n,m", [(1, 1), (2, 1), (2, 2)])  # no '=', '==', '='
def test_misplaced_padding_is_refused(one, n, m):
    """'=' at position T - 3 (never padding) and '=' inside the first 44 characters (the header,
    decoded on the host) are refused, by decode and by apply, and nothing is applied."""
    ids, ro, data = _shape_stream(n, m, n)
    text = wire.encode(ids, ro, data)
    T = len(text) - 6
    page = np.random.default_rng(6).integers(1, 256, (1, 4096), dtype=np.uint8)
    one.upload("replica", page)
    for pos in (T - 3, 10, 43):
        bad = text[:6 + pos] + b"=" + text[6 + pos + 1:]
        assert len(bad) == len(text) and bad != text
        with pytest.raises(ValueError):
            wire.decode(bad)
        with pytest.raises(GdsmError) as e:
            one.wire_decode(bad, n, max(16, len(data)))
        assert e.value.errno == 22
        with pytest.raises(GdsmError) as e:
            one.wire_apply(bad)
        assert e.value.errno == 22
    assert np.array_equal(one.download("replica"), page)
    i2, r2 = one.wire_decode(text, n, max(16, len(data)))  # the context still decodes
    i2.free()
    r2.free()


def test_encode_capacity_one_byte_short(one):
    ids, ro, data = _shape_stream(3, 3, 9)
    text = wire.encode(ids, ro, data)
    runs = Runs.from_host(one, HostRuns(ro, data))
    dids = one.ids(ids)
    L = _lib.load()
    need = len(text)  # the text needs need + 1 bytes: its NUL
    for cap in (need, 0):
        buf = C.create_string_buffer(need + 1)
        ln = C.c_uint64(0)
        rc = L.gdsm_wire_encode(one.handle, dids.ptr, C.byref(runs.s), buf if cap else None, cap, C.byref(ln))
        assert rc == -28 and ln.value == need
        assert buf.raw == b"\0" * (need + 1)
    buf = C.create_string_buffer(need + 1)
    ln = C.c_uint64(0)
    assert L.gdsm_wire_encode(one.handle, dids.ptr, C.byref(runs.s), buf, need + 1, C.byref(ln)) == 0
    assert buf.raw[:need] == text and ln.value == need
    runs.free()
    dids.free()


def test_decode_into_a_stream_too_small(one):
    ids, ro, data = _shape_stream(3, 3, 9)
    text = wire.encode(ids, ro, data)
    with pytest.raises(GdsmError) as e:
        one.wire_decode(text, 2, len(data))  # one record short
    assert e.value.errno == 28
    L = _lib.load()
    out = Runs(one, 3, len(data))
    dids = one.buffer(16)
    out.s.cap = len(data) - 4  # four data bytes short
    n = C.c_uint64(0)
    assert L.gdsm_wire_decode(one.handle, text, len(text), dids.ptr, C.byref(out.s), C.byref(n)) == -28
    out.s.cap = len(data)
    assert L.gdsm_wire_decode(one.handle, text, len(text), dids.ptr, C.byref(out.s), C.byref(n)) == 0
    assert n.value == 3
    out.free()
    dids.free()
