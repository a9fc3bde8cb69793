"""GPU Needleman-Wunsch (gdsm_nw_diff_batch, the legacy diff() on the GPU) against the reference's
own goldens, the vectors the reference produced (tests/golden/nw_ref.npz) and the C oracle
(or_nw_diff <- gallocy/utils/diff.cpp:73-167) on seeded random pairs, on the structured corpus of
tests/nw_corpus.py (paths far from the trace's guessed strip entries) and around the launcher:
chunked batches, stale workspace slots, output bounds. Bit-exact: the outputs are bytes."""
import ctypes as C

import numpy as np
import pytest

import gallocy_amd as ga
from gallocy_amd import _lib
from gallocy_amd.gdsm import GdsmError
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with ga.Context(1, arenas=()) as c:
        yield c


def _rand(rng, n, alphabet=256):
    return bytes(rng.integers(0, alphabet, n, dtype=np.uint8))


def test_reference_test_diff_goldens(ctx):
    # test/test_diff.cpp:13-16, 24-31 and the SURVEY §8c KATs, in one batch
    cases = [(b"GGAATGG", b"ATG", b"GGAATGG", b"---AT-G"),
             (b"FOO BOP BOOP", b"FOOO BOOP BOP", b"F-OO B-OP BOOP", b"FOOO BOOP B-OP"),
             (b"", b"", b"", b""), (b"", b"ABC", b"---", b"ABC"), (b"ABC", b"", b"ABC", b"---"),
             (b"AB", b"BA", b"AB", b"BA"), (b"ABCD", b"BCDA", b"ABCD-", b"-BCDA"),
             (b"AAAA", b"AA", b"AAAA", b"--AA"), (b"AA", b"AAAA", b"--AA", b"AAAA"),
             (b"ACGT", b"TGCA", b"ACGT", b"TGCA"), (b"HELLO", b"YELLOW", b"HELLO-", b"YELLOW"),
             (b"0123456789", b"0123X56789", b"0123456789", b"0123X56789")]
    got = ctx.nw_diff_batch([(a, b) for a, b, _, _ in cases])
    assert got == [(o1, o2) for _, _, o1, o2 in cases]


def test_reference_produced_vectors(ctx, golden):
    from tests.test_oracle import _nw_golden_cases
    cases = list(_nw_golden_cases(golden))
    assert len(cases) >= 31
    got = ctx.nw_diff_batch([(a, b) for a, b, _, _ in cases])
    assert got == [(o1, o2) for _, _, o1, o2 in cases]


# Shapes around every boundary of the kernel: strips (512 rows; 256 in the 4-row build), the
# 8-strip group whose last strip hands over through global memory (n1 > 4096), the lane pipeline
# (64 columns), the 16-step blocks, the 64-step phases and the regions the trace recomputes from
# checkpoints (a path through many regions: long and thin both ways).
SHAPES = [(1, 1), (1, 300), (300, 1), (63, 64), (64, 65), (255, 17), (256, 256), (257, 1000),
          (1000, 257), (700, 700), (4096, 33), (4097, 80), (8500, 40), (50, 5000),
          (128, 65), (129, 66), (200, 193), (3000, 2900), (16, 3000), (511, 100), (512, 512),
          (513, 70)]


@pytest.mark.parametrize("alphabet", [256, 4, 2])
def test_random_pairs_vs_oracle(ctx, alphabet):
    """Small alphabets make ties everywhere, which exercises diag > left > up."""
    rng = np.random.default_rng(100 + alphabet)
    pairs = [(_rand(rng, n1, alphabet), _rand(rng, n2, alphabet)) for n1, n2 in SHAPES]
    got = ctx.nw_diff_batch(pairs)
    for (a, b), g in zip(pairs, got):
        assert g == oracle.nw_diff(a, b), (len(a), len(b))


def test_pages_with_sparse_writes_and_shifts(ctx):
    """4 KiB pages (BASELINE config 1 shape): substitution-only edits (identity alignment), a
    memmove-shifted page and an insertion, which the run diff cannot express but NW can."""
    rng = np.random.default_rng(7)
    pairs = []
    for i in range(6):
        twin = bytearray(_rand(rng, 4096))
        cur = bytearray(twin)
        for off in rng.choice(512, 5, replace=False):
            cur[8 * off:8 * off + 8] = _rand(rng, 8)
        pairs.append((bytes(twin), bytes(cur)))
    base = _rand(rng, 4096)
    pairs.append((base, base[100:] + _rand(rng, 100)))
    pairs.append((base, base[:2000] + b"INSERTED" + base[2000:4088]))
    got = ctx.nw_diff_batch(pairs)
    for (a, b), g in zip(pairs, got):
        assert g == oracle.nw_diff(a, b)
    for (a, b), (o1, o2) in zip(pairs[:6], got[:6]):
        assert o1 == a and o2 == b  # equal-length substitutions align gap-free


def test_long_strings_read_b_from_global(ctx):
    """Beyond 48 KiB the fill reads b from global memory instead of LDS; the whole batch takes
    that kernel (max_len decides), short pairs included."""
    rng = np.random.default_rng(11)
    pairs = [(_rand(rng, 60, 4), _rand(rng, 50000, 4)), (_rand(rng, 50000, 4), _rand(rng, 70, 4)),
             (_rand(rng, 700, 4), _rand(rng, 650, 4))]
    got = ctx.nw_diff_batch(pairs)
    for (a, b), g in zip(pairs, got):
        assert g == oracle.nw_diff(a, b), (len(a), len(b))


def test_max_len_is_enforced(ctx):
    with pytest.raises(GdsmError):
        ctx.nw_diff_batch([(b"A" * 100, b"B" * 10)], max_len=64)


def test_legacy_diff_symbol_offloaded(ctx):
    """gdsm_set_diff_device routes the C++ `diff` symbol (diff.h:9-11) to the GPU."""
    lib = _lib.load()
    fn = getattr(lib, _lib.LEGACY_DIFF_SYMBOL)
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t,
                   C.POINTER(C.c_void_p)]
    rng = np.random.default_rng(3)
    a, b = _rand(rng, 3000, 4), _rand(rng, 2900, 4)
    ga.set_diff_device(ctx, 0)
    try:
        r1, r2 = C.c_void_p(), C.c_void_p()
        assert fn(a, len(a), C.byref(r1), b, len(b), C.byref(r2)) == 0
        want = oracle.nw_diff(a, b)
        got = (C.string_at(r1, len(want[0])), C.string_at(r2, len(want[1])))
        assert C.string_at(r1) == want[0].split(b"\0")[0]  # NUL-terminated like the reference
        libc = C.CDLL(None)
        libc.free(r1)
        libc.free(r2)
        assert got == want
        assert ga.diff(a, b) == want  # gdsm_nw_diff takes the same route
    finally:
        ga.set_diff_device(None)


# ---- paths far from the trace's guessed strip entries, chunked launches, stale slots ----------
def _check(pairs, got):
    assert len(got) == len(pairs)
    for i, ((a, b), g) in enumerate(zip(pairs, got)):
        assert g == oracle.nw_diff(a, b), (i, len(a), len(b))


def test_structured_corpus_vs_oracle(ctx):
    """tests/nw_corpus.py: re-walks that merge on their first row, later or never, column-0
    re-walks, row-0 runs, entries 600 columns off the guess (tests/test_nw_corpus.py pins that
    the corpus reaches them). One batch, then pair by pair."""
    from tests import nw_corpus
    corpus = nw_corpus.corpus()
    want = {name: oracle.nw_diff(a, b) for name, (a, b) in corpus.items()}
    got = ctx.nw_diff_batch(list(corpus.values()))
    for name, g in zip(corpus, got):
        assert g == want[name], name
    for name, pair in corpus.items():
        assert ctx.nw_diff_batch([pair]) == [want[name]], name


SWEEP_N1 = (511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
SWEEP_N2 = (1, 2, 15, 16, 17, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193, 194, 255, 256, 257, 300)
# more than 8 strips and more than 80 columns: the last wave of a group hands its bottom row to
# wave 0 through global memory while the 256-slot rings wrap, over several phases
WIDE_GROUPS = ((4700, 900), (8200, 300), (4097, 257))


@pytest.mark.parametrize("shapes,alphabet",
                         [("sweep", 2), ("sweep", 4), ("wide", 4), ("wide", 256)])
def test_boundary_sweep_vs_oracle(ctx, shapes, alphabet):
    """Strip and group boundaries in n1 against lane, block, phase and ring boundaries in n2."""
    rng = np.random.default_rng(1000 + alphabet + (shapes == "wide"))
    dims = WIDE_GROUPS if shapes == "wide" else [(n1, n2) for n1 in SWEEP_N1 for n2 in SWEEP_N2]
    pairs = [(_rand(rng, n1, alphabet), _rand(rng, n2, alphabet)) for n1, n2 in dims]
    _check(pairs, ctx.nw_diff_batch(pairs))


def test_zero_length_beside_long_pairs(ctx):
    """The fill returns early for a pair with an empty string and leaves its workspace slot as
    the previous launch wrote it; the trace of such a pair must read none of it."""
    rng = np.random.default_rng(21)
    dims = [(1500, 700), (1500, 0), (0, 1500), (600, 0), (0, 0), (513, 1), (1, 513), (1500, 700)]
    pairs = [(_rand(rng, n1, 4), _rand(rng, n2, 4)) for n1, n2 in dims]
    want = [oracle.nw_diff(a, b) for a, b in pairs]
    assert ctx.nw_diff_batch(pairs) == want
    assert ctx.nw_diff_batch(pairs) == want
    # and once shifted by a slot: every empty pair in a slot a long pair has just filled
    assert ctx.nw_diff_batch(pairs[-1:] + pairs[:-1]) == want[-1:] + want[:-1]


def _pair_ws_bytes(max_len):
    """Geo::per_pair() of gdsm_nw.hip restated: checkpoints, bottom rows and row records."""
    strips = max(1, -(-max_len // 512))
    blocks = (max_len + 63 + 15) // 16
    ck = strips * ((blocks * 16 + 63) // 64) * 64 * 40
    rows = (strips * (max_len + 64) * 4 + 255) & ~255
    rec = ((max_len + 2) * 4 + 255) & ~255
    return ck + rows + rec


CHUNK_WS = 4 << 30  # gdsm_nw_diff_batch: at most this much workspace per launch


@pytest.mark.parametrize("case", ["lds", "global_b"])
def test_batch_cut_into_chunks(case):
    """A max_len far above the strings sets the workspace strides and makes the launcher cut the
    batch (first_pair > 0, slots reused from chunk to chunk)."""
    rng = np.random.default_rng(31)
    if case == "lds":
        max_len, n = 49136, 45
        dims = [tuple(int(v) for v in rng.integers(1, 1201, 2)) for _ in range(n)]
        for i, d in {2: (0, 900), 7: (1100, 0), 19: (0, 0), 20: (1200, 1200), 23: (700, 0),
                     39: (0, 1), 40: (513, 1199), 44: (1025, 64)}.items():
            dims[i] = d
        per_launch = [20, 20, 5]
        for f in (0, 20, 40):  # every chunk has multi-strip pairs
            assert sum(n1 > 512 for n1, _ in dims[f:f + 20]) >= 2
    else:
        max_len = 200000
        dims = [(3000, 2900), (0, 40), (1537, 700), (1, 3000)]
        per_launch = [1, 1, 1, 1]
    chunk = CHUNK_WS // _pair_ws_bytes(max_len)
    cuts = [min(chunk, len(dims) - f) for f in range(0, len(dims), max(chunk, 1))]
    assert cuts == per_launch, (chunk, _pair_ws_bytes(max_len))
    pairs = [(_rand(rng, n1, 4), _rand(rng, n2, 4)) for n1, n2 in dims]
    with ga.Context(1, arenas=()) as c:
        c.prof_enable()
        got = c.nw_diff_batch(pairs, max_len=max_len)
        prof = c.prof_read()
        assert prof["nw_fill"][1] == len(per_launch) and prof["nw_trace"][1] == len(per_launch)
        _check(pairs, got)
        assert c.nw_diff_batch(pairs) == got
        assert c.prof_read()["nw_fill"][1] == 1


def test_b_staging_switch(ctx):
    """max_len 49136 is the last at which the fill stages b in LDS; 49137 reads it from global
    memory. The same pair, as long as the staging allows, through both."""
    rng = np.random.default_rng(41)
    a, b = _rand(rng, 60, 4), _rand(rng, 49136, 4)
    want = [oracle.nw_diff(a, b)]
    assert ctx.nw_diff_batch([(a, b)], max_len=49136) == want
    assert ctx.nw_diff_batch([(a, b)], max_len=49137) == want


def test_outputs_touch_only_their_bytes(ctx):
    """Pair i owns |a_i| + |b_i| + 1 bytes at a_off[i] + b_off[i] + i of both outputs and writes
    its L_i alignment bytes and one NUL there; nothing else in the buffers changes."""
    rng = np.random.default_rng(51)
    dims = [(700, 650), (0, 30), (30, 0), (1100, 40), (40, 1100), (0, 0), (513, 512), (64, 65),
            (1, 1), (300, 299)]
    pairs = [(_rand(rng, n1, 4), _rand(rng, n2, 4)) for n1, n2 in dims]
    want = [oracle.nw_diff(a, b) for a, b in pairs]
    n = len(pairs)
    a_off = np.zeros(n + 1, np.uint64)
    b_off = np.zeros(n + 1, np.uint64)
    a_off[1:] = np.cumsum([n1 for n1, _ in dims])
    b_off[1:] = np.cumsum([n2 for _, n2 in dims])
    total = int(a_off[-1] + b_off[-1]) + n
    tail = 256  # room behind the last slot, watched as well
    ins = [np.frombuffer(b"".join(p[0] for p in pairs), np.uint8), a_off,
           np.frombuffer(b"".join(p[1] for p in pairs), np.uint8), b_off]
    bufs = [ctx.buffer(x.nbytes).upload(x) for x in ins]
    o1 = ctx.buffer(total + tail).upload(np.full(total + tail, 0xA5, np.uint8))
    o2 = ctx.buffer(total + tail).upload(np.full(total + tail, 0xA5, np.uint8))
    ol = ctx.buffer(8 * (n + 1)).upload(np.full(n + 1, 2**64 - 1, np.uint64))
    try:
        _lib.check(_lib.load().gdsm_nw_diff_batch(ctx.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr,
                                                  bufs[3].ptr, n, 1100, o1.ptr, o2.ptr, ol.ptr))
        h1, h2 = o1.download(np.uint8, total + tail), o2.download(np.uint8, total + tail)
        lens = ol.download(np.uint64, n + 1)
    finally:
        for x in (*bufs, o1, o2, ol):
            x.free()
    assert sum(len(w[0]) < n1 + n2 for w, (n1, n2) in zip(want, dims)) >= 6  # slots with slack
    assert lens.tolist() == [len(w[0]) for w in want] + [2**64 - 1]
    e1, e2 = (np.full(total + tail, 0xA5, np.uint8) for _ in range(2))
    for i, (w1, w2) in enumerate(want):
        o = int(a_off[i] + b_off[i]) + i
        assert len(w1) + 1 <= dims[i][0] + dims[i][1] + 1
        e1[o:o + len(w1) + 1] = np.frombuffer(w1 + b"\0", np.uint8)
        e2[o:o + len(w2) + 1] = np.frombuffer(w2 + b"\0", np.uint8)
    assert np.array_equal(h1, e1) and np.array_equal(h2, e2)


def test_diff_device_threshold(ctx):
    """gdsm_set_diff_device(ctx, min_cells): n1 * n2 below min_cells stays on the CPU."""
    rng = np.random.default_rng(61)
    below = (_rand(rng, 199, 4), _rand(rng, 200, 4))
    at = (_rand(rng, 200, 4), _rand(rng, 200, 4))
    ctx.prof_enable()
    ga.set_diff_device(ctx, 40000)
    try:
        assert ga.diff(*below) == oracle.nw_diff(*below)
        assert ctx.prof_read()["nw_fill"][1] == 0
        assert ga.diff(*at) == oracle.nw_diff(*at)
        assert ctx.prof_read()["nw_fill"][1] == 1
    finally:
        ga.set_diff_device(None)
        ctx.prof_enable(False)


def test_batch_argument_checks(ctx):
    """Refused or finished before any launch."""
    fn = _lib.load().gdsm_nw_diff_batch
    off = ctx.buffer(16).upload(np.zeros(2, np.uint64))
    buf = ctx.buffer(16)
    try:
        assert fn(ctx.handle, buf.ptr, off.ptr, buf.ptr, off.ptr, 1, (1 << 20) + 1, buf.ptr,
                  buf.ptr, buf.ptr) == -22
        assert fn(ctx.handle, buf.ptr, off.ptr, buf.ptr, off.ptr, 0, 64, None, None, None) == 0
        assert fn(ctx.handle, buf.ptr, off.ptr, buf.ptr, off.ptr, 1, 64, buf.ptr, buf.ptr,
                  None) == -22
    finally:
        off.free()
        buf.free()


@pytest.mark.parametrize("name", ["c1", "cl", "dense", "edge"])
def test_page_windows_against_reference_alignments(ctx, golden, name):
    """The GPU NW on every 1024-B page window the REFERENCE diff() aligned for the page-diff pins
    (tests/golden/c1_windows.npz, ref_windows.npz; made by oracle/_ref): config 1's, config 3's
    clustered, a dense set and the SPEC edge pages. Every window — the ones whose reference
    alignment has gaps included — gives the reference's alignment length and the crc32 of both
    alignment strings."""
    import zlib

    from tests.helpers import c1_windows, window_pages
    if name == "c1":
        g = golden["c1_windows"]
        L, crc = g["L"], g["crc"]
        t, c = c1_windows()
    else:
        L, crc = golden["ref_windows"][name + "_L"], golden["ref_windows"][name + "_crc"]
        t, c = window_pages(name, golden)
    tw, cw = t.reshape(-1, 1024), c.reshape(-1, 1024)
    got = ctx.nw_diff_batch([(tw[i].tobytes(), cw[i].tobytes()) for i in range(len(tw))])
    for i, (o1, o2) in enumerate(got):
        assert len(o1) == L[i] and [zlib.crc32(o1), zlib.crc32(o2)] == crc[i].tolist(), (name, i)
