"""CPU checks of the C-ABI boundary (no GPU compute): libgdsm.so loads, exports every entry point
include/gdsm.h declares plus the legacy C++ `diff` symbol, and fails cleanly without a GPU."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "gdsm.h"


def declared_functions():
    text = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gdsm_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_header():
    from gallocy_amd import _lib
    lib = _lib.load()
    names = declared_functions()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm missing")
def test_legacy_diff_symbol_has_reference_mangling():
    from gallocy_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    # gallocy/include/gallocy/utils/diff.h:9-11, mangled name measured in SURVEY §8b
    assert re.search(r"\bT _Z4diffPKcmRPcS0_mS2_\b", out)
    for n in declared_functions():
        assert re.search(rf"\bT {n}\b", out), n


def test_legacy_diff_through_cxx_symbol():
    """Calls the C++-linkage `diff` exactly as test/test_diff.cpp does (char*& out-params)."""
    from gallocy_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, _lib.LEGACY_DIFF_SYMBOL)
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_char_p, C.c_size_t,
                   C.POINTER(C.c_char_p)]
    for a, b, o1, o2 in [(b"GGAATGG", b"ATG", b"GGAATGG", b"---AT-G"),
                         (b"FOO BOP BOOP", b"FOOO BOOP BOP", b"F-OO B-OP BOOP", b"FOOO BOOP B-OP")]:
        r1, r2 = C.c_char_p(), C.c_char_p()
        assert fn(a, len(a), C.byref(r1), b, len(b), C.byref(r2)) == 0
        assert (r1.value, r2.value) == (o1, o2)


def test_nw_diff_matches_reference_vectors(golden):
    import gallocy_amd as ga
    g = golden["nw_ref"]
    blob = g["blob"].tobytes()
    i = 0
    for n, m, L in g["lens"]:
        a, b = blob[i:i + n], blob[i + n:i + n + m]
        i += n + m
        assert ga.diff(a, b) == (blob[i:i + L], blob[i + L:i + 2 * L])
        i += 2 * L


def test_nw_diff_beyond_reference_limit():
    """The reference crashes from 1181 B on; ours aligns a whole 4 KiB page."""
    import gallocy_amd as ga
    rng = np.random.default_rng(3)
    a = bytes(rng.integers(1, 256, 4096, dtype=np.uint8))
    b = bytearray(a)
    b[100] ^= 0x11
    b[2000:2003] = b"xyz"
    o1, o2 = ga.diff(a, bytes(b))
    assert o1 == a and o2 == bytes(b)


def test_no_gpu_is_reported_not_crashed():
    from gallocy_amd import _lib
    lib = _lib.load()
    n = C.c_int(-1)
    rc = lib.gdsm_device_count(C.byref(n))
    if n.value > 0:
        pytest.skip("a GPU is visible")
    assert rc in (0, -19) and n.value == 0
    h = C.c_void_p()
    assert lib.gdsm_init(C.byref(h), 0, 16, 0) == -19  # -ENODEV
    assert lib.gdsm_sync(None) == -22


def test_workspace_sizing():
    """gdsm_diff_workspace_bytes(n) for the single-pass diff: a ticket counter and one 8-B
    look-back granule per 16 pages, then the spill pool sized for the smallest spill geometry
    (16 pages per wave, plus two workgroups for the partial units of split streams: a
    generation word per workgroup slot, up to 1280 workgroup slots of 4 x 24 KiB); non-decreasing
    in n. Short lists (<= 32768 pages, the 2-page geometry) get no spill pool unless a spill
    geometry is forced (gdsm_tune "diff_variant" 5-7); lists of <= 2048 pages take one page per
    wave (a granule per page)."""
    from gallocy_amd import _lib
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    slots = lambda n: min(1280, ((n + 15) // 16 + 3) // 4 + 2)  # noqa: E731
    for forced in (0, 7):
        assert lib.gdsm_tune(b"diff_variant", forced) == 0
        try:
            for n in (1, 1000, 32768, 32769, 1 << 20, 1 << 24):
                pool = slots(n) * 4 * 24576 if (n > 32768 or forced) else 0
                want = up(8 * (1 + max((n + 15) // 16, (min(n, 32768) + 1) // 2,
                                       min(n, 2048))) + 64) + up(4 * 1280) + pool
                assert lib.gdsm_diff_workspace_bytes(n) == want, (n, forced)
            sizes = [lib.gdsm_diff_workspace_bytes(n) for n in range(1, 200000, 997)]
            assert sizes == sorted(sizes)
        finally:
            lib.gdsm_tune(b"diff_variant", 0)
    assert lib.gdsm_diff_workspace_bytes(32768) < 1 << 20  # was ~50 MB with the pool


CALLER = Path(__file__).resolve().parents[1] / "oracle" / "_ref" / "legacy_caller"


@pytest.mark.skipif(not CALLER.exists(), reason="oracle/_ref/legacy_caller not built (no reference tree)")
def test_legacy_caller_on_gallocy_internal_heap():
    """A compiled C++ caller (oracle/legacy_caller.cpp, linked with the reference's own
    allocators/internal.cpp + utils/constants.cpp) installs internal_malloc / internal_free via
    gdsm_set_allocator, replays the three test/test_diff.cpp bodies through libgdsm's diff()
    symbol, checks every output lies in the internal heap's zone, and frees it with
    internal_free (gallocy/utils/diff.cpp:135-136, allocators/internal.cpp:31-57)."""
    import os

    from gallocy_amd import _lib
    # the library the other tests load (gallocy_amd/lib, or GDSM_LIB) comes first in the caller's
    # search, before the run path it was linked with
    libdir = str(_lib.LIB_PATH.parent)
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(
        [libdir] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]))
    r = subprocess.run([str(CALLER)], capture_output=True, text=True, timeout=120, env=env)
    if r.returncode == 127:  # the loader's own failure: say what it searched
        ldd = subprocess.run(["ldd", str(CALLER)], capture_output=True, text=True, env=env)
        r.stderr += f"\n{_lib.LIB_PATH} exists: {_lib.LIB_PATH.exists()}\n{ldd.stdout}{ldd.stderr}"
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("ok ")


def test_tune_rejects_measurement_only_variants():
    """Kernels that do not produce valid output, and the retired four-pass coherence path, are not
    selectable in the product library (they exist only in a -DGDSM_MEASURE build); the valid
    variants are."""
    from gallocy_amd import _lib
    L = _lib.load()
    for key, bad in ((b"coh_variant", 3), (b"coh_variant", 4), (b"coh_variant", -1),
                     (b"diff_variant", 9),
                     (b"apply_variant", 9), (b"no_such_knob", 0)):
        assert L.gdsm_tune(key, bad) == -22, (key, bad)
    for key, ok in ((b"diff_variant", 1), (b"diff_variant", 2), (b"diff_variant", 3),
                    (b"diff_variant", 4), (b"diff_variant", 5), (b"diff_variant", 6), (b"diff_variant", 7),
                    (b"diff_variant", 8),
                    (b"coh_variant", 0), (b"coh_variant", 1), (b"coh_variant", 2)):
        assert L.gdsm_tune(key, ok) == 0
    assert L.gdsm_tune(b"diff_variant", 0) == 0 and L.gdsm_tune(b"coh_variant", 0) == 0
    # the short-list and small-batch launch forms (all valid); kSkip only in measurement builds
    for key, bad in ((b"diff_skip", 1), (b"diff_solo_max", 17), (b"diff_chain", 5),
                     (b"coh_chain", 2), (b"coh_span", 8)):
        assert L.gdsm_tune(key, bad) == -22, (key, bad)
    for key, ok, default in ((b"diff_solo_max", 16, 0), (b"diff_chain", 3, 2), (b"coh_chain", 0, 1),
                             (b"coh_span", 2, 4)):
        assert L.gdsm_tune(key, ok) == 0 and L.gdsm_tune(key, default) == 0
    # gdsm_rounds' launch forms: -1 (automatic) / 0 / 1, and the LDS form's workgroup count
    # (0 = automatic, up to kRoundsLdsMaxWGs = 16)
    max_wgs = 16
    try:
        for key in (b"rounds_xcd", b"rounds_lds"):
            for bad in (-2, 2):
                assert L.gdsm_tune(key, bad) == -22, (key, bad)
            for ok in (-1, 0, 1):
                assert L.gdsm_tune(key, ok) == 0, (key, ok)
        for bad in (-1, max_wgs + 1):
            assert L.gdsm_tune(b"rounds_lds_wg", bad) == -22, bad
        for ok in (0, 3, max_wgs):
            assert L.gdsm_tune(b"rounds_lds_wg", ok) == 0, ok
    finally:
        for key, default in ((b"rounds_xcd", -1), (b"rounds_lds", -1), (b"rounds_lds_wg", 0)):
            assert L.gdsm_tune(key, default) == 0


@pytest.mark.skipif(bool(__import__("os").environ.get("GDSM_LIB")),
                    reason="the driver links the in-tree libgdsm.so, not a GDSM_LIB build")
def test_native_replay_driver_exports_its_loop():
    """libgdsm_replay.so (gallocy_amd/native/replay.cpp, config 5's C++ round loop over the C ABI)
    links the in-tree libgdsm.so and exports gdsm_replay_mmult and its two-thread form, which
    refuse null contexts before touching any."""
    from gallocy_amd.replay import native_driver
    d = native_driver()
    z = np.zeros(2, np.int64)
    for fn in (d.gdsm_replay_mmult, d.gdsm_replay_mmult_threads):
        assert fn(None, None, 0, 1, None, z.ctypes.data, None, None, None, z.ctypes.data, None,
                  z.ctypes.data, None, 1) == -22


def test_release_argument_checks():
    """gdsm_release refuses unknown flags and a target list without a target arena before it
    touches a context (-EINVAL), like the other entry points on a NULL context."""
    from gallocy_amd import _lib
    lib = _lib.load()
    runs = _lib.GdsmRuns()
    assert lib.gdsm_release(None, None, 0, C.byref(runs), -1, None, 0) == -22      # no context
    assert lib.gdsm_release(None, None, 0, C.byref(runs), 2, None, 2) == -22       # unknown flag
    ids = (C.c_uint32 * 1)(0)
    assert lib.gdsm_release(None, None, 0, C.byref(runs), -1, C.cast(ids, C.c_void_p), 1) == -22


def test_nw_diff_on_reference_page_windows(golden):
    """libgdsm's CPU NW (the legacy diff()'s host path) on every 1024-B page window the REFERENCE
    diff() aligned (c1_windows.npz, ref_windows.npz, oracle/_ref): same length and crc32 of both
    alignment strings, windows with gaps included."""
    import zlib

    import gallocy_amd as ga
    from tests.helpers import REF_WINDOW_SETS, c1_windows, window_pages
    sets = [("c1", *c1_windows(), golden["c1_windows"]["L"], golden["c1_windows"]["crc"])]
    for name in REF_WINDOW_SETS:
        sets.append((name, *window_pages(name, golden), golden["ref_windows"][name + "_L"],
                     golden["ref_windows"][name + "_crc"]))
    for name, t, c, L, crc in sets:
        tw, cw = t.reshape(-1, 1024), c.reshape(-1, 1024)
        for i in range(0, len(tw), 3 if name in ("c1", "cl") else 1):
            o1, o2 = ga.diff(tw[i].tobytes(), cw[i].tobytes())
            assert len(o1) == L[i] and [zlib.crc32(o1), zlib.crc32(o2)] == crc[i].tolist(), (name, i)
