"""CPU checks of the page digest (docs/SPEC.md §10) and of the conditional fetch's model (§11): the
SPEC's fixed vectors, the numpy model against a term-by-term restatement in python integers, the
sensitivity of both rows to small changes of a page, the model of gdsm_fetch_changed on a hand-made
case, and the immediate argument checks of gdsm_digest, gdsm_digest_raw and gdsm_fetch_changed,
which refuse before they touch a context or a GPU."""
import ctypes as C

import numpy as np

from tests import digest_model as dm
from tests import fetch_model as fm


def test_first_key():
    assert int(dm.KEYS[0]) == 0x5692161D
    assert len(dm.KEYS) == 1028 and int(dm.KEYS.max()) < 1 << 32


def test_fixed_vectors():
    cases = [(np.zeros(4096, np.uint8), 0x06397FB63BB6EAFD, 0xB3D0051BF22BF1EC),
             (np.full(4096, 0xFF, np.uint8), 0x06397DBCED7578A1, 0xB3D00323A05CEE0F),
             ((np.arange(4096) % 251).astype(np.uint8), 0x127E8BD480F46EB6, 0xE48810DA78C8F27B)]
    got = dm.digests(np.stack([c[0] for c in cases]))
    for (page, s0, s1), d in zip(cases, got):
        assert (int(d[0]), int(d[1])) == (s0, s1)
        assert dm.digest_scalar(page) == (s0, s1)


def test_numpy_model_equals_scalar_restatement():
    rng = np.random.default_rng(10)
    pages = rng.integers(0, 256, (5, 4096), dtype=np.uint8)
    pages[3, :2048] = 0xFF      # words whose key add wraps mod 2^32
    got = dm.digests(pages)
    assert got.shape == (5, 2) and got.dtype == np.uint64
    for p, d in zip(pages, got):
        assert (int(d[0]), int(d[1])) == dm.digest_scalar(p)
    # one page, any shape that holds 4096 bytes
    assert np.array_equal(dm.digests(pages[2]), got[2:3])


def perturbations(rng, page):
    """(name, changed copy) for each perturbation of the issue's list; every copy differs."""
    out = []
    for name, byte in (("bit in byte 0", 0), ("bit in byte 4095", 4095)):
        q = page.copy()
        q[byte] ^= np.uint8(1 << int(rng.integers(0, 8)))
        out.append((name, q))
    w = page.view("<u4")
    i = int(rng.integers(0, 512))
    q = page.copy()
    qw = q.view("<u4")
    qw[2 * i], qw[2 * i + 1] = w[2 * i + 1], w[2 * i]
    out.append(("the two u32 of a pair swapped", q))
    a, b = (int(x) for x in rng.choice(512, 2, replace=False))
    q = page.copy()
    q8 = q.view("<u8")
    q8[a], q8[b] = page.view("<u8")[b], page.view("<u8")[a]
    out.append(("two 8-B words swapped", q))
    q = page.copy()
    q[int(rng.integers(0, 4096))] ^= np.uint8(rng.integers(1, 256))
    out.append(("one random byte", q))
    out.append(("rotated by 16 bytes", np.roll(page, 16)))
    return out


def test_both_rows_change_under_small_perturbations():
    rng = np.random.default_rng(11)
    for _ in range(8):
        page = rng.integers(0, 256, 4096, dtype=np.uint8)
        base = dm.digests(page)[0]
        for name, q in perturbations(rng, page):
            assert not np.array_equal(q, page), name
            d = dm.digests(q)[0]
            assert d[0] != base[0] and d[1] != base[1], name


def test_model_fetch_changed_on_a_hand_made_case():
    """2 ranks, 6 pages (per = 3). Rank 0 asks for pages 1 (local, equal), 2 (local, differs),
    3 (remote, equal in A = CURRENT, TWIN differs) and 5 (remote, differs in its last byte)."""
    rng = np.random.default_rng(12)
    Z = 6
    rep = [rng.integers(0, 256, (Z, 4096), dtype=np.uint8) for _ in range(2)]
    arenas = [{a: rng.integers(0, 256, (Z, 4096), dtype=np.uint8) for a in ("current", "twin")}
              for _ in range(2)]
    arenas[0]["current"][1] = rep[0][1]
    arenas[0]["current"][3] = rep[1][0]
    arenas[0]["current"][5] = rep[1][2]
    arenas[0]["current"][5, 4095] ^= 1
    req = [np.array([1, 2, 3, 5]), np.zeros(0, np.int64)]
    out, changed, stats = dm.fetch_changed(rep, req, [None, None], arenas, Z)
    assert changed[0].tolist() == [0, 1, 0, 1] and changed[1].tolist() == []
    assert stats == [[1, 1, 1, 1], [0, 0, 0, 0]]
    want = fm.fetch(rep, req, [None, None], arenas, Z)
    for r in range(2):
        for a in ("current", "twin"):
            assert np.array_equal(out[r][a], want[r][a])
    assert np.array_equal(out[0]["twin"][3], rep[1][0])   # the skipped page still arrives clean
    # TWIN only: A is TWIN, whose copies all differ
    tw = [{"twin": x["twin"]} for x in arenas]
    _, changed, stats = dm.fetch_changed(rep, req, [None, None], tw, Z)
    assert changed[0].tolist() == [1, 1, 1, 1] and stats[0] == [2, 0, 2, 0]
    assert dm.first_arena(("twin", "current")) == "current" and dm.first_arena(("twin",)) == "twin"


def test_digest_argument_checks():
    from gallocy_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint64 * 4)()
    p = C.cast(buf, C.c_void_p)
    assert lib.gdsm_digest(None, 1, None, 0, None) == -22          # no context, whatever else
    assert lib.gdsm_digest(None, 1, None, 2, p) == -22
    assert lib.gdsm_digest(None, 7, p, 2, p) == -22
    assert lib.gdsm_digest_raw(None, None, 0, None, None) == -22   # no arena
    assert lib.gdsm_digest_raw(None, None, 2, p, None) == -22
    assert lib.gdsm_digest_raw(p, None, 2, None, None) == -22      # n without out
    assert list(buf) == [0, 0, 0, 0]


def test_fetch_changed_argument_checks():
    """As gdsm_fetch: a NULL context or communicator is refused at once (-EINVAL), whatever else
    is passed."""
    from gallocy_amd import _lib
    lib = _lib.load()
    ids = (C.c_uint32 * 2)(0, 1)
    p = C.cast(ids, C.c_void_p)
    fake = C.cast(ids, C.c_void_p)  # never dereferenced: the NULL argument is refused first
    assert lib.gdsm_fetch_changed(None, None, None, None, 0, 1, 2, 0, None, None) == -22
    assert lib.gdsm_fetch_changed(None, fake, p, None, 2, 8, 2, 0, None, None) == -22
    assert lib.gdsm_fetch_changed(fake, None, p, None, 2, 8, 2, 0, None, None) == -22
    assert lib.gdsm_fetch_changed(None, None, None, None, 2, 8, 2, 0, p, p) == -22
    assert lib.gdsm_fetch_changed(None, None, p, p, 2, 0, 7, 0xFF, None, None) == -22
