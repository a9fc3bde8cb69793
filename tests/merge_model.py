"""Numpy restatement of docs/SPEC.md §8 (gdsm_merge), written from the SPEC text and independent
of the kernel: K diff streams in priority order, joined by page id, composed byte by byte into one
canonical stream, with the bytes where the inputs overlapped and where they disagreed counted."""
from __future__ import annotations

import numpy as np

PAGE = 4096
MAX_RUNS = 2048


def parse_record(rec: np.ndarray):
    """(cov bool[4096], val uint8[4096]) of one record, (None, None) for an empty one, or the
    string "bad" for a record gdsm_apply refuses (SPEC §4)."""
    size = len(rec)
    if size == 0:
        return None, None
    if size < 4 or size % 4:
        return "bad", None
    nr = int(rec[:4].view("<u4")[0])
    if nr == 0 or nr > MAX_RUNS or size < 4 + 4 * nr:
        return "bad", None
    hdr = rec[4:4 + 4 * nr].view("<u4")
    off = (hdr & 0xFFFF).astype(np.int64)
    ln = (hdr >> 16).astype(np.int64)
    end = off + ln
    if (ln == 0).any() or (end > PAGE).any() or (off[1:] < end[:-1]).any():
        return "bad", None
    total = int(ln.sum())
    if size != 4 + 4 * nr + (total + 3) // 4 * 4:
        return "bad", None
    cov = np.zeros(PAGE, bool)
    val = np.zeros(PAGE, np.uint8)
    # sorted, non-overlapping runs: the payload is the covered bytes in position order
    marks = np.zeros(PAGE + 1, np.int32)
    np.add.at(marks, off, 1)
    np.add.at(marks, end, -1)
    cov[:] = np.cumsum(marks[:PAGE]) > 0
    val[cov] = rec[4 + 4 * nr:4 + 4 * nr + total]
    return cov, val


def build_record(cov: np.ndarray, val: np.ndarray) -> bytes:
    """The SPEC §3 record whose runs are the maximal ranges of cov, payload val."""
    if not cov.any():
        return b""
    edges = np.diff(np.concatenate([[0], cov.astype(np.int8), [0]]))
    starts = np.flatnonzero(edges == 1)
    ends = np.flatnonzero(edges == -1)
    hdr = (starts | ((ends - starts) << 16)).astype("<u4")
    pay = val[cov].tobytes()
    pay += b"\0" * (-len(pay) % 4)
    return np.array([len(starts)], "<u4").tobytes() + hdr.tobytes() + pay


def _offsets_ok(rec_off, cap) -> bool:
    ro = np.asarray(rec_off, np.uint64)
    return bool(ro[0] == 0 and (ro[1:] >= ro[:-1]).all() and not (ro & np.uint64(3)).any()
                and int(ro[-1]) <= cap)


def _ascending(a) -> bool:
    a = np.asarray(a, np.int64)
    return bool((a[1:] > a[:-1]).all())


def merge_ex(streams, ids=None, out_ids=None, n_out=None, caps=None):
    """streams: [(rec_off, data)] in priority order (a later stream wins); ids: per stream a page
    list or None; out_ids: the out page list or None (identity over n_out entries, default the
    first stream's record count). -> (rec_off, data, conflicts[n_out], overlap_total,
    conflict_total, invalid); invalid = the next sync reports -EINVAL. An offset array or page list
    that fails its check empties the whole output."""
    K = len(streams)
    ids = [None] * K if ids is None else list(ids)
    if out_ids is None:
        n_out = len(streams[0][0]) - 1 if n_out is None else n_out
        pages = np.arange(n_out, dtype=np.int64)
    else:
        pages = np.asarray(out_ids, np.int64)
        n_out = len(pages)
    empty = (np.zeros(n_out + 1, np.uint64), np.zeros(0, np.uint8), np.zeros(n_out, np.uint32), 0, 0,
             True)
    if not _ascending(pages):
        return empty
    where = []
    for k, (ro, data) in enumerate(streams):
        cap = len(data) if caps is None else caps[k]
        if not _offsets_ok(ro, cap):
            return empty
        n = len(ro) - 1
        if ids[k] is None:
            assert n == n_out and out_ids is None or n == n_out
            where.append({int(p): i for i, p in enumerate(pages)} if out_ids is not None
                         else {i: i for i in range(n)})
        else:
            if not _ascending(ids[k]):
                return empty
            where.append({int(p): i for i, p in enumerate(ids[k])})
    invalid = False
    recs, conflicts = [], np.zeros(n_out, np.uint32)
    ov_total = cf_total = 0
    for i, p in enumerate(pages):
        cov = np.zeros(PAGE, bool)
        win = np.zeros(PAGE, np.uint8)
        ncov = np.zeros(PAGE, np.int32)
        differ = np.zeros(PAGE, bool)
        first = np.zeros(PAGE, np.uint8)
        for k, (ro, data) in enumerate(streams):
            # a stream without a list holds out entry i's record at i
            r = i if ids[k] is None else where[k].get(int(p))
            if r is None:
                continue
            c, v = parse_record(np.asarray(data[int(ro[r]):int(ro[r + 1])], np.uint8))
            if isinstance(c, str):
                invalid = True
                continue
            if c is None:
                continue
            fresh = c & ~cov
            first[fresh] = v[fresh]
            differ |= c & cov & (v != first)
            ncov += c
            win[c] = v[c]
            cov |= c
        recs.append(build_record(cov, win))
        ov_total += int((ncov >= 2).sum())
        conflicts[i] = int(differ.sum())
        cf_total += int(differ.sum())
    rec_off = np.zeros(n_out + 1, np.uint64)
    if recs:
        rec_off[1:] = np.cumsum([len(r) for r in recs])
    return (rec_off, np.frombuffer(b"".join(recs), np.uint8).copy(), conflicts, ov_total, cf_total,
            invalid)


def merge(streams, ids=None, out_ids=None, n_out=None, caps=None):
    """-> (rec_off, data, conflicts[n_out], overlap_total, conflict_total)."""
    return merge_ex(streams, ids, out_ids, n_out, caps)[:5]


def writer_streams(n, K, mode, ppm, oracle):
    """The K writers of the overlap recipe: twin from gen_pages(n, seed=7); writer k changes the
    bytes that gen_pages(n, seed=100+k) changes, to that generator's bytes.
    -> (twin, [CURRENT_k], [(rec_off, data)])."""
    twin, _ = oracle.gen_pages(n, seed=7, mode=mode, ppm=ppm)
    curs, streams = [], []
    for k in range(K):
        t2, c2 = oracle.gen_pages(n, seed=100 + k, mode=mode, ppm=ppm)
        cur = np.where(t2 != c2, c2, twin)
        curs.append(cur)
        streams.append(oracle.diff_pages(twin, cur))
    return twin, curs, streams
