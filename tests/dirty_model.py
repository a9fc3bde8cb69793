"""numpy model of gdsm_dirty_scan (docs/SPEC.md §12): which list entries name a page that differs
between two arenas, in list order, with their number and the bound of their diff stream."""
import numpy as np

PAGE = 4096
CHUNK = 16
MAX_RECORD = 10244


def chunks_differing(a, b):
    """C per page of the arenas: its 16-B chunks in which a and b differ in at least one byte."""
    d = a.reshape(-1, PAGE // CHUNK, CHUNK) != b.reshape(-1, PAGE // CHUNK, CHUNK)
    return d.any(axis=2).sum(axis=1).astype(np.int64)


def dirty_scan(a, b, ids=None, n=None, n_pages=None):
    """(pages uint32[count], pos uint32[count], count, bound) of the list ids[0..n) (None: pages
    0 .. n-1) over the arenas a, b (uint8[Z, 4096]). An id >= n_pages (default Z) is not dirty."""
    Z = a.shape[0] if n_pages is None else n_pages
    if ids is None:
        ids = np.arange(a.shape[0] if n is None else n, dtype=np.int64)
    ids = np.asarray(ids, np.int64)[:n]
    valid = ids < Z
    C = np.zeros(len(ids), np.int64)
    C[valid] = chunks_differing(a[:Z], b[:Z])[ids[valid]]
    pos = np.flatnonzero(C > 0)
    bound = int(np.minimum(MAX_RECORD, 4 + 48 * C[pos]).sum())
    return ids[pos].astype(np.uint32), pos.astype(np.uint32), len(pos), bound
