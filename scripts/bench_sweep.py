"""gdsm_coh_select and gdsm_coh_retire (SPEC §14) against the box's read ceiling over the same
number of bytes, on one GPU.

    python scripts/bench_sweep.py [--pages 16777216 67108864] [--reps 11] [--out FILE]

Per table size: one page-table-only context of that many pages, 8 nodes, as gdsm_coh_init leaves it
(every node owns an eighth of the pages, EXCLUSIVE). Every figure is a median of --reps calls after
a warm-up, each call timed by HIP events on the context's stream (as gdsm_probe_ceiling times its
launches), with no host synchronisation inside the timed span:
  select_none   (word & 0xFF) == 0x100: nothing selected (the flag and sum launches, an emit launch
                that finds every flag word empty);
  select_all    mask 0: every page listed (4 B written per page);
  select_count  mask 0 with no list: the flag and sum launches alone;
  retire_dry    node 0 leaves, heir 1: an eighth of the pages moved and listed, nothing stored;
  retire_wet    the same with the table updated; gdsm_coh_init puts the table back before every
                call, outside the timed span.
A sweep reads 8 B per page; its rate is reported as a share of gdsm_probe_ceiling(GDSM_PROBE_READ)
over two buffers of 4 n bytes each, measured in the same process. Prints one JSON line."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import gallocy_amd as ga  # noqa: E402
from gallocy_amd.gdsm import check, lib  # noqa: E402


def timed(stream, fn, reps, before=None):
    """Median and minimum ms of fn's work on `stream`, after one untimed call; `before` runs ahead
    of every call, outside the timed span."""
    ms = []
    for r in range(reps + 1):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms)}


def bench(n, reps):
    with ga.Context(n, arenas=()) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        ctx.coh_init(8)
        out, tot = ctx.buffer(4 * n), ctx.buffer(24)
        h = ctx.handle

        def sel(mask, value, lst=True):
            check(lib().gdsm_coh_select(h, mask, value, 0, 0, n, out.ptr if lst else None,
                                        n if lst else 0, tot.ptr), "gdsm_coh_select")

        def ret(flags):
            check(lib().gdsm_coh_retire(h, 0, 1, 0, 0, 0, n, out.ptr, n, tot.ptr, flags),
                  "gdsm_coh_retire")

        def total(words):
            ctx.sync()
            return [int(x) for x in tot.download(np.uint64, words)]

        # the read ceiling over the table's bytes: two buffers of n / 1024 pages
        probe_pages = max(1, n // 1024)
        a, b = ctx.buffer(probe_pages * 4096), ctx.buffer(probe_pages * 4096)
        best, med = C.c_float(0), C.c_float(0)
        check(lib().gdsm_probe_ceiling(h, 0, a.ptr, b.ptr, None, probe_pages, 11, C.byref(best),
                                       C.byref(med)), "gdsm_probe_ceiling")
        table_bytes = 8 * n
        cases = {
            "select_none": (lambda: sel(0xFF, 0x100), None, 1),
            "select_all": (lambda: sel(0, 0), None, 1),
            "select_count": (lambda: sel(0, 0, False), None, 1),
            "retire_dry": (lambda: ret(1), None, 3),
            "retire_wet": (lambda: ret(0), lambda: ctx.coh_init(8), 3),
        }
        rows = {}
        for name, (fn, before, words) in cases.items():
            t = timed(stream, fn, reps, before)
            rows[name] = {**t, "totals": total(words),
                          "GBps": table_bytes / (t["ms_median"] * 1e-3) / 1e9,
                          "read_ceiling_over_sweep": med.value / t["ms_median"]}
        first = out.download(np.uint32, 4).tolist()
        ok = (rows["select_none"]["totals"] == [0] and rows["select_all"]["totals"] == [n] and
              rows["retire_dry"]["totals"] == rows["retire_wet"]["totals"] and
              rows["retire_wet"]["totals"][1] == -(-n // 8) and first == [0, 1, 2, 3])
    return {"pages": n, "table_bytes": table_bytes, "read_ceiling_ms_best": best.value,
            "read_ceiling_ms_median": med.value,
            "read_ceiling_GBps": table_bytes / (best.value * 1e-3) / 1e9, **rows,
            "totals_ok": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, nargs="+", default=[1 << 24, 1 << 26])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    result = {"bench": "sweep", "device": torch.cuda.get_device_name(0), "version": ga.version(),
              "reps": args.reps, "tables": [bench(n, args.reps) for n in args.pages]}
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
