"""gdsm_coh_clean and gdsm_coh_lookup (SPEC §15) against the page-table sweeps on the same table and
against the box's read ceiling over the bytes a call touches, on one GPU.

    python scripts/bench_cohlist.py [--pages 16777216] [--reps 11] [--out FILE]

One page-table-only context of --pages pages, 2 nodes, every page written by node 0 (a GPU
coherence batch: EXCLUSIVE, owned by node 0, dirty). Three lists of global pages on the device:
  all        every page, ascending;
  eighth     every eighth page, ascending;
  perm_1m    a random permutation of 2^20 distinct pages.
Per list, each figure a median of --reps calls after a warm-up, each call timed by HIP events on the
context's stream with no host synchronisation inside the timed span:
  clean_all_dirty   gdsm_coh_clean(node 0) with status_out and stats: every entry is owned dirty, so
                    every entry issues the atomic; the batch puts the table back before every call,
                    outside the timed span;
  clean_none_dirty  the same call on the cleaned table: every entry ALREADY, no atomic;
  lookup            gdsm_coh_lookup(shift 0, mask ~0) with faults_out.
The difference of the two cleans is what the 32-bit atomics cost. Yardsticks on the same table in
the same process: gdsm_coh_retire wet and dry (node 0 leaves: every page moves; no list is emitted)
and gdsm_coh_select of all pages (count only and listed); and gdsm_probe_ceiling(GDSM_PROBE_READ)
over as many bytes as the call touches nominally: 4 n of list, 8 n of table words and the outputs
(n status bytes; 8 n for lookup). A sparse list touches more of the table than that in whole cache
lines; the share is then below what the bytes moved would give. Prints one JSON line."""
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
    rng = np.random.default_rng(1)
    lists = {"all": np.arange(n, dtype=np.uint32),
             "eighth": np.arange(0, n, 8, dtype=np.uint32),
             "perm_1m": rng.permutation(n)[:min(n, 1 << 20)].astype(np.uint32)}
    with ga.Context(n, arenas=()) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        h = ctx.handle
        ev = ctx.gen_events(np.ones(n, np.uint64), seed=2, n_nodes=1, write_pct=100)

        def dirty_table():
            ctx.coh_init(2)
            ctx.coherence_batch(ev)

        status, out, fl = ctx.buffer(n), ctx.buffer(4 * n), ctx.buffer(4 * n)
        tot = ctx.buffer(32)

        def totals(words):
            ctx.sync()
            return [int(x) for x in tot.download(np.uint64, words)]

        def ceiling(nbytes):
            pages = max(1, nbytes // 2 // 4096)
            a, b = ctx.buffer(pages * 4096), ctx.buffer(pages * 4096)
            best, med = C.c_float(0), C.c_float(0)
            check(lib().gdsm_probe_ceiling(h, 0, a.ptr, b.ptr, None, pages, 11, C.byref(best),
                                           C.byref(med)), "gdsm_probe_ceiling")
            a.free()
            b.free()
            return {"bytes": 2 * pages * 4096, "ms_best": best.value, "ms_median": med.value}

        rows = {}
        ok = True
        for name, ids in lists.items():
            m = len(ids)
            d_ids = ctx.ids(ids)

            def clean():
                check(lib().gdsm_coh_clean(h, 0, d_ids.ptr, m, 0, status.ptr, tot.ptr, 0),
                      "gdsm_coh_clean")

            def lookup():
                check(lib().gdsm_coh_lookup(h, d_ids.ptr, m, 0, 0, 0xFFFFFFFF, out.ptr, fl.ptr),
                      "gdsm_coh_lookup")

            row = {"entries": m}
            row["clean_all_dirty"] = timed(stream, clean, reps, dirty_table)
            ok &= totals(4) == [m, 0, 0, 0]
            row["clean_none_dirty"] = timed(stream, clean, reps)
            ok &= totals(4) == [0, m, 0, 0]
            row["lookup"] = timed(stream, lookup, reps)
            ctx.sync()
            ok &= bool((out.download(np.uint32, 4) == 0x20001).all())   # EXCLUSIVE, node 0, clean
            row["atomics_ms"] = (row["clean_all_dirty"]["ms_median"] -
                                 row["clean_none_dirty"]["ms_median"])
            for call, nbytes in (("clean", 13 * m), ("lookup", 20 * m)):
                c = ceiling(nbytes)
                row["read_ceiling_" + call] = c
                for k in ("clean_all_dirty", "clean_none_dirty") if call == "clean" else ("lookup",):
                    row[k]["read_ceiling_over_call"] = c["ms_median"] / row[k]["ms_median"]
                    row[k]["nominal_GBps"] = nbytes / (row[k]["ms_median"] * 1e-3) / 1e9
            rows[name] = row
            d_ids.free()

        # the sweeps on the same table (8 B read per page; the wet retire stores 4 B per page)
        def sel(lst):
            check(lib().gdsm_coh_select(h, 0, 0, 0, 0, n, out.ptr if lst else None,
                                        n if lst else 0, tot.ptr), "gdsm_coh_select")

        def ret(flags):
            check(lib().gdsm_coh_retire(h, 0, 1, 0, 0, 0, n, None, 0, tot.ptr, flags),
                  "gdsm_coh_retire")

        sweeps = {"retire_wet": timed(stream, lambda: ret(0), reps, dirty_table)}
        ok &= totals(3) == [n, n, n]
        dirty_table()
        sweeps["retire_dry"] = timed(stream, lambda: ret(1), reps)
        ok &= totals(3) == [n, n, n]
        sweeps["select_all_count"] = timed(stream, lambda: sel(False), reps)
        sweeps["select_all_listed"] = timed(stream, lambda: sel(True), reps)
        ok &= totals(1) == [n]
        sweeps["read_ceiling_table"] = ceiling(8 * n)
        ev.free()
    return {"pages": n, "lists": rows, "sweeps": sweeps, "totals_ok": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    result = {"bench": "cohlist", "device": torch.cuda.get_device_name(0), "version": ga.version(),
              "reps": args.reps, **bench(args.pages, args.reps)}
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
