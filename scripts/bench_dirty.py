"""gdsm_dirty_scan (SPEC §12) against the box's read ceiling and against what a caller without it
does today, a diff of the whole arena, on one GPU.

    python scripts/bench_dirty.py [--pages 1048576] [--reps 11] [--out FILE]

One context of --pages pages (TWIN and CURRENT) in three states: 0 %, 1 % and (all but the few the
generator leaves alone) 100 % of its pages written, each written page in about 1 % of its words.
Every figure is a median of --reps launches after a warm-up, timed by HIP events on the context's
stream. Per state: the scan of all pages (8 KiB read per entry: the page of either arena) and its
share of gdsm_probe_ceiling(GDSM_PROBE_READ) measured in the same run; gdsm_diff of all pages on
the same arenas into a stream sized by the scan's bound. At 1 %: the round's writer end both ways,
scan -> read the count on the host -> release(dirty list) (the host read is inside the timed span)
against release(all pages), with the bytes each leaves to exchange: stream + rec_off. The releases
run without RETWIN so that every repetition sees the same arenas. Prints one JSON line."""
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


def timed(stream, fn, reps):
    """Median and minimum ms of fn's work on `stream`, after one untimed call."""
    fn()
    stream.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n = args.pages
    rng = np.random.default_rng(3)
    with ga.Context(n, arenas=("twin", "current")) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        pages, pos, stats = ctx.buffer(4 * n), ctx.buffer(4 * n), ctx.buffer(16)

        def scan():
            check(lib().gdsm_dirty_scan(ctx.handle, ga.TWIN, ga.CURRENT, None, n, pages.ptr,
                                        pos.ptr, n, stats.ptr), "gdsm_dirty_scan")

        def read_stats():
            ctx.sync()
            return [int(x) for x in stats.download(np.uint64, 2)]

        ctx.gen_pages(seed=7, arenas=("twin", "current"))
        ctx.sync()
        best, med = C.c_float(0), C.c_float(0)
        check(lib().gdsm_probe_ceiling(ctx.handle, 0, ctx.arena_ptr("twin"),
                                       ctx.arena_ptr("current"), None, n, 5, C.byref(best),
                                       C.byref(med)), "gdsm_probe_ceiling")
        ceiling = 2 * n * 4096 / (best.value * 1e-3)
        keep = np.sort(rng.choice(n, n // 100, replace=False))
        rest = ctx.ids(np.setdiff1d(np.arange(n, dtype=np.uint32), keep.astype(np.uint32)))
        states = []
        for name in ("0pct", "1pct", "100pct"):
            if name == "0pct":
                ctx.twin()
            else:
                ctx.gen_pages(seed=7, arenas=("twin", "current"))
                if name == "1pct":
                    ctx.twin(rest)
            scan()
            count, bound = read_stats()
            row = {"state": name, "dirty_pages": count, "bound_bytes": bound}
            t = timed(stream, scan, args.reps)
            rate = 2 * n * 4096 / (t["ms_median"] * 1e-3)
            row["scan"] = {**t, "bytes_read": 2 * n * 4096, "GBps": rate / 1e9,
                           "share_of_read_ceiling": rate / ceiling}
            runs = ga.Runs(ctx, n, cap=max(bound, 16))
            ctx.diff(n=n, out=runs)
            stream_bytes = runs.total()  # (also tells the diff the density it picks its geometry by)
            row["diff_all"] = {**timed(stream, lambda: ctx.diff(n=n, out=runs), args.reps),
                               "stream_bytes": stream_bytes, "rec_off_bytes": 8 * (n + 1)}
            row["scan_over_diff_all"] = row["scan"]["ms_median"] / row["diff_all"]["ms_median"]
            if name == "1pct":
                some = ga.Runs(ctx, count, cap=max(bound, 16))

                def scan_release():
                    scan()
                    k, _ = read_stats()
                    ctx.release(pages, n=k, out=some, retwin=False)

                row["scan_then_release_dirty"] = {
                    **timed(stream, scan_release, args.reps),
                    "stream_bytes": some.total(), "rec_off_bytes": 8 * (count + 1),
                    "id_list_bytes": 4 * count}
                row["release_all"] = {
                    **timed(stream, lambda: ctx.release(n=n, out=runs, retwin=False), args.reps),
                    "stream_bytes": runs.total(), "rec_off_bytes": 8 * (n + 1),
                    "id_list_bytes": 4 * n}
                # (the generator leaves a few pages unwritten, so the list may be a little shorter)
                got = pages.download(np.uint32, count)
                row["dirty_list_ascending_within_the_written_pages"] = bool(
                    np.isin(got, keep).all() and (np.diff(got.astype(np.int64)) > 0).all())
                some.free()
            runs.free()
            states.append(row)
        clean = states[0]["scan_over_diff_all"]
    result = {"bench": "dirty_scan", "device": "MI355X", "version": ga.version(),
              "reps": args.reps, "pages": n, "read_ceiling_ms_best": best.value,
              "read_ceiling_GBps": ceiling / 1e9, "states": states,
              "clean_scan_over_diff": clean, "clean_scan_within_1p10_of_diff": clean <= 1.10}
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
