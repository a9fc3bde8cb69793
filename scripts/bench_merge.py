"""gdsm_merge against the only route the library had to one combined stream before it: K
gdsm_apply calls onto a scratch arena holding the twin, then gdsm_diff against the twin.

    python scripts/bench_merge.py [--pages 1048576] [--K 2,8] [--reps 11] [--out FILE]
    python scripts/bench_merge.py --only-merge --K 8     # the merge alone (for a kernel trace)

K writer streams are made on the device: writer k's stream is the diff of SPEC §6 pages with seed
100 + k (config 3's shape, CLUSTERED 100 000 ppm), the twin is seed 7's. The two routes are timed
alternately in one run, each timing ending in gdsm_sync; the medians are reported. Route (b) also
needs the twin and reads 8 KiB per page; it is the time yardstick only (its stream differs from
the merge's wherever a writer restored a twin byte). The merge's algorithmic bytes (its inputs and
output once, offsets included) over the GDSM_PROF_MERGE time are printed as a share of 8 TB/s,
beside the box's read ceiling from gdsm_probe_ceiling in the same run. Prints one JSON line."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import gallocy_amd as ga  # noqa: E402
from gallocy_amd._lib import GdsmRuns  # noqa: E402
from gallocy_amd.gdsm import check, lib  # noqa: E402

PEAK = 8e12  # bytes/s, MI355X HBM3E


def writer_streams(ctx, K, n, mode, ppm, bpp):
    streams = []
    for k in range(K):
        ctx.gen_pages(seed=100 + k, mode=mode, ppm=ppm, arenas=("twin", "current"))
        r = ga.Runs(ctx, n, n * bpp)
        ctx.diff(out=r)
        r.bytes = r.total()
        streams.append(r)
    ctx.gen_pages(seed=7, mode=mode, ppm=ppm, arenas=("twin",))
    ctx.sync()
    return streams


def timed(fn, ctx):
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def bench_k(ctx, K, args, ceiling):
    n = args.pages
    streams = writer_streams(ctx, K, n, ga.GEN_CLUSTERED, 100000, args.bpp)
    in_bytes = sum(s.bytes for s in streams)
    merged = ga.Runs(ctx, n, in_bytes)
    scratch = ga.Runs(ctx, n, in_bytes)
    twin_p, cur_p = ctx.arena_ptr("twin"), ctx.arena_ptr("current")

    arr = (GdsmRuns * K)(*[s.s for s in streams])
    stats_buf = ctx.buffer(16)

    def route_a():  # the C ABI with buffers allocated once (Context.merge allocates per call)
        check(lib().gdsm_merge(ctx.handle, K, arr, None, None, n, C.byref(merged.s), None,
                               stats_buf.ptr), "gdsm_merge")

    def reset_b():  # the scratch arena holds the twin (not timed)
        check(lib().gdsm_memcpy_d2d(ctx.handle, cur_p, twin_p, n * 4096), "d2d")
        ctx.sync()

    def route_b():
        for s in streams:
            ctx.apply(s, "current")
        ctx.diff(out=scratch)

    route_a()  # untimed warm-up (sizes every workspace)
    ctx.sync()
    reset_b()
    route_b()
    ctx.sync()
    out_bytes, b_bytes = merged.total(), scratch.total()
    if args.only_merge:
        for _ in range(args.reps):
            route_a()
        ctx.sync()
        return {"K": K, "pages": n, "merged_bytes": out_bytes}
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(timed(route_a, ctx))
        reset_b()
        tb.append(timed(route_b, ctx))
    ctx.prof_enable(True)
    for _ in range(args.reps):
        route_a()
    ms, launches = ctx.prof_read()["merge"]
    ctx.prof_enable(False)
    route_a()
    ctx.sync()
    st = stats_buf.download(np.uint64, 2)
    stats = {"overlap_bytes": int(st[0]), "conflict_bytes": int(st[1])}
    algo = in_bytes + out_bytes + 8 * (n + 1) * (K + 1)  # streams and offsets once; no id lists
    prof_ms = ms / max(launches, 1)
    row = {"K": K, "pages": n, "input_bytes": in_bytes, "merged_bytes": out_bytes,
           "apply_diff_stream_bytes": b_bytes, **stats,
           "merge_ms_median": statistics.median(ta), "merge_ms_min": min(ta),
           "apply_diff_ms_median": statistics.median(tb), "apply_diff_ms_min": min(tb),
           "merge_not_slower": statistics.median(ta) <= statistics.median(tb),
           "prof_merge_ms": prof_ms, "algorithmic_bytes": algo,
           "algorithmic_TBps": algo / (prof_ms * 1e-3) / 1e12,
           "share_of_8TBps": algo / (prof_ms * 1e-3) / PEAK,
           "read_ceiling_TBps": ceiling}
    for r in (*streams, merged, scratch, stats_buf):
        r.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1 << 20)
    ap.add_argument("--K", default="2,8")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--bpp", type=int, default=1024, help="stream bytes allocated per page")
    ap.add_argument("--only-merge", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    with ga.Context(args.pages) as ctx:
        best, med = C.c_float(0), C.c_float(0)
        check(lib().gdsm_probe_ceiling(ctx.handle, 0, ctx.arena_ptr("twin"),
                                       ctx.arena_ptr("current"), None, args.pages, 5,
                                       C.byref(best), C.byref(med)), "gdsm_probe_ceiling")
        ceiling = 2 * args.pages * 4096 / (best.value * 1e-3) / 1e12
        rows = [bench_k(ctx, int(k), args, ceiling) for k in args.K.split(",")]
    result = {"bench": "merge", "device": "MI355X", "version": ga.version(), "reps": args.reps,
              "rows": rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
