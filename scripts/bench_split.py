"""gdsm_runs_split (SPEC §13) against the box's copy ceiling and against what a caller without it
does today, on one GPU.

    python scripts/bench_split.py [--pages 1048576] [--reps 11] [--out FILE] [--only CASE]

One context of --pages pages. Every kernel figure is a median of --reps calls of the raw entry point
(no host synchronisation inside) after a warm-up, timed by HIP events on the context's stream, and
given as GB/s of the bytes the call has to move: the input's data, offsets and ids read once, every
output's data, offsets and ids written; next to it the data alone (input read + outputs written)
and the share of gdsm_probe_ceiling(GDSM_PROBE_COPY) measured in the same process.
  release_by_home   the diff stream of all --pages pages at 1 % word writes (records of about
                    66 B) into 8 homes;
  dense_by_home     a synthetic stream of 4104-B records of about the same total size into 8 homes;
  broadcast_2 / _8  the release's stream, every record to 2 and to 8 destinations (mask form).
Then the sparse release's writer end both ways, by the host clock around work that ends in a
synchronise, for the list of all pages in order: today (download the list, cut it by home on the
host, 8 gdsm_diff launches over the sublists) against gdsm_diff of the list + gdsm_runs_split
(whose one host read is inside).
--only CASE runs that one kernel case alone (for a kernel trace of it). Prints one JSON line."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import gallocy_amd as ga  # noqa: E402
from gallocy_amd.gdsm import check, lib  # noqa: E402

G = 8


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


def host_timed(ctx, fn, reps):
    """Median and minimum ms by the host clock of fn followed by a synchronise."""
    fn()
    ctx.sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms)}


class RawSplit:
    """gdsm_runs_split_raw on the context's stream into outputs sized once for the worst case."""

    def __init__(self, ctx, rec_off, data, cap, n, out_cap):
        self.ctx, self.n = ctx, n
        self.rec_off, self.data, self.cap = rec_off, data, cap
        self.o_ro = [ctx.buffer(8 * (n + 1)) for _ in range(G)]
        self.o_data = [ctx.buffer(max(out_cap, 16)) for _ in range(G)]
        self.o_ids = [ctx.buffer(4 * max(n, 1)) for _ in range(G)]
        self.counts = ctx.buffer(16 * G)
        self.ws_bytes = lib().gdsm_runs_split_workspace_bytes(n, G)
        self.ws = ctx.buffer(self.ws_bytes)
        self.p_ro = (C.c_void_p * G)(*[b.ptr for b in self.o_ro])
        self.p_data = (C.c_void_p * G)(*[b.ptr for b in self.o_data])
        self.p_ids = (C.c_void_p * G)(*[b.ptr for b in self.o_ids])
        self.caps = (C.c_uint64 * G)(*([out_cap] * G))
        self.ncaps = (C.c_uint64 * G)(*([n] * G))

    def __call__(self, ids, dest, per, g):
        check(lib().gdsm_runs_split_raw(self.rec_off, self.data, self.cap, ids, dest, per, self.n,
                                        g, self.p_ro, self.p_data, self.caps, self.ncaps,
                                        self.p_ids, self.counts.ptr, None, 0, self.ws.ptr,
                                        self.ws_bytes, self.ctx.stream), "gdsm_runs_split_raw")

    def read_counts(self, g):
        self.ctx.sync()
        return self.counts.download(np.uint64, 2 * G).reshape(G, 2)[:g]

    def free(self):
        for b in (*self.o_ro, *self.o_data, *self.o_ids, self.counts, self.ws):
            b.free()


def case(name, stream, sp, ids, dest, per, g, total_in, with_ids, reps, ceiling):
    sp(ids, dest, per, g)
    counts = sp.read_counts(g)
    recs, out_bytes = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    t = timed(stream, lambda: sp(ids, dest, per, g), reps)
    data_bytes = total_in + out_bytes
    moved = (data_bytes + 8 * (sp.n + 1) + (4 * sp.n if with_ids else 0) + (4 * sp.n if dest else 0)
             + 8 * (recs + g) + 4 * recs)
    sec = t["ms_median"] * 1e-3
    return {"case": name, "records_in": sp.n, "destinations": g, "bytes_in": total_in,
            "records_out": recs, "bytes_out": out_bytes, "bytes_moved": moved, **t,
            "GBps": moved / sec / 1e9, "data_GBps": data_bytes / sec / 1e9,
            "share_of_copy_ceiling": moved / sec / ceiling}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="")
    args = ap.parse_args()

    def want(name):
        return not args.only or args.only == name

    n = args.pages
    per = -(-n // G)
    with ga.Context(n) as ctx:
        stream = torch.cuda.ExternalStream(ctx.stream)
        ctx.gen_pages(seed=7)
        ctx.sync()
        best, med = C.c_float(0), C.c_float(0)
        check(lib().gdsm_probe_ceiling(ctx.handle, 1, ctx.arena_ptr("twin"), None,
                                       ctx.arena_ptr("replica"), n, 5, C.byref(best),
                                       C.byref(med)), "gdsm_probe_ceiling")
        ceiling = 2 * n * 4096 / (best.value * 1e-3)
        # the release's stream and its page list
        runs = ga.Runs(ctx, n, cap=n * 256)
        ctx.diff(n=n, out=runs)
        total = runs.total()
        ids = ctx.ids(np.arange(n, dtype=np.uint32))
        rows = []
        sp = RawSplit(ctx, runs.s.rec_off, runs.s.data, runs.s.cap, n, total)
        if want("release_by_home"):
            rows.append(case("release_by_home", stream, sp, ids.ptr, None, per, G, total, True,
                             args.reps, ceiling))
        for g in (2, 8):
            if not want(f"broadcast_{g}"):
                continue
            dest = ctx.ids(np.full(n, (1 << g) - 1, np.uint32))
            rows.append(case(f"broadcast_{g}", stream, sp, ids.ptr, dest.ptr, 0, g, total, True,
                             args.reps, ceiling))
            dest.free()
        sp.free()
        # dense: 4104-B records, the same total size
        nd = max(G, total // 4104)
        d_ro = ctx.buffer(8 * (nd + 1)).upload(np.arange(nd + 1, dtype=np.uint64) * 4104)
        d_data = ctx.buffer(nd * 4104)
        check(lib().gdsm_memcpy_d2d(ctx.handle, d_data.ptr, ctx.arena_ptr("current"), nd * 4104),
              "gdsm_memcpy_d2d")
        sp = RawSplit(ctx, d_ro.ptr, d_data.ptr, nd * 4104, nd, -(-nd // G) * 4104)
        if want("dense_by_home"):
            rows.append(case("dense_by_home", stream, sp, None, None, -(-nd // G), G, nd * 4104,
                             False, args.reps, ceiling))
        sp.free()
        writer = None
        if not args.only:
            # the writer's end of the sparse release, both ways (host clock, synchronise inside)
            outs = [ga.Runs(ctx, per, cap=total // G + total // 16 + 4096) for _ in range(G)]
            oids = [ctx.buffer(4 * per) for _ in range(G)]
            host_list = np.empty(n, np.uint32)

            def today():
                check(lib().gdsm_memcpy_d2h(ctx.handle, host_list.ctypes.data, ids.ptr, 4 * n), "d2h")
                cuts = np.searchsorted(host_list, np.arange(G + 1, dtype=np.uint64) * per)
                for d in range(G):
                    c = int(cuts[d + 1] - cuts[d])
                    if c:
                        ctx.diff(ids.ptr + 4 * int(cuts[d]), n=c, out=outs[d])

            def with_split():
                ctx.diff(ids, n=n, out=runs)
                ctx.runs_split(runs, ids=ids, per=per, G=G, outs=list(zip(outs, oids)))

            t_today = host_timed(ctx, today, args.reps)
            today_bytes = sum(o.total() for o in outs)
            t_split = host_timed(ctx, with_split, args.reps)
            split_bytes = sum(o.total() for o in outs)
            t_diff = timed(stream, lambda: ctx.diff(ids, n=n, out=runs), args.reps)
            writer = {"today_download_cut_8_diffs": {**t_today, "stream_bytes": today_bytes},
                      "diff_then_split": {**t_split, "stream_bytes": split_bytes},
                      "diff_of_the_list_alone": t_diff,
                      "split_over_today": t_split["ms_median"] / t_today["ms_median"]}
    by_name = {r["case"]: r for r in rows}
    result = {"bench": "runs_split", "device": "MI355X", "version": ga.version(),
              "reps": args.reps, "pages": n, "copy_ceiling_ms_best": best.value,
              "copy_ceiling_GBps": ceiling / 1e9, "cases": rows, "writer_end": writer,
              "small_over_dense_rate":
                  by_name["release_by_home"]["GBps"] / by_name["dense_by_home"]["GBps"]
                  if not args.only else None}
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
