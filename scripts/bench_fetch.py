"""gdsm_fetch (SPEC §9) on one GPU: the local path against the box's copy ceiling, and a 2-rank
loopback fetch.

    python scripts/bench_fetch.py [--pages 1048576] [--loop-pages 262144] [--reps 11] [--out FILE]

Local path: a one-rank communicator, so every page is homed at the caller and goes arena to arena
(no staging, no transfer): a random ascending half of the arena's pages from REPLICA into CURRENT
and TWIN, 4 KiB read + 8 KiB written per page, timed by GDSM_PROF_FETCH. In the same run
gdsm_probe_ceiling(GDSM_PROBE_COPY) measures the fastest plain copy of the same arena (4 KiB read +
4 KiB written per page); the fetch's bytes/s are reported as a share of that. 2-rank loopback: two
contexts as threads of this process, each asking for a random half of all pages, so about half of
each list crosses the (device-to-device copy) transport through both staging buffers; its
GDSM_PROF_FETCH span includes the host's waits for the other rank. Prints one JSON line."""
import argparse
import ctypes as C
import json
import statistics
import sys
import threading
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import gallocy_amd as ga  # noqa: E402
from gallocy_amd import exchange  # noqa: E402
from gallocy_amd.gdsm import check, lib  # noqa: E402


def half(rng, total):
    return np.sort(rng.choice(total, total // 2, replace=False)).astype(np.uint32)


def bench_local(args):
    n = args.pages
    rng = np.random.default_rng(1)
    with ga.Context(n) as ctx:
        ctx.gen_pages(seed=7, arenas=("twin", "current", "replica"))
        ctx.sync()
        best, med = C.c_float(0), C.c_float(0)
        check(lib().gdsm_probe_ceiling(ctx.handle, 1, ctx.arena_ptr("replica"), None,
                                       ctx.arena_ptr("current"), n, 5, C.byref(best),
                                       C.byref(med)), "gdsm_probe_ceiling")
        copy_Bps = 2 * n * 4096 / (best.value * 1e-3)
        comm = exchange.Comm.loopback([ctx])[0]
        pages = half(rng, n)
        ids = ctx.ids(pages)
        exchange.fetch(ctx, comm, ids, None, len(pages), n)  # untimed warm-up
        ctx.sync()
        ctx.prof_enable(True)
        ms = []
        for _ in range(args.reps):
            exchange.fetch(ctx, comm, ids, None, len(pages), n)
            t, k = ctx.prof_read()["fetch"]
            ms.append(t / max(k, 1))
        ctx.prof_enable(False)
        ok = bool(np.array_equal(ctx.download("current", int(pages[5]), 1),
                                 ctx.download("replica", int(pages[5]), 1)))
        comm.close()
    moved = len(pages) * 3 * 4096
    t = statistics.median(ms) * 1e-3
    return {"pages": n, "fetched": len(pages), "bytes_moved": moved,
            "fetch_ms_median": statistics.median(ms), "fetch_ms_min": min(ms),
            "fetch_TBps": moved / t / 1e12, "copy_ceiling_ms_best": best.value,
            "copy_ceiling_TBps": copy_Bps / 1e12, "share_of_copy_ceiling": moved / t / copy_Bps,
            "spot_check_ok": ok}


def bench_loopback(args):
    G, z = 2, args.loop_pages
    total = G * z
    rng = np.random.default_rng(2)
    ctxs = [ga.Context(total) for _ in range(G)]
    for r, c in enumerate(ctxs):
        c.gen_pages(seed=20 + r, arenas=("twin", "current", "replica"))
        c.sync()
    comms = exchange.Comm.loopback(ctxs)
    lists = [half(rng, total) for _ in range(G)]
    bufs = [c.ids(lists[r]) for r, c in enumerate(ctxs)]
    ms = [[] for _ in range(G)]
    errs = []

    def rank(r):
        try:
            ctx = ctxs[r]
            exchange.fetch(ctx, comms[r], bufs[r], None, len(lists[r]), total)
            ctx.sync()
            ctx.prof_enable(True)
            for _ in range(args.reps):
                exchange.fetch(ctx, comms[r], bufs[r], None, len(lists[r]), total)
                t, k = ctx.prof_read()["fetch"]
                ms[r].append(t / max(k, 1))
            ctx.prof_enable(False)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    stuck = any(t.is_alive() for t in th)
    if errs or stuck:
        raise RuntimeError(f"loopback fetch failed: {errs or 'a rank is stuck'}")
    remote = [int((lists[r] // z != r).sum()) for r in range(G)]
    for c in comms:
        c.close()
    for c in ctxs:
        c.close()
    return {"ranks": G, "pages_per_rank": z, "fetched_per_rank": [len(x) for x in lists],
            "remote_per_rank": remote,
            "fetch_ms_median_per_rank": [statistics.median(m) for m in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1 << 20)
    ap.add_argument("--loop-pages", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    result = {"bench": "fetch", "device": "MI355X", "version": ga.version(), "reps": args.reps,
              "local": bench_local(args), "loopback": bench_loopback(args)}
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
