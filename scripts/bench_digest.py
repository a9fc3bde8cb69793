"""gdsm_digest (SPEC §10) against the box's read ceiling, and gdsm_fetch_changed (SPEC §11) against
gdsm_fetch on the same lists, on one GPU.

    python scripts/bench_digest.py [--pages 1048576] [--loop-pages 262144] [--reps 11]
                                   [--only-digest] [--out FILE]

Digest run: one arena of --pages pages digested with no list (pages 0 .. n-1) and with a random
ascending half, each launch timed by GDSM_PROF_DIGEST (HIP events on the context stream) after a
warm-up; 4 KiB read per page, 16 B written. In the same run gdsm_probe_ceiling(GDSM_PROBE_READ)
measures the fastest plain read of two such arenas; the digest's bytes/s are reported as a share of
that.

Fetch run: 2 loopback ranks (threads of this process, one context each), --loop-pages pages homed
at each; every rank asks for a random half of all pages into CURRENT and TWIN, so about half of its
list is homed at the other rank. Before every timed call the destinations are reset so that 0 %,
50 % or 100 % of the entries are stale (CURRENT differs from the home copy in about 1 % of its
words), then gdsm_fetch_changed is timed by GDSM_PROF_FETCH, which spans the whole protocol, the
host's waits for the other rank included; gdsm_fetch on the same lists is timed the same way. The
loopback transport's sends are device-to-device copies, so the run shows the protocol's overhead
(digests, flags, the second host read) and the bytes it keeps off the transport, NOT a gain over
xGMI. Prints one JSON line."""
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


def bench_digest(args):
    n = args.pages
    rng = np.random.default_rng(1)
    with ga.Context(n, arenas=("twin", "current")) as ctx:
        ctx.gen_pages(seed=7, arenas=("twin", "current"))
        ctx.sync()
        best, med = C.c_float(0), C.c_float(0)
        check(lib().gdsm_probe_ceiling(ctx.handle, 0, ctx.arena_ptr("twin"),
                                       ctx.arena_ptr("current"), None, n, 5, C.byref(best),
                                       C.byref(med)), "gdsm_probe_ceiling")
        ceiling = 2 * n * 4096 / (best.value * 1e-3)
        pick = half(rng, n)
        ids = ctx.ids(pick)
        out = ctx.buffer(16 * n)
        rows = {}
        for name, lst, k in (("identity", None, n), ("random_half", ids, len(pick))):
            ctx.digest("current", lst, n=k, out=out)  # untimed warm-up
            ctx.sync()
            ctx.prof_enable(True)
            ms = []
            for _ in range(args.reps):
                ctx.digest("current", lst, n=k, out=out)
                t, launches = ctx.prof_read()["digest"]
                ms.append(t / max(launches, 1))
            ctx.prof_enable(False)
            t = statistics.median(ms) * 1e-3
            rows[name] = {"pages": k, "bytes_read": k * 4096, "ms_median": statistics.median(ms),
                          "ms_min": min(ms), "GBps": k * 4096 / t / 1e9,
                          "share_of_read_ceiling": k * 4096 / t / ceiling}
        # the two runs agree on the pages both digested (out holds the random half's)
        some = out.download(np.uint64, 2 * 64).reshape(64, 2)
        ctx.digest("current", None, n=n, out=out)
        ctx.sync()
        full = out.download(np.uint64, 2 * n).reshape(n, 2)
        ok = bool(np.array_equal(some, full[pick[:64]]))
    return {"pages": n, "read_ceiling_ms_best": best.value, "read_ceiling_GBps": ceiling / 1e9,
            **rows, "spot_check_ok": ok}


def bench_fetch(args):
    G, z = 2, args.loop_pages
    total = G * z
    rng = np.random.default_rng(2)
    ctxs = [ga.Context(total) for _ in range(G)]
    for r, c in enumerate(ctxs):
        # page p of TWIN / CURRENT is global page p; REPLICA page i of rank r is global page r*z + i
        # with the TWIN content: a TWIN page equals its home copy, a generated CURRENT page does not
        c.gen_pages(seed=20, arenas=("twin", "current"))
        c.gen_pages(seed=20, first_global=r * z, arenas=("replica",))
        c.sync()
    comms = exchange.Comm.loopback(ctxs)
    lists = [half(rng, total) for _ in range(G)]
    bufs = [c.ids(lists[r]) for r, c in enumerate(ctxs)]
    stale_pct = (0, 50, 100)
    # per rank and case: the entries that are to be fresh (equal to the home copy) before the call
    fresh = [[np.sort(rng.permutation(lists[r])[:len(lists[r]) * (100 - pct) // 100])
              .astype(np.uint32) for pct in stale_pct] for r in range(G)]
    fbufs = [[c.ids(f) if len(f) else None for f in fresh[r]] for r, c in enumerate(ctxs)]
    ms = [{"fetch": [], **{pct: [] for pct in stale_pct}} for _ in range(G)]
    stats = [{} for _ in range(G)]
    errs = []

    def timed(ctx, fn, into):
        ctx.sync()
        ctx.prof_enable(True)
        fn()
        t, k = ctx.prof_read()["fetch"]
        ctx.prof_enable(False)
        into.append(t / max(k, 1))

    def rank(r):
        try:
            ctx, comm, n = ctxs[r], comms[r], len(lists[r])
            st = ctx.buffer(32)
            exchange.fetch(ctx, comm, bufs[r], None, n, total)               # untimed warm-ups
            exchange.fetch_changed(ctx, comm, bufs[r], None, n, total, stats=st)
            for rep in range(args.reps):
                timed(ctx, lambda: exchange.fetch(ctx, comm, bufs[r], None, n, total),
                      ms[r]["fetch"])
                for k, pct in enumerate(stale_pct):
                    # every CURRENT page stale, then the fresh entries from their homes
                    ctx.gen_pages(seed=20, arenas=("current",))
                    exchange.fetch(ctx, comm, fbufs[r][k], None, len(fresh[r][k]), total,
                                   dst=("current",))
                    timed(ctx, lambda: exchange.fetch_changed(ctx, comm, bufs[r], None, n, total,
                                                              stats=st), ms[r][pct])
                    stats[r][pct] = [int(x) for x in st.download(np.uint64, 4)]
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=rank, args=(r,)) for r in range(G)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    stuck = any(t.is_alive() for t in th)
    if errs or stuck:
        raise RuntimeError(f"loopback fetch failed: {errs or 'a rank is stuck'}")
    # after the last call every listed page equals its home copy in both arenas
    p = int(lists[0][-1])
    ok = bool(np.array_equal(ctxs[0].download("current", p, 1),
                             ctxs[p // z].download("replica", p % z, 1)) and
              np.array_equal(ctxs[0].download("twin", p, 1), ctxs[0].download("current", p, 1)))
    remote = [int((lists[r] // z != r).sum()) for r in range(G)]
    for c in comms:
        c.close()
    for c in ctxs:
        c.close()
    cases = []
    for pct in stale_pct:
        moved = sum(stats[r][pct][0] for r in range(G))
        cases.append({"stale_pct": pct, "stats_per_rank": [stats[r][pct] for r in range(G)],
                      "ms_median_per_rank": [statistics.median(ms[r][pct]) for r in range(G)],
                      # ids 4 B + digest 16 B + flag 4 B per remote entry, 4 KiB per changed page
                      "transport_bytes": sum(remote) * 24 + moved * 4096})
    return {"ranks": G, "pages_per_rank": z, "fetched_per_rank": [len(x) for x in lists],
            "remote_per_rank": remote,
            "fetch": {"ms_median_per_rank": [statistics.median(ms[r]["fetch"]) for r in range(G)],
                      "transport_bytes": sum(remote) * (4 + 4096)},  # id out, page back
            "fetch_changed": cases, "transport": "loopback (device-to-device copies)",
            "spot_check_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1 << 20)
    ap.add_argument("--loop-pages", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--only-digest", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    result = {"bench": "digest", "device": "MI355X", "version": ga.version(), "reps": args.reps,
              "digest": bench_digest(args)}
    if not args.only_digest:
        result["fetch_changed"] = bench_fetch(args)
    print(json.dumps(result))
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
