"""bench.py on one GPU at a reduced page count: the plain run's line (the headline and the
per-stage times only) at N = 1 and with two ranks sharing the GPU, what --dump-outputs writes
(checked byte for byte against the C oracle's pages and diff stream), and the fields --full adds."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SEED = 11
FULL_ONLY = ("roofline", "step_hbm_gbs", "step_frac_of_box_read", "replica_equals_current",
             "cpu_baseline")


def _bench(*args, gpus=1):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", str(gpus), "--seed",
                        str(SEED), *args], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0])


# 5000: more pages than the dump samples, no multiple of the diff's pages per wave; 300: every
# page dumped. --overlap on with 2 steps: the last step's stream is the second of the two buffers.
@pytest.mark.parametrize("n,steps,extra", [(5000, 3, []), (300, 2, ["--overlap", "on"])])
def test_plain_run_line_and_dumped_outputs(tmp_path, n, steps, extra):
    d = _bench("--steps", str(steps), "--warmup", "1", "--total-pages", str(n),
               "--dump-outputs", str(tmp_path / "out"), *extra)
    assert d["metric"] == "pages diffed+applied/sec (4 KiB)" and d["unit"] == "pages/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u8" and d["n_gpus"] == 1
    assert d["steps"] == steps and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert d["stages"]["diff"]["launches"] == steps and d["stage_ms_per_step"]["diff"] > 0
    assert not [k for k in FULL_ONLY if k in d]
    assert "payload_bytes_per_step" not in d["config"]

    out = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert sorted(out) == ["diff_record_bytes", "diff_records", "diff_total_bytes",
                           "replica_pages", "sample_page_ids"]
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    ids = out["sample_page_ids"].astype(np.int64)
    assert len(ids) == n if n <= 1024 else 1024 <= len(ids) <= 1026
    assert ids[0] == 0 and ids[-1] == n - 1 and (np.diff(ids) > 0).all()
    twin, cur = oracle.gen_pages(n, seed=SEED, mode=0, ppm=10000)
    ro, data = oracle.diff_pages(twin, cur)
    assert np.array_equal(out["replica_pages"], cur[ids].astype(np.float32))
    assert out["diff_total_bytes"].tolist() == [float(ro[-1])] == [float(d["config"]["diff_bytes_per_step"])]
    assert np.array_equal(out["diff_record_bytes"], (ro[ids + 1] - ro[ids]).astype(np.float64))
    want = np.concatenate([data[int(ro[p]):int(ro[p + 1])] for p in ids])
    assert len(want) > 0 and np.array_equal(out["diff_records"], want.astype(np.float32))


def test_plain_run_two_ranks_dumps_rank_0_home_block(tmp_path, monkeypatch):
    """N = 2 without a launcher (two ranks on cuda:0 over the gloo rehearsal transport): the plain
    line, and rank 0's dumped REPLICA sample equals CURRENT of its home block, pages [0, n)."""
    monkeypatch.setenv("GDSM_BENCH_BACKEND", "gloo")
    n = 2 * 8192
    d = _bench("--steps", "2", "--warmup", "1", "--total-pages", str(2 * n),
               "--dump-outputs", str(tmp_path / "out"), gpus=2)
    assert d["n_gpus"] == 2 and d["full"] is False and d["ms_per_step"] > 0
    assert d["exchange"]["received_bytes_per_step"] > 0
    assert not [k for k in FULL_ONLY + ("same_run_reference", "roofline_xgmi") if k in d]
    out = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert sorted(out) == ["replica_pages", "sample_page_ids"]
    ids = out["sample_page_ids"].astype(np.int64)
    assert ids[0] == 0 and ids[-1] == n - 1 and 1024 <= len(ids) <= 1026
    _, cur = oracle.gen_pages(n, seed=SEED, mode=0, ppm=10000)
    assert np.array_equal(out["replica_pages"], cur[ids].astype(np.float32))


def test_full_run_adds_the_checks_and_ceilings():
    d = _bench("--steps", "2", "--warmup", "1", "--total-pages", "5000", "--full", "--no-cpu")
    assert d["full"] is True and d["replica_equals_current"] is True
    assert d["ms_per_step"] > 0 and d["cpu_baseline"] is None
    roof = d["roofline"]
    assert roof["box_read_gbs"] > 0 and roof["box_copy_gbs"] > 0 and roof["frac_of_box"] > 0
    assert d["step_hbm_gbs"] > 0 and d["step_frac_of_box_read"] > 0
    twin, cur = oracle.gen_pages(5000, seed=SEED, mode=0, ppm=10000)
    assert d["config"]["payload_bytes_per_step"] == int(np.count_nonzero(twin != cur))
