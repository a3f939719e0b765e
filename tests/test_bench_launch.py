"""bench.py's launch and exit-code contract on a CPU-only box (gloo, world 2), on the stand-in library (tests/standin_lib.py
through tests/standin/sitecustomize.py):
* `python bench.py --gpus 2 ...` WITHOUT a launcher environment starts its own ranks (python -m torch.distributed.run as a child
  process), relays rank 0's one JSON line and exits with the child's code - the reference's multi-GPU entry points are single
  commands too (reid/faiss_utils.py:121-135, image_reid_inference.py:211);
* a sub-workload that never comes back (a rank lost in a collective) ends the job through the watchdog with a NON-ZERO exit code
  after the partial line has been printed - at one rank and at two."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "standin")
SMALL = ["--crops", "8", "--steps", "1", "--warmup", "0", "--no-cpu", "--single"]


def _bench(args, timeout, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(REID_TEST_STANDIN="1", PYTHONPATH=STANDIN + os.pathsep + env.get("PYTHONPATH", ""), OMP_NUM_THREADS="2")
    env.update({k: str(v) for k, v in env_extra.items()})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)


def _one_line(r):
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, (r.stdout, r.stderr[-2000:])
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_bench_starts_its_own_ranks_when_no_launcher_did():
    r = _bench(["--gpus", "2", "--workload", "embed"] + SMALL, 280)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _one_line(r)
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert "RCCL all-gather" in out["config"]["sharding"]
    assert "torch.distributed.run" in r.stderr            # the self-launch notice


@pytest.mark.timeout(300)
def test_bench_refuses_a_launcher_that_disagrees_with_gpus():
    r = _bench(["--gpus", "2", "--workload", "embed"] + SMALL, 120, WORLD_SIZE=1, RANK=0, LOCAL_RANK=0)
    assert r.returncode == 2 and r.stdout.strip() == ""


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus,rank0_delay", [(1, 0.0), (2, 0.0), (2, 4.0)])
def test_lost_sub_workload_ends_the_job_with_a_nonzero_exit_code(gpus, rank0_delay):
    """batch256 (the second weight load of the --full line) never returns on the last rank: the watchdog prints what the headline
    measured, with the failure recorded in the sub-object, and every rank leaves with status 3.  Every rank's watchdog fires on its
    own clock and the launcher takes the others down as soon as one has left - so a rank other than 0 waits for rank 0's "line is
    out" flag first (for what is left of the sub-workload's limit plus a margin).  The order that used to lose the line is FORCED
    once instead of hoped for in five repetitions: rank 0's watchdog is held back by 4 s (REID_BENCH_TEST_RANK0_WATCHDOG_DELAY), so
    rank 1 notices first, and the partial line must still come out."""
    r = _bench(["--gpus", str(gpus), "--full"] + SMALL, 280, REID_STANDIN_HANG_AT_LOAD=2, REID_STANDIN_HANG_RANK=gpus - 1, REID_BENCH_LIMIT_SCALE=0.03,
               REID_BENCH_TEST_RANK0_WATCHDOG_DELAY=rank0_delay)
    assert r.returncode != 0, (r.stdout, r.stderr[-3000:])
    out = _one_line(r)
    assert out["value"] > 0 and "error" in out["batch256"]
    if gpus == 1:
        assert r.returncode == 3


@pytest.mark.timeout(300)
def test_plain_run_is_the_headline_alone():
    """Without --full the line is the headline's timed steps and nothing else: no side runs of the other arithmetic modes, no
    roofline or cpu_baseline, no sub-workloads; --full still adds them, and the other configurations are refused without it."""
    head = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"}
    small = ["--crops", "8", "--steps", "2", "--warmup", "1"]
    r = _bench(["--gpus", "1"] + small, 280)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _one_line(r)
    assert set(out) == head and out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["dtype"] == "f16x3"
    r = _bench(["--gpus", "1", "--full", "--workload", "embed", "--no-cpu"] + small, 280)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _one_line(r)
    assert head < set(out) and {"roofline", "f32_path", "f16_path", "f16x3_vs_f32"} <= set(out)
    r = _bench(["--gpus", "1", "--workload", "swin"] + small, 60)
    assert r.returncode == 2 and r.stdout.strip() == "" and "--full" in r.stderr


@pytest.mark.timeout(300)
def test_bench_dumps_what_the_last_timed_step_computed(tmp_path):
    """--dump-outputs DIR: the headline's embeddings and distance matrix of the last timed step, fp32, from the seeded crops of the
    run (here through the stand-in network, so the files can be recomputed on the host)."""
    from oracle import matching
    from reid_amd import synth
    from standin_lib import _embed_rows
    r = _bench(["--gpus", "1", "--workload", "embed", "--dump-outputs", str(tmp_path / "out"),
                "--crops", "8", "--steps", "3", "--warmup", "0", "--no-cpu", "--single"], 280)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _one_line(r)
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["distmat.npy", "embeddings.npy"]
    emb, dist = np.load(tmp_path / "out" / "embeddings.npy"), np.load(tmp_path / "out" / "distmat.npy")
    assert emb.dtype == np.float32 and dist.dtype == np.float32
    np.testing.assert_array_equal(emb, _embed_rows(list(synth.crops_u8(8, seed=1))))
    np.testing.assert_allclose(dist, matching.euclidean_dist(emb, emb), rtol=1e-6, atol=1e-6)


def test_dump_outputs_keeps_to_its_budget_with_a_fixed_row_sample(tmp_path, monkeypatch):
    """An output larger than its share of the budget is written as the same sorted, seeded sample of rows in every run; int32
    outputs become fp64, fp32 stays fp32."""
    import bench

    class Host:
        """What dump_outputs needs of a DevArray, over host memory (a device pointer is the row index)."""
        def __init__(self, a):
            self.a, self.shape, self.dtype, self.nbytes = a, a.shape, a.dtype, a.nbytes
            self.engine = self

        def numpy(self):
            return self.a.copy()

        def row_ptr(self, r):
            return int(r)

        def d2h(self, out, r):
            out[...] = self.a[r]

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40 * 1024)
    rng = np.random.default_rng(5)
    small = rng.normal(size=(4, 8)).astype(np.float32)
    big = rng.normal(size=(300, 64)).astype(np.float32)          # 76.8 kB: more than the 39 kB the other two leave
    idx = rng.integers(0, 1 << 30, size=(10, 20)).astype(np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": Host(big), "small": Host(small), "idx": Host(idx)})
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("big", "small", "idx")}
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in got) <= 40 * 1024 + 3 * 128
    np.testing.assert_array_equal(got["small"], small)
    assert got["idx"].dtype == np.float64 and (got["idx"] == idx).all()
    assert got["big"].dtype == np.float32 and 0 < len(got["big"]) < len(big)
    rows = [int(np.flatnonzero((big == row).all(1))[0]) for row in got["big"]]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    np.testing.assert_array_equal(got["big"], np.load(tmp_path / "b" / "big.npy"))
