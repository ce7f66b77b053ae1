"""`python bench.py --gpus N` without a launcher must start its own N ranks (one process per GPU) before any GPU
call and have rank 0 print exactly one JSON line (the driver's contract).  `--dry-run` swaps RCCL for gloo and the
GPU step for an empty one, so the launch / rendezvous / barrier / gather plumbing of every mode runs here on CPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--dry-run", *extra],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # ONE line, from rank 0 only
    return json.loads(lines[0])


@pytest.mark.parametrize("mode,scaling", [("iter", "weak"), ("problems", "strong"), ("rhs", "strong")])
def test_bench_spawns_its_own_ranks(mode, scaling):
    out = _run("--gpus", "2", "--mode", mode, "--nrhs", "7", "--problems", "5", *(("--full",) if mode == "iter" else ()))
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1 and out["dry_run"] is True
    assert out["scaling"] == scaling and out["value"] > 0 and out["higher_is_better"] is True
    if mode == "iter":
        # --full measures both sharded axes of SURVEY.md 8(e) behind the headline pass: the rows of a short `problems`
        # pass and a short `rhs` pass ride in the same JSON line (and exist at N = 1 as anchors)
        sm = out["scale_modes"]
        assert set(sm) == {"problems", "rhs"}, sm
        assert sm["problems"]["scaling"] == "strong" and sm["problems"]["config"]["problems_per_rank"] == 3
        assert sm["rhs"]["scaling"] == "strong" and sm["rhs"]["config"]["columns_per_rank"] == 4
        assert sm["problems"]["value"] > 0 and sm["rhs"]["value"] > 0
    if mode == "problems":
        assert out["config"]["problems_per_rank"] == 3       # rank 0 of 2 holds problems 0, 2, 4
    if mode == "rhs":
        assert out["config"]["columns_per_rank"] == 4        # columns 0, 2, 4, 6


def test_bench_single_rank_needs_no_launcher():
    out = _run("--full")
    assert out["n_gpus"] == 1 and out["dry_run"] is True
    assert set(out["scale_modes"]) == {"problems", "rhs"}        # the N = 1 anchors of the two sharded axes
    assert _run("--full", "--no-scale-modes")["scale_modes"] is None


def test_plain_run_reports_the_timed_steps_only():
    """A plain run times --steps steps after --warmup and reports them; the scale modes are --full's."""
    out = _run("--steps", "3", "--warmup", "2")
    assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] >= 0
    assert out["metric"] and out["unit"] == "KKT factorize+solve/s" and out["dtype"] == "f64" and out["higher_is_better"] is True
    assert "scale_modes" not in out and "cpu_baseline" not in out and "roofline" not in out


def test_bench_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "no CPU fallback" in (r.stdout + r.stderr)


@pytest.mark.gpu
def test_dump_outputs_repeat_from_run_to_run(tmp_path):
    """--dump-outputs writes what the last timed step returned; with the same arguments the inputs are the same, and
    so are the outputs (up to the summation order of the device's reductions)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    n = 4000
    dumps = []
    for i in range(2):
        d = tmp_path / str(i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--n", str(n),
                            "--dump-outputs", str(d)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1 and json.loads(lines[0])["steps"] == 3, r.stdout
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = dumps
    assert set(a) == {"step_x", "step_s", "step_z", "dtau_dkappa_affine_combined"}
    assert a["step_x"].shape == (n,) and a["step_s"].shape == a["step_z"].shape == (2 * n,)
    assert a["dtau_dkappa_affine_combined"].shape == (4,)
    for k in a:
        assert a[k].dtype == np.float64 and np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0, k
        assert np.abs(a[k] - b[k]).max() <= 1e-9 * np.abs(a[k]).max(), k
