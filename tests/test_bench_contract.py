"""bench.py driver-contract tests (CPU): the JSON line schema and the
multi-rank launch behavior the round-end SCALE run depends on."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def _run_bench(*args, timeout=240, env=None):
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), *args],
        capture_output=True, text=True, cwd=REPO, timeout=timeout, env=env,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:]
    return json.loads(lines[-1])


def test_bench_single_rank_schema():
    rec = _run_bench("--steps", "3", "--warmup", "1")
    assert rec["metric"] == "learner_env_steps_per_sec"
    assert rec["n_gpus"] == 1
    assert rec["scaling"] == "weak"
    assert rec["higher_is_better"] is True
    assert rec["data"] == "synthetic"
    assert rec["config"]["parallelism"] == "dp1"
    assert rec["config"]["global_batch"] == 128
    # whole-job aggregate consistency: value == transitions / elapsed
    expect = rec["n_gpus"] * 128 * 5 / (rec["ms_per_step"] / 1000.0)
    assert abs(expect - rec["value"]) / rec["value"] < 1e-6


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's stats and updated weights
    as float32 .npy under the 64 MB cap; --full is accepted and keeps the
    result line; --steps is the number of timed steps reported."""
    import numpy as np

    out = tmp_path / "dump"
    rec = _run_bench("--steps", "2", "--warmup", "1", "--full",
                     "--dump-outputs", str(out))
    assert rec["metric"] == "learner_env_steps_per_sec"
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    files = sorted(out.glob("*.npy"))
    names = {f.stem for f in files}
    assert "stat_loss-total" in names
    assert any(n.startswith("param_model.") for n in names)
    total = 0
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32, f.name
        assert np.isfinite(a).all(), f.name
        total += a.nbytes
    assert 0 < total <= 64 * 1024 * 1024


def test_bench_inputs_and_dump_sample_are_reproducible(tmp_path):
    """Same arguments → identical inputs, and an over-budget array is cut to
    the same seeded sample each time."""
    import numpy as np

    sys.path.insert(0, str(REPO))
    import bench
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.batch_size, p.seq_len = "IMPALA", 8, 5
    a = bench.make_synthetic_batch(p, "cpu", seed=100)
    b = bench.make_synthetic_batch(p, "cpu", seed=100)
    assert a.keys() == b.keys()
    assert all((a[k] == b[k]).all() for k in a)

    big = np.arange(1000, dtype=np.float64)
    old = bench.DUMP_BUDGET_BYTES
    bench.DUMP_BUDGET_BYTES = 2 * 100 * 4  # two arrays, 100 floats each
    try:
        bench.dump_outputs(tmp_path / "a", {"big": big, "small": big[:10]})
        bench.dump_outputs(tmp_path / "b", {"big": big, "small": big[:10]})
    finally:
        bench.DUMP_BUDGET_BYTES = old
    x, y = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert x.dtype == np.float32 and x.shape == (100,)
    assert (x == y).all() and (np.diff(x) > 0).all()
    assert (np.load(tmp_path / "a" / "small.npy") == big[:10]).all()


def test_bench_multirank_self_exec_reports_true_world():
    """`python bench.py --gpus 2` (no torchrun) must SELF-EXEC into 2 real
    ranks — the round-1 hazard was one rank doing the work while the line
    claimed a 2x aggregate. n_gpus/global_batch must reflect the actual
    world size. This is a launch-contract test, not a device test: with
    fewer than two GPUs the two ranks run on the CPU over gloo (as in
    test_ddp.py), since rank 1 would otherwise have no device to claim."""
    import os

    import torch

    env = None
    if torch.cuda.device_count() < 2:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    rec = _run_bench("--gpus", "2", "--steps", "3", "--warmup", "1", env=env)
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "dp2"
    assert rec["config"]["global_batch"] == 256


def test_bench_staged_mode_cpu():
    """--mode staged (pinned fill + step + pipelined weight publish) runs
    on CPU and reports the same schema with mode labeled."""
    rec = _run_bench("--mode", "staged", "--steps", "3", "--warmup", "1")
    assert rec["config"]["mode"] == "staged"
    assert rec["metric"] == "learner_env_steps_per_sec"
    assert rec["value"] > 0
