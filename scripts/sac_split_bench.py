"""Sweep against split-K weight gradients in the two fused SAC steps
(``wgrad_kernel``), device events.

    python scripts/sac_split_bench.py [--repeats 5] [--iters 200]

``updater.step`` (one graph replay of the fused DAG) for SAC and
SAC-Continuous at S=5, H=64:

(a) B = 128, 512, 1536: ``"sweep"`` against ``"split"``;
(b) B = 2048, 4096 (past the sweep kernels' 8192 rows): ``"split"`` against
    the eager autograd step, which is what ``"sweep"`` falls back to there.

Every shape is warmed up, the settings alternate block by block inside one
process, a block is ``--iters`` calls between two device events (a tenth of
that for the eager step), and each block repeats ``--repeats`` times. One
JSON line per measurement: median, min and max of the blocks in µs per call.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

DEV = "cuda:0"
ALGOS = ("SAC", "SAC-Continuous")
BATCHES_BOTH = (128, 512, 1536)
BATCHES_SPLIT = (2048, 4096)


def block_us(fn, iters: int) -> float:
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def alternate(fns: dict, iters: dict, repeats: int) -> dict:
    for k, fn in fns.items():
        block_us(fn, max(iters[k] // 4, 5))  # warm-up
    vals = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            vals[k].append(block_us(fn, iters[k]))
    return vals


def report(name: str, values: list[float], **cfg):
    print(json.dumps({
        "metric": name, "unit": "us/call",
        "median": round(sorted(values)[len(values) // 2], 2),
        "min": round(min(values), 2), "max": round(max(values), 2),
        "values": [round(v, 2) for v in values], **cfg,
    }), flush=True)


def make_step(algo: str, B: int, setting: str):
    """``updater.step`` on one synthetic batch: the fused step with either
    kernel, or ("eager") the autograd step the sweep falls back to."""
    from bench import env_shape, make_synthetic_batch
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.batch_size, p.seq_len = algo, B, 5
    p.obs_dim, p.n_actions, _ = env_shape(algo)
    p.wgrad_kernel = "sweep" if setting == "eager" else setting
    upd_cls, model_cls = switch_module(algo)
    torch.manual_seed(0)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    upd = upd_cls(model, p, DEV)
    batch = make_synthetic_batch(p, DEV, seed=0)
    assert upd.fused_step is not None
    assert upd.fused_step.fits(batch) == (setting != "eager"), (B, setting)
    return lambda: upd.step(batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded"
    assert args.repeats >= 5, "a range needs at least five blocks"
    for algo in ALGOS:
        for B in BATCHES_BOTH + BATCHES_SPLIT:
            kinds = (("sweep", "split") if B in BATCHES_BOTH
                     else ("eager", "split"))
            fns = {k: make_step(algo, B, k) for k in kinds}
            iters = {k: max(args.iters // 10, 5) if k == "eager"
                     else args.iters for k in kinds}
            for k, v in alternate(fns, iters, args.repeats).items():
                report("sac_step", v, algo=algo, setting=k, B=B, S=5)


if __name__ == "__main__":
    main()
