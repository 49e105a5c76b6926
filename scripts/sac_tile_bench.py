"""Row kernels against row tiles in the two fused SAC steps
(``rows_kernel``), device events.

    python scripts/sac_tile_bench.py [--repeats 5] [--iters 200]
                                     [--algos SAC SAC-Continuous]
                                     [--batches 128 512 1536 2048 4096]
                                     [--hidden 64]

``updater.step`` (one graph replay of the fused DAG) for SAC and
SAC-Continuous at S=5, H=64 and ``"wgrad_kernel": "split"``, so every batch
size stays on the HIP DAG: ``"row"`` (the 8- and 11-launch DAGs) against
``"tile"`` (the legacy launch sequence on row tiles). ``--hidden 128`` times
the H=128 kernels (csrc/seq_lstm_tile128_multi.hip); there ``"row"`` is the
legacy sequence too, the 8- and 11-launch DAGs being built for H=64.

Every shape is warmed up, the two settings alternate block by block inside
one process, a block is ``--iters`` calls between two device events, and each
block repeats ``--repeats`` times. One JSON line per measurement: median, min
and max of the blocks in µs per call.
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
BATCHES = (128, 512, 1536, 2048, 4096)
KERNELS = ("row", "tile")


def block_us(fn, iters: int) -> float:
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def alternate(fns: dict, iters: int, repeats: int) -> dict:
    for fn in fns.values():
        block_us(fn, max(iters // 4, 5))  # warm-up (captures the graph)
    vals = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            vals[k].append(block_us(fn, iters))
    return vals


def report(name: str, values: list[float], **cfg):
    print(json.dumps({
        "metric": name, "unit": "us/call",
        "median": round(sorted(values)[len(values) // 2], 2),
        "min": round(min(values), 2), "max": round(max(values), 2),
        "values": [round(v, 2) for v in values], **cfg,
    }), flush=True)


def make_step(algo: str, B: int, rows_kernel: str, hidden: int = 64):
    """``updater.step`` on one synthetic batch with either recurrent kernel."""
    from bench import env_shape, make_synthetic_batch
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.batch_size, p.seq_len = algo, B, 5
    p.obs_dim, p.n_actions, _ = env_shape(algo)
    p.wgrad_kernel, p.rows_kernel = "split", rows_kernel
    p.hidden_size = hidden
    upd_cls, model_cls = switch_module(algo)
    torch.manual_seed(0)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    upd = upd_cls(model, p, DEV)
    batch = make_synthetic_batch(p, DEV, seed=0)
    assert upd.fused_step is not None and upd.fused_step.fits(batch)
    assert upd.fused_step.rows_kernel == rows_kernel
    return lambda: upd.step(batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--algos", nargs="+", default=list(ALGOS), choices=ALGOS)
    ap.add_argument("--batches", nargs="+", type=int, default=list(BATCHES))
    ap.add_argument("--hidden", type=int, default=64, choices=(64, 128))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded"
    assert args.repeats >= 5, "a range needs at least five blocks"
    for algo in args.algos:
        for B in args.batches:
            fns = {k: make_step(algo, B, k, args.hidden) for k in KERNELS}
            for k, v in alternate(fns, args.iters, args.repeats).items():
                report("sac_step", v, algo=algo, rows_kernel=k,
                       wgrad_kernel="split", B=B, S=5, H=args.hidden)


if __name__ == "__main__":
    main()
