"""Row rollout against the row-tile rollout (``rollout_kernel``), device events.

    python scripts/rollout_tile_bench.py [--repeats 7] [--iters 200]

One ``DeviceRollout.rollout()`` call (one launch) at H=64, S=5:

(a) CartPole-v1 (categorical) at N = 128, 1024, 4096, 16384;
(b) MountainCarContinuous-v0, Gaussian mode 1 (SAC-C), the same four N;
(c) Acrobot-v1 (categorical, the heaviest per-env chain) at N = 1024, 4096.

Every shape is warmed up, ``"row"`` and ``"tile"`` alternate block by block
inside one process, a block is ``--iters`` calls between two device events,
and each block repeats ``--repeats`` times. One JSON line per measurement:
median, min and max of the blocks in µs per call.
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
S = 5
SHAPES = (
    ("CartPole-v1", None, (128, 1024, 4096, 16384)),
    ("MountainCarContinuous-v0", 1, (128, 1024, 4096, 16384)),
    ("Acrobot-v1", None, (1024, 4096)),
)
OBS_ACT = {"CartPole-v1": (4, 2), "MountainCarContinuous-v0": (2, 1),
           "Acrobot-v1": (6, 3)}


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
        block_us(fn, max(iters // 4, 10))  # warm-up
    vals = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            vals[k].append(block_us(fn, iters))
    return vals


def report(values: list[float], **cfg):
    print(json.dumps({
        "metric": "rollout_call", "unit": "us/call",
        "median": round(sorted(values)[len(values) // 2], 2),
        "min": round(min(values), 2), "max": round(max(values), 2),
        "values": [round(v, 2) for v in values], **cfg,
    }), flush=True)


def make_rollouts(env: str, mode, n_envs: int) -> dict:
    """A row and a tile rollout on one core (same weights, same seed)."""
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.networks.models import MlpLSTMSeperateContinuous
    from pdrl_amd.ops.rollout import DeviceRollout

    torch.manual_seed(0)
    cls = MlpLSTMSingle if mode is None else MlpLSTMSeperateContinuous
    core = cls(*OBS_ACT[env], S, 64).to(DEV).actor.core
    return {k: DeviceRollout(core, env, n_envs, S, DEV, seed=1,
                             time_horizon=500, kernel=k).rollout
            for k in ("row", "tile")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded"
    assert args.repeats >= 5, "a range needs at least five blocks"
    for env, mode, sizes in SHAPES:
        for n_envs in sizes:
            fns = make_rollouts(env, mode, n_envs)
            iters = args.iters if n_envs <= 4096 else max(args.iters // 4, 20)
            for k, v in alternate(fns, iters, args.repeats).items():
                report(v, rollout_kernel=k, env=env, N=n_envs, S=S)


if __name__ == "__main__":
    main()
