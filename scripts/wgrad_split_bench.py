"""Sweep against split-K weight gradients (``wgrad_kernel``), device events.

    python scripts/wgrad_split_bench.py [--repeats 5] [--iters 200]

(a) the wgrad launch alone at H=64, S=5, F=4, D=3: ``seq_lstm_wgrad_out``
    against ``seq_lstm_wgrad_split_out`` at N = 640 … 7680, split alone at
    N = 10240 and 20480 (past the sweep's row table), with the slab plan the
    host heuristic picked;
(b) the whole IMPALA step (``updater.step``: one graph replay where the fused
    step covers the shape, the eager autograd step where it does not) at
    B = 128, 512, 1536 under both settings, and at B = 2048 and 4096, where
    ``"sweep"`` is the eager fallback and ``"split"`` the fused step.

Every shape is warmed up, the two kernels alternate block by block inside
one process, a block is ``--iters`` calls between two device events, and
each block repeats ``--repeats`` times. One JSON line per measurement:
median, min and max of the blocks in µs per call.

``--trace-step B --kernel K`` instead runs 300 steps of one configuration and
nothing else: the run to put under a kernel trace.
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
H, S, F_DIM, D_OUT = 64, 5, 4, 3


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


def report(name: str, values: list[float], **cfg):
    print(json.dumps({
        "metric": name, "unit": "us/call",
        "median": round(sorted(values)[len(values) // 2], 2),
        "min": round(min(values), 2), "max": round(max(values), 2),
        "values": [round(v, 2) for v in values], **cfg,
    }), flush=True)


def launch_section(e, args):
    opt = dict(device=DEV, dtype=torch.float32)
    for N in (640, 1280, 2560, 5120, 7680, 10240, 20480):
        B = N // S
        torch.manual_seed(N)
        t = dict(x=torch.randn(B, S, F_DIM, **opt),
                 h0=torch.randn(B, H, **opt) * 0.5,
                 stash=torch.randn(B, S, 7 * H, **opt) * 0.5,
                 dgates=torch.randn(B, S, 4 * H, **opt) * 0.1,
                 dxb=torch.randn(B, S, H, **opt) * 0.1,
                 gouts=torch.randn(B, S, D_OUT, **opt) * 0.1)
        ins = [t[k] for k in ("x", "h0", "stash", "dgates", "dxb", "gouts")]
        outs = [torch.empty(H, 4 * H, **opt), torch.empty(H, 4 * H, **opt),
                torch.empty(F_DIM, H, **opt), torch.empty(H, **opt),
                torch.empty(4 * H, **opt), torch.empty(H, D_OUT, **opt),
                torch.empty(D_OUT, **opt)]
        norm = torch.zeros(1, **opt)
        floats, n_tickets, rows, slabs = e.seq_lstm_wgrad_split_plan(
            N, H, F_DIM, D_OUT, 0)
        ws = torch.empty(max(floats, 1), **opt)
        tickets = torch.zeros(n_tickets, device=DEV, dtype=torch.int32)
        fns = {"split": lambda: e.seq_lstm_wgrad_split_out(
            *ins, *outs, norm, ws, tickets, 0)}
        if N <= 8192:
            fns["sweep"] = lambda: e.seq_lstm_wgrad_out(*ins, *outs, norm)
        for k, v in alternate(fns, args.iters, args.repeats).items():
            report("wgrad_launch", v, kernel=k, N=N, slab_rows=rows,
                   slabs=slabs if k == "split" else 1)


def make_step(B: int, kernel: str):
    from bench import make_synthetic_batch
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.batch_size, p.seq_len = "IMPALA", B, S
    p.obs_dim, p.n_actions, p.wgrad_kernel = 4, 2, kernel
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    upd = ImpalaUpdater(model, p, DEV)
    batch = make_synthetic_batch(p, DEV, seed=0)
    fused = upd.fused_step is not None and upd.fused_step.fits(batch)
    return (lambda: upd.step(batch)), fused


def step_section(args):
    for B in (128, 512, 1536, 2048, 4096):
        fns, path = {}, {}
        for kernel in ("sweep", "split"):
            fns[kernel], fused = make_step(B, kernel)
            path[kernel] = "fused" if fused else "eager"
        iters = args.iters if B <= 1536 else max(args.iters // 4, 20)
        for k, v in alternate(fns, iters, args.repeats).items():
            report("impala_step", v, wgrad_kernel=k, B=B, path=path[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--trace-step", type=int, default=0, metavar="B")
    ap.add_argument("--kernel", default="sweep", choices=("sweep", "split"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded"
    if args.trace_step:
        fn, _ = make_step(args.trace_step, args.kernel)
        for _ in range(300):
            fn()
        torch.cuda.synchronize()
        return
    assert args.repeats >= 5, "a range needs at least five blocks"
    launch_section(ops.ext(), args)
    step_section(args)


if __name__ == "__main__":
    main()
