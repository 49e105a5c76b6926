"""V-MPO's block middle kernel against the wide one (``vmpo_mid_kernel``),
device events.

    python scripts/vmpo_wide_bench.py [--repeats 5] [--iters 200]

(a) the middle launch alone at S=5, A=2: ``vmpo_mid`` against
    ``vmpo_mid_wide`` at BT = 640, 4096 and 7168, wide alone at BT = 8192,
    32768 and 65536 (past the block kernel's LDS), with the slab count the
    host heuristic picked;
(b) the whole V-MPO step (``updater.step``) at B = 2048 and 8192: the default
    keys, under which these shapes take the eager autograd step, against
    ``"vmpo_mid_kernel": "wide"`` + ``"wgrad_kernel": "split"``, one graph
    replay of the fused step.

Every shape is warmed up, the two sides alternate block by block inside one
process, a block is ``--iters`` calls between two device events, and each
block repeats ``--repeats`` times. One JSON line per measurement: median, min
and max of the blocks in µs per call.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

from scripts.wgrad_split_bench import DEV, alternate, report  # noqa: E402

S, A = 5, 2


def launch_section(e, args):
    opt = dict(device=DEV, dtype=torch.float32)
    for BT in (640, 4096, 7168, 8192, 32768, 65536):
        B = BT // (S - 1)
        N = B * S
        torch.manual_seed(BT)
        ins = [torch.randn(B, S, A + 1, **opt), torch.randn(N, A, **opt),
               -torch.rand(N, **opt), torch.randn(N, **opt) * 0.3 + 1.0,
               torch.randn(BT, **opt), torch.randn(BT, **opt),
               torch.zeros(1, **opt), torch.zeros(1, **opt)]
        outs = [torch.empty(BT, **opt), torch.zeros(8, **opt),
                torch.zeros(1, **opt), torch.zeros(1, **opt),
                torch.zeros(8, **opt), torch.zeros(1, **opt),
                torch.ones(1, device=DEV, dtype=torch.int32)]
        coefs = (A, 1.0, 0.5, 0.001, 0.01, 0.005, 0.01)
        floats, n_tickets = e.vmpo_mid_wide_workspace(BT, 0)
        ws = torch.empty(max(floats, 1), **opt)
        tickets = torch.zeros(n_tickets, device=DEV, dtype=torch.int32)
        fns = {"wide": lambda: e.vmpo_mid_wide(*ins, *outs, *coefs, ws,
                                               tickets, 0)}
        if 2 * BT * 4 <= 56 * 1024:
            fns["block"] = lambda: e.vmpo_mid(*ins, *outs, *coefs)
        for k, v in alternate(fns, args.iters, args.repeats).items():
            report("vmpo_mid_launch", v, kernel=k, BT=BT,
                   slabs=max(floats // 8, 1) if k == "wide" else 1)


def make_step(B: int, wide: bool):
    from bench import make_synthetic_batch
    from pdrl_amd.agents.learner_module import VMPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.batch_size, p.seq_len = "V-MPO", B, S
    p.obs_dim, p.n_actions = 4, A
    if wide:
        p.vmpo_mid_kernel, p.wgrad_kernel = "wide", "split"
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, A, p.seq_len, p.hidden_size)
    upd = VMPOUpdater(model, p, DEV)
    batch = make_synthetic_batch(p, DEV, seed=0)
    fused = upd.fused_step is not None and upd.fused_step.fits(batch)
    return (lambda: upd.step(batch)), fused


def step_section(args):
    for B in (2048, 8192):
        fns, path = {}, {}
        for name, wide in (("default", False), ("wide+split", True)):
            fns[name], fused = make_step(B, wide)
            path[name] = "fused" if fused else "eager"
        for k, v in alternate(fns, max(args.iters // 4, 20),
                              args.repeats).items():
            report("vmpo_step", v, keys=k, B=B, path=path[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded"
    assert args.repeats >= 5, "a range needs at least five blocks"
    launch_section(ops.ext(), args)
    step_section(args)


if __name__ == "__main__":
    main()
