"""Row kernels against the H = 128 row tiles (``rows_kernel``), device events.

    python scripts/rows_tile128_bench.py [--repeats 5] [--iters 200]

Hidden size 128, F=4, D=3, IMPALA, ``"wgrad_kernel": "split"`` throughout:

(a) the two recurrent launches alone at S=5, B = 128, 512, 1536, 4096:
    ``"row"`` is ``seq_lstm_forward`` + ``seq_lstm_backward_core`` (what the
    step launches at this width; they allocate their outputs), ``"tile128"``
    is ``seq_lstm_fwd_tile128`` + ``seq_lstm_bwd_tile128`` on preallocated
    buffers, as in the step's workspace;
(b) the whole IMPALA step (``updater.step``, one graph replay) at the same
    four B;
(c) past the row forward's S <= 32: the tile launches alone at B=256, S=64,
    and the whole step at B=4096, S=64.

Timing is that of ``rows_tile_bench.py``: every shape warmed up, the settings
alternating block by block inside one process, a block is ``--iters`` calls
between two device events, ``--repeats`` blocks each. One JSON line per
measurement: median, min and max of the blocks in µs per call.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "scripts"))

import torch  # noqa: E402
from rows_tile_bench import alternate, report  # noqa: E402

DEV = "cuda:0"
H, F_DIM, D_OUT = 128, 4, 3
BATCHES = (128, 512, 1536, 4096)


def recurrent_launches(e, B: int, S: int, with_row: bool) -> dict:
    """The recurrent launches of one step on random inputs, as closures."""
    from pdrl_amd.networks.models import SeqLSTMCore

    opt = dict(device=DEV, dtype=torch.float32)
    torch.manual_seed(B)
    core = SeqLSTMCore(F_DIM, H, {"logits": D_OUT - 1, "value": 1}).to(DEV)
    w = [p.detach() for p in (core.body_w, core.body_b, core.w_ih, core.w_hh,
                              core.b_g, core.heads_w, core.heads_b)]
    bw = [w[0], w[2], w[3], w[5]]
    x = torch.randn(B, S, F_DIM, **opt)
    hx = torch.randn(B, S, H, **opt) * 0.5
    cx = torch.randn(B, S, H, **opt) * 0.5
    h0, c0 = hx[:, 0], cx[:, 0]
    outs = torch.empty(B, S, D_OUT, **opt)
    gouts = torch.randn(B, S, D_OUT, **opt) * 0.1
    hS, cS = torch.empty(B, H, **opt), torch.empty(B, H, **opt)
    stash = torch.empty(B, S, 7 * H, **opt)
    dgates, dxb = torch.empty(B, S, 4 * H, **opt), torch.empty(B, S, H, **opt)

    def tile128():
        e.seq_lstm_fwd_tile128(x, h0, c0, *w, outs, hS, cS, stash, dgates)
        e.seq_lstm_bwd_tile128(gouts, stash, c0, w[2], w[3], w[5], dgates, dxb)

    def row():
        _, _, _, st = e.seq_lstm_forward(x, h0, c0, *w)
        e.seq_lstm_backward_core(gouts, None, None, st, x, c0, *bw)

    return {"row": row, "tile128": tile128} if with_row else {"tile128": tile128}


def make_step(B: int, S: int, rows_kernel: str):
    from bench import make_synthetic_batch
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.batch_size, p.seq_len, p.hidden_size = "IMPALA", B, S, H
    p.obs_dim, p.n_actions = 4, 2
    p.wgrad_kernel, p.rows_kernel = "split", rows_kernel
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    upd = ImpalaUpdater(model, p, DEV)
    batch = make_synthetic_batch(p, DEV, seed=0)
    assert upd.fused_step is not None and upd.fused_step.fits(batch)

    def step():
        return upd.step(batch)

    step.updater = upd
    return step


def check_replayed(step, **cfg):
    """The timed step ran as a captured graph and left finite statistics."""
    fs = step.updater.fused_step
    vals = [float(v) for v in step().values()]
    assert fs._graph is not None, "the step did not run under graph replay"
    assert all(abs(v) < 1e6 for v in vals), vals
    print(f"# graph replay ok, stats finite: {cfg}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded"
    assert args.repeats >= 5, "a range needs at least five blocks"
    e = ops.ext()
    for B in BATCHES:
        fns = recurrent_launches(e, B, 5, with_row=True)
        iters = args.iters if B <= 1536 else max(args.iters // 2, 20)
        for k, v in alternate(fns, iters, args.repeats).items():
            report("recurrent_launches", v, rows_kernel=k, B=B, S=5)
    fns = recurrent_launches(e, 256, 64, with_row=False)
    for k, v in alternate(fns, max(args.iters // 4, 10), args.repeats).items():
        report("recurrent_launches", v, rows_kernel=k, B=256, S=64)

    for B in BATCHES:
        fns = {k: make_step(B, 5, k) for k in ("row", "tile128")}
        iters = args.iters if B <= 1536 else max(args.iters // 4, 20)
        for k, v in alternate(fns, iters, args.repeats).items():
            report("impala_step", v, rows_kernel=k, wgrad_kernel="split", B=B,
                   S=5)
        if B == 4096:
            check_replayed(fns["tile128"], B=B, S=5)
    fns = {"tile128": make_step(4096, 64, "tile128")}
    for k, v in alternate(fns, 10, args.repeats).items():
        report("impala_step", v, rows_kernel=k, wgrad_kernel="split", B=4096,
               S=64)
    check_replayed(fns["tile128"], B=4096, S=64)


if __name__ == "__main__":
    main()
