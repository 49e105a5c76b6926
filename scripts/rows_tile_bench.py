"""Row kernels against row tiles (``rows_kernel``), device events.

    python scripts/rows_tile_bench.py [--repeats 5] [--iters 200]

Both settings run with ``"wgrad_kernel": "split"``, at H=64, F=4, D=3:

(a) the two recurrent launches alone at S=5, B = 128, 512, 1536, 4096:
    ``"row"`` is ``seq_lstm_fwd_loss`` + ``seq_lstm_bwd_fin`` (the pair the
    step launches past one row per CU; they carry the IMPALA loss phase),
    ``"tile"`` is ``seq_lstm_fwd_tile`` + ``seq_lstm_bwd_tile`` and, as a
    second row, the same with ``onpolicy_loss_rows`` + ``onpolicy_stats_fin``
    between them, which is the like-for-like amount of work;
(b) the whole IMPALA step (``updater.step``, one graph replay) at the same
    four B;
(c) the two tile launches alone at B=256, S=160, which no row kernel can
    launch.

Every shape is warmed up, the settings alternate block by block inside one
process, a block is ``--iters`` calls between two device events, and each
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
H, F_DIM, D_OUT = 64, 4, 3
BATCHES = (128, 512, 1536, 4096)


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


def recurrent_launches(e, B: int, S: int, with_row: bool) -> dict:
    """The recurrent launches of one IMPALA step on random inputs, as
    closures over preallocated buffers."""
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
    outs, gouts = torch.empty(B, S, D_OUT, **opt), torch.empty(B, S, D_OUT, **opt)
    hS, cS = torch.empty(B, H, **opt), torch.empty(B, H, **opt)
    stash = torch.empty(B, S, 7 * H, **opt)
    dgates, dxb = torch.empty(B, S, 4 * H, **opt), torch.empty(B, S, H, **opt)
    part, stats = torch.empty(B, 8, **opt), torch.zeros(8, **opt)
    norm = torch.zeros(1, **opt)
    act = torch.randint(0, 2, (B * S,), device=DEV).float()
    behav = -torch.rand(B, S, **opt)
    rew = torch.rand(B, S, **opt)
    fir = (torch.rand(B, S, **opt) < 0.1).float()
    coefs = (1.0, 0.5, 0.01, 0.0)  # cp, cv, ce, creg
    loss = (act, behav, rew, fir, gouts, part, norm, 0, 0.99, 0.95, 0.8, 0.1,
            1.0, 1.0, *coefs[:3], 0.2, coefs[3])

    def tile():
        e.seq_lstm_fwd_tile(x, h0, c0, *w, outs, hS, cS, stash)
        e.seq_lstm_bwd_tile(gouts, stash, c0, w[2], w[3], w[5], dgates, dxb)

    def tile_loss():
        e.seq_lstm_fwd_tile(x, h0, c0, *w, outs, hS, cS, stash)
        e.onpolicy_loss_rows(outs, *loss)
        e.onpolicy_stats_fin(part, stats, 0, B, S, D_OUT, *coefs)
        e.seq_lstm_bwd_tile(gouts, stash, c0, w[2], w[3], w[5], dgates, dxb)

    def row():
        e.seq_lstm_fwd_loss(x, h0, c0, *w, outs, hS, cS, stash, *loss)
        e.seq_lstm_bwd_fin(gouts, stash, x, c0, *bw, dgates, dxb, stats, part,
                           0, *coefs)

    tile_loss()  # gouts hold real head grads for the bare tile pair
    fns = {"tile": tile, "tile+loss": tile_loss}
    if with_row:
        fns = {"row": row, **fns}
    return fns


def launch_section(e, args):
    for B in BATCHES:
        fns = recurrent_launches(e, B, 5, with_row=True)
        for k, v in alternate(fns, args.iters, args.repeats).items():
            report("recurrent_launches", v, rows_kernel=k, B=B, S=5)
    fns = recurrent_launches(e, 256, 160, with_row=False)
    fns.pop("tile+loss")
    for k, v in alternate(fns, max(args.iters // 8, 10), args.repeats).items():
        report("recurrent_launches", v, rows_kernel=k, B=256, S=160)


def make_step(B: int, rows_kernel: str):
    from bench import make_synthetic_batch
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.batch_size, p.seq_len = "IMPALA", B, 5
    p.obs_dim, p.n_actions = 4, 2
    p.wgrad_kernel, p.rows_kernel = "split", rows_kernel
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    upd = ImpalaUpdater(model, p, DEV)
    batch = make_synthetic_batch(p, DEV, seed=0)
    assert upd.fused_step is not None and upd.fused_step.fits(batch)
    return lambda: upd.step(batch)


def step_section(args):
    for B in BATCHES:
        fns = {k: make_step(B, k) for k in ("row", "tile")}
        iters = args.iters if B <= 1536 else max(args.iters // 2, 20)
        for k, v in alternate(fns, iters, args.repeats).items():
            report("impala_step", v, rows_kernel=k, wgrad_kernel="split", B=B)


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
