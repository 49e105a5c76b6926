"""Row-tile recurrent kernels for hidden size 128
(csrc/seq_lstm_tile128.hip): the forward against a float64 core, forward +
BPTT through the weight gradients they feed against float64 autograd, and the
fused on-policy step under ``rows_kernel="tile128"`` against eager autograd.
All tests here require an MI355X."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 128
SENTINEL = -12345.0
PAD = 16  # spare rows behind B: a ragged tile must leave them alone
#        B   S   F  D
CASES = [(1, 1, 4, 3),    # one row of one tile, no recurrence
         (17, 5, 4, 3),   # second tile holds one row
         (40, 3, 6, 4),   # three ragged tiles, other input and head widths
         (16, 48, 4, 3)]  # past the row forward's S <= 32


def _ext():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops.ext()


@functools.lru_cache(maxsize=None)
def _case(B, S, F, D):
    """(core, its float64 copy, x, hx, cx); hx/cx are (B, S, H) and the
    kernels get their [:, 0] views, as in the step."""
    from pdrl_amd.networks.models import SeqLSTMCore

    torch.manual_seed(1000 * B + S)
    core = SeqLSTMCore(F, H, {"logits": D - 1, "value": 1}).to(DEV)
    x = torch.randn(B, S, F, device=DEV)
    hx = torch.randn(B, S, H, device=DEV) * 0.5
    cx = torch.randn(B, S, H, device=DEV) * 0.5
    return core, copy.deepcopy(core).double(), x, hx, cx


def _weights(core):
    return [p.detach() for p in (core.body_w, core.body_b, core.w_ih,
                                 core.w_hh, core.b_g, core.heads_w,
                                 core.heads_b)]


def _eager(core, x, hx, cx):
    heads, h, c = core._forward_eager(x, hx[:, 0], cx[:, 0])
    return torch.cat([heads[n] for n in core.head_names], dim=-1), h, c


def _forward(e, core, x, hx, cx):
    """The tile forward into NaN-filled outputs; outs, stash and the scratch
    tensor sit in front of PAD sentinel rows. Returns (outs, hS, cS, stash)."""
    B, S, _ = x.shape
    opt = dict(device=DEV, dtype=torch.float32)
    padded = [torch.full((B + PAD, S, W), SENTINEL, **opt)
              for W in (core.out_dim, 7 * H, 4 * H)]
    outs, stash, scratch = (t[:B].fill_(float("nan")) for t in padded)
    hS = torch.full((B, H), float("nan"), **opt)
    cS = torch.full((B, H), float("nan"), **opt)
    e.seq_lstm_fwd_tile128(x, hx[:, 0], cx[:, 0], *_weights(core), outs, hS,
                           cS, stash, scratch)
    for name, t in zip(("outs", "stash", "scratch"), padded):
        assert bool((t[B:] == SENTINEL).all()), f"{name} written past B"
    return outs, hS, cS, stash


@pytest.mark.parametrize("B,S,F,D", CASES)
def test_fwd_tile128_vs_float64(B, S, F, D):
    e = _ext()
    core, core64, x, hx, cx = _case(B, S, F, D)
    with torch.no_grad():
        ref = _eager(core64, x.double(), hx.double(), cx.double())
        atol = 1e-5
        if S == 48:  # another summation order over 128 terms, 48 steps deep
            f32 = _eager(core, x, hx, cx)
            err = max(float((a.double() - r).abs().max())
                      for a, r in zip(f32, ref))
            atol = max(atol, 4.0 * err)
    outs, hS, cS, _ = _forward(e, core, x, hx, cx)
    for name, got, want in zip(("outs", "hS", "cS"), (outs, hS, cS), ref):
        err = float((got.double() - want).abs().max())
        print(f"{name} ({B},{S},{F},{D}): max err {err:.3e}, atol {atol:.3e}")
        torch.testing.assert_close(got.double(), want, rtol=0.0, atol=atol,
                                   msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("B,S,F,D", [c for c in CASES if 1 < c[1] <= 32])
def test_fwd_bwd_tile128_weight_grads_vs_float64(B, S, F, D):
    e = _ext()
    core, core64, x, hx, cx = _case(B, S, F, D)
    opt = dict(device=DEV, dtype=torch.float32)
    gouts = torch.randn(B, S, D, **opt) * 0.1
    outs, _, _, stash = _forward(e, core, x, hx, cx)
    dgates = torch.full((B, S, 4 * H), float("nan"), **opt)
    dxb = torch.full((B, S, H), float("nan"), **opt)
    e.seq_lstm_bwd_tile128(gouts, stash, cx[:, 0], core.w_ih.detach(),
                           core.w_hh.detach(), core.heads_w.detach(), dgates,
                           dxb)
    grads = [torch.full_like(p, float("nan")) for p in (
        core.w_ih, core.w_hh, core.body_w, core.body_b, core.b_g,
        core.heads_w, core.heads_b)]
    e.seq_lstm_wgrad_out(x, hx[:, 0], stash, dgates, dxb, gouts, *grads, None)

    core64.zero_grad()
    ref_outs, _, _ = _eager(core64, x.double(), hx.double(), cx.double())
    (ref_outs * gouts.double()).sum().backward()
    want = (core64.w_ih, core64.w_hh, core64.body_w, core64.body_b,
            core64.b_g, core64.heads_w, core64.heads_b)
    names = ("dw_ih", "dw_hh", "dbody_w", "dbody_b", "db_g", "dheads_w",
             "dheads_b")
    for name, g_, p_ in zip(names, grads, want):
        err = float((g_.double() - p_.grad).abs().max())
        print(f"{name} ({B},{S},{F},{D}): max abs err {err:.3e}")
        torch.testing.assert_close(g_.double(), p_.grad, rtol=1e-4, atol=1e-5,
                                   msg=lambda m: f"{name}: {m}")


def _updater(algo, rows_kernel, wgrad_kernel, vmpo_mid_kernel):
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params

    continuous = algo.endswith("Continuous")
    p = load_params()
    p.algo, p.rows_kernel = algo, rows_kernel
    p.wgrad_kernel, p.vmpo_mid_kernel = wgrad_kernel, vmpo_mid_kernel
    p.batch_size, p.seq_len, p.hidden_size = 17, 5, H
    p.obs_dim, p.n_actions = (2, 1) if continuous else (4, 2)
    p.coef_alpha_below = p.coef_alpha_upper = 0.0075  # pin V-MPO's sampled dual
    upd_cls, model_cls = switch_module(algo)
    torch.manual_seed(3)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    upd = upd_cls(model, p, DEV)
    assert upd.fused_step is not None
    assert upd.fused_step.rows_kernel == rows_kernel
    return upd, model, p, continuous


@pytest.mark.parametrize("algo,wgrad_kernel,vmpo_mid_kernel", [
    ("IMPALA", "sweep", "block"),
    ("IMPALA", "split", "block"),
    ("PPO-Continuous", "sweep", "block"),
    ("V-MPO", "sweep", "block"),
    ("V-MPO", "sweep", "wide"),
])
def test_tile128_fused_grads_vs_autograd(algo, wgrad_kernel, vmpo_mid_kernel):
    _ext()
    from tests.conftest import make_batch

    stats = {}
    for rows_kernel in ("row", "tile128"):
        upd, model, p, continuous = _updater(algo, rows_kernel, wgrad_kernel,
                                             vmpo_mid_kernel)
        batch = make_batch(p, n_actions=p.n_actions, continuous=continuous,
                           device=DEV, seed=21)
        assert upd.fused_step.fits(batch)
        upd.fused_step.compute_grads_only(batch)
        stats[rows_kernel] = upd.fused_step.stats_buf.clone()
    torch.testing.assert_close(stats["tile128"], stats["row"], rtol=1e-5,
                               atol=0.0)

    fused = {n: q.grad.detach().clone() for n, q in model.named_parameters()}
    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in model.named_parameters():
        err = float((fused[n] - q.grad).abs().max())
        print(f"{algo} {n}: max abs err {err:.3e}")
        torch.testing.assert_close(fused[n], q.grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda m: f"{algo} {n}: {m}")
