"""V-MPO's multi-workgroup middle kernel (csrc/vmpo_mid_wide.hip): against a
float64 reference at the shapes where slabs, ties and the radix digits can go
wrong, its selected set against the block kernel's, its run-to-run bit
reproducibility, and the fused V-MPO step built on it against eager
autograd, past the block kernel's 7168-transition cap included. All tests
here require an MI355X."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COEF = dict(cp=1.0, cv=0.5, creg=0.001, eps_eta=0.01, eps_alpha=0.0075)
LOG_ETA, LOG_ALPHA = math.log(0.8), math.log(1.3)
BLOCK_MAX_BT = 7168


def _ext():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops.ext()


def _adv(kind, BT, g):
    if kind == "random":
        return torch.randn(BT, generator=g)
    if kind == "equal":
        return torch.full((BT,), 0.25)
    if kind == "three":
        return torch.tensor([-1.0, 0.5, 2.0])[torch.randint(0, 3, (BT,),
                                                            generator=g)]
    # "binades": a third above, a third below, mixed signs over 2^-5 .. 2^3,
    # and a third one ulp apart around 0.75, where the K-th largest falls:
    # the first digit separates the binades, the second 0.76 and 0.80 from
    # the cluster (same sign, exponent and two mantissa bits), the third the
    # cluster's own members
    n = BT // 3
    ulps = torch.arange(n, dtype=torch.int32) + torch.tensor(
        0.75).view(torch.int32)
    hi = torch.tensor([0.76, 0.80, 1.25, 3.5, 6.0, 0.9, 2.0])[:n]
    lo = torch.tensor([-8.0, -2.5, -0.3, -0.04, 0.04, 0.3, 0.7])[:BT - 2 * n]
    adv = torch.cat([hi, ulps.view(torch.float32), lo])
    return adv[torch.randperm(BT, generator=g)]


def _inputs(B, S, A, kind):
    g = torch.Generator().manual_seed(1000 * B + 10 * S + A)
    N, BT = B * S, B * (S - 1)
    t = dict(mo=torch.randn(B, S, A + 1, generator=g),
             behav=torch.randn(N, A, generator=g),
             logp=-torch.rand(N, generator=g) - 0.05,
             lse=torch.randn(N, generator=g) * 0.3 + 1.0,
             adv=_adv(kind, BT, g), td=torch.randn(BT, generator=g) * 2.0)
    return {k: v.float().to(DEV) for k, v in t.items()}


def _reference(t, B, S, A):
    """float64: first K of a stable descending sort, softmax, sums, duals."""
    d = {k: v.double() for k, v in t.items()}
    BT, K = B * (S - 1), max(1, B * (S - 1) // 2)
    i = torch.arange(BT, device=DEV)
    si = (i // (S - 1)) * S + i % (S - 1)
    eta, alpha = math.exp(LOG_ETA), math.exp(LOG_ALPHA)
    sel = torch.zeros(BT, dtype=torch.bool, device=DEV)
    sel[torch.sort(d["adv"], descending=True, stable=True).indices[:K]] = True
    m = d["adv"][sel].max()
    e = torch.exp((d["adv"] - m) / eta) * sel
    Z = e.sum()
    mo = d["mo"].reshape(-1, A + 1)[si]
    lpb = torch.log_softmax(d["behav"][si], -1)
    kl = (lpb.exp() * (lpb - (mo[:, :A] - d["lse"][si, None]))).sum(-1).mean()
    dv = mo[:, A] - d["td"]
    vl = torch.where(dv.abs() < 1, 0.5 * dv * dv, dv.abs() - 0.5).mean()
    pl = -(e / Z * d["logp"][si]).sum()
    lse_sel = m / eta + Z.log() - math.log(K)
    c = COEF
    total = (c["cp"] * pl + c["cv"] * vl + eta * c["eps_eta"] + eta * lse_sel
             + alpha * c["eps_alpha"] + c["creg"] * (mo[:, :A] ** 2).mean())
    g_eta = (c["eps_eta"] + lse_sel - (e * d["adv"]).sum() / Z / eta) * eta
    g_alpha = alpha * (c["eps_alpha"] - kl)
    scal = torch.stack([total, pl, vl, torch.tensor(eta, device=DEV),
                        torch.tensor(alpha, device=DEV), kl, g_eta, g_alpha,
                        g_eta ** 2 + g_alpha ** 2])
    return sel, e / Z, scal


def _call(e, fn, t, A, seed, extra=()):
    """One launch of a middle kernel on fresh outputs; returns (psi, the nine
    scalars of _reference, scalars_g[7], rng_state after)."""
    opt = dict(device=DEV, dtype=torch.float32)
    out = dict(psi=torch.full_like(t["adv"], float("nan")),
               scal=torch.zeros(8, **opt), g_eta=torch.zeros(1, **opt),
               g_alpha=torch.zeros(1, **opt), stats=torch.zeros(8, **opt),
               norm=torch.zeros(1, **opt),
               rng=torch.tensor([seed], dtype=torch.int32, device=DEV))
    c = COEF
    fn(t["mo"], t["behav"], t["logp"], t["lse"], t["adv"], t["td"],
       torch.tensor([LOG_ETA], **opt), torch.tensor([LOG_ALPHA], **opt),
       out["psi"], out["scal"], out["g_eta"], out["g_alpha"], out["stats"],
       out["norm"], out["rng"], A, c["cp"], c["cv"], c["creg"], c["eps_eta"],
       c["eps_alpha"], c["eps_alpha"], *extra)
    nine = torch.cat([out["stats"][:6], out["g_eta"], out["g_alpha"],
                      out["norm"]])
    return out["psi"], nine, out["scal"][7], int(out["rng"])


def _wide_buffers(e, BT, slab):
    floats, tickets = e.vmpo_mid_wide_workspace(BT, slab)
    return (torch.empty(max(floats, 1), device=DEV),
            torch.zeros(tickets, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("B,S,A,slab,kind", [
    (1, 2, 2, 0, "random"),      # BT = 1
    (1, 4, 2, 2, "random"),      # BT = 3, K = 1, last slab has one element
    (5, 5, 2, 0, "random"),      # one slab, no ticket
    (5, 5, 3, 6, "random"),      # slabs cut mid-row, odd leftovers, A = 3
    (16, 5, 2, 16, "random"),    # BT an exact multiple of the slab
    (16, 5, 2, 16, "equal"),     # all ties; ranks cross slab boundaries
    (16, 5, 2, 24, "three"),     # threshold straddles slabs, n_eq > need_eq
    (7, 4, 2, 5, "binades"),     # every radix digit decides
    (1800, 5, 2, 0, "random"),   # BT = 7200, past the block cap, heuristic
])
def test_wide_vs_float64(B, S, A, slab, kind):
    e = _ext()
    BT, K = B * (S - 1), max(1, B * (S - 1) // 2)
    t = _inputs(B, S, A, kind)
    sel, psi_ref, scal_ref = _reference(t, B, S, A)
    ws, tickets = _wide_buffers(e, BT, slab)
    seed = 12345
    lcg = (seed * 1664525 + 1013904223) % 2 ** 32
    for call in (1, 2):  # the second call proves the ticket reset itself
        psi, nine, alpha, rng = _call(e, e.vmpo_mid_wide, t, A, seed,
                                      (ws, tickets, slab))
        assert torch.equal(psi > 0, sel), (call, "selected set")
        assert float(psi[~sel].abs().sum()) == 0.0 and int(sel.sum()) == K
        torch.testing.assert_close(psi.double()[sel], psi_ref[sel],
                                   rtol=1e-3, atol=1e-6 / K)
        print(call, nine.tolist(), scal_ref.tolist())
        torch.testing.assert_close(nine.double(), scal_ref, rtol=1e-3,
                                   atol=1e-5)
        torch.testing.assert_close(float(alpha), math.exp(LOG_ALPHA),
                                   rtol=1e-3, atol=1e-5)
        assert rng % 2 ** 32 == lcg
    assert int(tickets.abs().sum()) == 0
    if BT <= BLOCK_MAX_BT:
        psi_b = _call(e, e.vmpo_mid, t, A, seed)[0]
        assert torch.equal(psi_b > 0, sel), "block kernel's selected set"


def test_wide_bit_reproducible():
    e = _ext()
    B, S, A, slab = 128, 5, 2, 64
    t = _inputs(B, S, A, "random")
    ws, tickets = _wide_buffers(e, B * (S - 1), slab)
    runs = [_call(e, e.vmpo_mid_wide, t, A, 7, (ws, tickets, slab))
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1][:8], runs[1][1][:8])  # stats, g_eta, g_alpha


@pytest.mark.parametrize("bsz,fwdloss,rtol,atol", [
    (16, "1", 2e-4, 2e-6), (16, "0", 2e-4, 2e-6),
    (2048, "1", 1e-3, 2e-5),  # BT = 8192: eager on the parent commit
])
def test_wide_fused_grads_vs_autograd(bsz, fwdloss, rtol, atol):
    _ext()
    from pdrl_amd.agents.learner_module import VMPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = bsz, 5, 4, 2
    p.hidden_size, p.vmpo_mid_kernel, p.wgrad_kernel = 64, "wide", "split"
    p.coef_alpha_below = p.coef_alpha_upper = 0.0075  # pin the sampled dual
    os.environ["PDRL_FWDLOSS"] = fwdloss
    try:
        torch.manual_seed(5)
        model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
        upd = VMPOUpdater(model, p, DEV)
        assert upd.fused_step is not None
        assert upd.fused_step.vmpo_mid_kernel == "wide"
        batch = make_batch(p, seed=31, device=DEV)
        assert upd.fused_step.fits(batch)

        upd.fused_step.compute_grads_only(batch)
        named = list(model.named_parameters()) + [
            ("log_eta", upd.log_eta), ("log_alpha", upd.log_alpha)]
        fused = {n: q.grad.detach().clone() for n, q in named}
        upd.optimizer.zero_grad()
        loss, _ = upd.compute_losses(batch)
        loss.backward()
        for n, q in named:
            dual = n.startswith("log_")
            torch.testing.assert_close(
                fused[n], q.grad, rtol=1e-3 if dual else rtol,
                atol=1e-5 if dual else atol, msg=lambda m: f"{n}: {m}")
        for _ in range(2):  # the graph path: capture, then a replay
            stats = upd.step(batch)
        assert all(math.isfinite(float(v)) for v in stats.values()), stats
    finally:
        os.environ.pop("PDRL_FWDLOSS", None)
