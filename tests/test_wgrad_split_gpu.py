"""Split-K weight-gradient kernel (csrc/wgrad_split.hip): exact against a
float64 reference on integer inputs at the shapes where a split can go
wrong, its norm accumulation, its run-to-run bit reproducibility, and the
fused on-policy step built on it against eager autograd, past the sweep
kernel's 8192-row cap included. All tests here require an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F_DIM, D_OUT = 4, 3
NAMES = ("dw_ih", "dw_hh", "dbody_w", "dbody_b", "db_g", "dheads_w",
         "dheads_b")


def _ext():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops.ext()


def _inputs(B, S, H, seed, integer):
    """Kernel inputs: small integers in {-2..2} (every product and partial
    sum is an integer below 2^24, so fp32 sums are exact in any order), or
    random at training magnitudes (activations 0.5, gradients 0.1)."""
    g = torch.Generator(device="cpu").manual_seed(seed)

    def mk(*shape, scale):
        if integer:
            return torch.randint(-2, 3, shape, generator=g).float().to(DEV)
        return (torch.randn(*shape, generator=g) * scale).to(DEV)

    return dict(
        x=mk(B, S, F_DIM, scale=1.0), h0=mk(B, H, scale=0.5),
        stash=mk(B, S, 7 * H, scale=0.5), dgates=mk(B, S, 4 * H, scale=0.1),
        dxb=mk(B, S, H, scale=0.1), gouts=mk(B, S, D_OUT, scale=0.1))


def _reference(t, H):
    """float64 einsum over n = (b, s); hprev is h0 at t = 0 and the stash h
    field of the step before otherwise."""
    d = {k: v.double() for k, v in t.items()}
    xb, h = d["stash"][..., :H], d["stash"][..., 6 * H:]
    hprev = torch.cat([d["h0"][:, None, :], h[:, :-1, :]], dim=1)
    return [
        torch.einsum("bsm,bsg->mg", xb, d["dgates"]),
        torch.einsum("bsm,bsg->mg", hprev, d["dgates"]),
        torch.einsum("bsf,bsj->fj", d["x"], d["dxb"]),
        d["dxb"].sum((0, 1)),
        d["dgates"].sum((0, 1)),
        torch.einsum("bsk,bsd->kd", h, d["gouts"]),
        d["gouts"].sum((0, 1)),
    ]


def _buffers(e, N, H, slab_rows):
    """(outputs, workspace, tickets, norm) for one shape; the tickets are
    zeroed here once and never again."""
    opt = dict(device=DEV, dtype=torch.float32)
    outs = [torch.empty(H, 4 * H, **opt), torch.empty(H, 4 * H, **opt),
            torch.empty(F_DIM, H, **opt), torch.empty(H, **opt),
            torch.empty(4 * H, **opt), torch.empty(H, D_OUT, **opt),
            torch.empty(D_OUT, **opt)]
    floats, tickets = e.seq_lstm_wgrad_split_workspace(N, H, F_DIM, D_OUT,
                                                       slab_rows)
    return (outs, torch.empty(max(floats, 1), **opt),
            torch.zeros(tickets, device=DEV, dtype=torch.int32),
            torch.zeros(1, **opt))


def _run(e, t, outs, ws, tickets, norm, slab_rows):
    for o in outs:
        o.fill_(float("nan"))
    e.seq_lstm_wgrad_split_out(t["x"], t["h0"], t["stash"], t["dgates"],
                               t["dxb"], t["gouts"], *outs, norm, ws, tickets,
                               slab_rows)


@pytest.mark.parametrize("B,S,H,slab_rows", [
    (3, 5, 64, 0),       # one slab: direct write, no ticket
    (8, 4, 64, 8),       # every slab boundary at t = 0
    (8, 4, 64, 6),       # boundaries mid-sequence
    (11, 3, 64, 16),     # N = 33: last slab shorter than one MFMA step
    (12, 8, 64, 32),     # N an exact multiple of the slab
    (97, 1, 64, 4),      # more slabs than a chunk has rows; S = 1: all h0
    (11, 3, 32, 8),      # H = 32, ragged multi-slab
    (11, 3, 128, 8),     # H = 128, ragged multi-slab
    (1640, 5, 64, 0),    # N = 8200, past the sweep's cap, host heuristic
])
def test_split_direct_vs_float64_exact(B, S, H, slab_rows):
    e = _ext()
    t = _inputs(B, S, H, seed=1000 * B + S, integer=True)
    ref = _reference(t, H)
    outs, ws, tickets, norm = _buffers(e, B * S, H, slab_rows)
    for call in (1, 2):  # the second call proves the tickets reset themselves
        _run(e, t, outs, ws, tickets, norm, slab_rows)
        for name, g_, r_ in zip(NAMES, outs, ref):
            assert torch.equal(g_.double(), r_), (name, call, B * S)
    assert int(tickets.abs().sum()) == 0


def test_split_norm_sq():
    """One float atomicAdd per finishing workgroup, each of a float sum of
    squares: the accumulated ||grad||² equals the sum of squares of the
    outputs up to the any-order rounding of a sum of M positive terms,
    M · 2⁻²⁴ relative, M the number of gradient elements."""
    e = _ext()
    B, S, H, slab_rows = 11, 3, 64, 8
    t = _inputs(B, S, H, seed=88, integer=False)
    outs, ws, tickets, norm = _buffers(e, B * S, H, slab_rows)
    _run(e, t, outs, ws, tickets, norm, slab_rows)
    for name, g_, r_ in zip(NAMES, outs, _reference(t, H)):
        torch.testing.assert_close(g_.double(), r_, rtol=1e-4, atol=1e-5,
                                   msg=lambda m: f"{name}: {m}")
    want = sum(float((o.double() ** 2).sum()) for o in outs)
    bound = sum(o.numel() for o in outs) * 2.0 ** -24
    rel = abs(float(norm) - want) / want
    print(f"norm_sq rel err {rel:.3e} bound {bound:.3e}")
    assert rel <= bound, (float(norm), want, rel)


def test_split_bit_reproducible():
    e = _ext()
    B, S, H, slab_rows = 128, 5, 64, 32
    t = _inputs(B, S, H, seed=99, integer=False)
    outs, ws, tickets, norm = _buffers(e, B * S, H, slab_rows)
    _run(e, t, outs, ws, tickets, norm, slab_rows)
    first = [o.clone() for o in outs]
    _run(e, t, outs, ws, tickets, norm, slab_rows)
    for name, a_, b_ in zip(NAMES, first, outs):
        assert torch.equal(a_, b_), name


@pytest.mark.parametrize("algo,bsz,rtol,atol", [
    ("IMPALA", 16, 1e-4, 1e-6),
    ("PPO-Continuous", 16, 1e-4, 1e-6),
    # B·S = 10240 > 8192: the project's tolerance for its B = 1024 parity
    # case holds here (profiles/wgrad_split.md)
    ("IMPALA", 2048, 1e-3, 2e-5),
])
def test_split_fused_grads_vs_autograd(algo, bsz, rtol, atol):
    _ext()
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    continuous = algo.endswith("Continuous")
    p = load_params()
    p.algo, p.wgrad_kernel = algo, "split"
    p.batch_size, p.seq_len, p.hidden_size = bsz, 5, 64
    p.obs_dim, p.n_actions = (2, 1) if continuous else (4, 2)
    upd_cls, model_cls = switch_module(algo)
    torch.manual_seed(3)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    upd = upd_cls(model, p, DEV)
    assert upd.fused_step is not None
    assert upd.fused_step.wgrad_kernel == "split"
    batch = make_batch(p, n_actions=p.n_actions, continuous=continuous,
                       device=DEV, seed=21)
    assert upd.fused_step.fits(batch)

    upd.fused_step.compute_grads_only(batch)
    fused = {n: q.grad.detach().clone() for n, q in model.named_parameters()}
    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in model.named_parameters():
        torch.testing.assert_close(fused[n], q.grad, rtol=rtol, atol=atol,
                                   msg=lambda m: f"{algo} B={bsz} {n}: {m}")
