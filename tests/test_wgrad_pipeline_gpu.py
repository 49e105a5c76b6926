"""Pipelined weight-gradient sweep: the K-sweep ring, the unrolled small-grad
sweep and the flat grid of csrc/wgrad_body.h against float64 references, at
the sizes where a software pipeline can go wrong (shorter than a chunk,
shorter than the ring, exactly full, ragged tail), and the fused on-policy
step (seq_lstm_bwd_fin + wgrad) against autograd at shapes the existing
parity tests do not run. All tests here require an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F_DIM, D_OUT = 4, 3
CHUNK, RING = 32, 3  # rows per chunk (4·kWgU) and ring depth kWgP
NAMES = ("dw_ih", "dw_hh", "dbody_w", "dbody_b", "db_g", "dheads_w",
         "dheads_b", "dbody2_w", "dbody2_b")


def _ext():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops.ext()


def _inputs(B, S, H, dual, seed):
    """Random kernel inputs at the magnitudes the kernel sees in training:
    activations of order 0.5, gradients of order 0.1. The kernel only reads
    them, so no forward pass is needed."""
    g = torch.Generator(device="cpu").manual_seed(seed)

    def rnd(*shape, scale):
        return (torch.randn(*shape, generator=g) * scale).to(DEV)

    t = dict(
        x=rnd(B, S, F_DIM, scale=1.0), h0=rnd(B, H, scale=0.5),
        stash=rnd(B, S, 7 * H, scale=0.5), dgates=rnd(B, S, 4 * H, scale=0.1),
        dxb=rnd(B, S, H, scale=0.1), gouts=rnd(B, S, D_OUT, scale=0.1),
    )
    if dual:
        t["x2"] = rnd(B, S, 2, scale=1.0)
    return t


def _reference(t, H):
    """float64 einsum over n = (b, s); hprev is h0 at t = 0 and the stash h
    field of the step before otherwise."""
    d = {k: v.double() for k, v in t.items()}
    xb, h = d["stash"][..., :H], d["stash"][..., 6 * H:]
    hprev = torch.cat([d["h0"][:, None, :], h[:, :-1, :]], dim=1)
    dual = "x2" in d
    half = H // 2 if dual else H
    ref = [
        torch.einsum("bsm,bsg->mg", xb, d["dgates"]),
        torch.einsum("bsm,bsg->mg", hprev, d["dgates"]),
        torch.einsum("bsf,bsj->fj", d["x"], d["dxb"][..., :half]),
        d["dxb"][..., :half].sum((0, 1)),
        d["dgates"].sum((0, 1)),
        torch.einsum("bsk,bsd->kd", h, d["gouts"]),
        d["gouts"].sum((0, 1)),
    ]
    if dual:
        ref += [torch.einsum("bsf,bsj->fj", d["x2"], d["dxb"][..., half:]),
                d["dxb"][..., half:].sum((0, 1))]
    return ref


# (B, S) → N = B·S against the 32-row chunk and the 3-chunk ring; from
# N = 160 (5 chunks) the steady-state loop runs, below that only the drain
SHAPES_H64 = [
    (1, 2),     # N=2    tail only
    (3, 5),     # N=15   ragged, less than one chunk
    (8, 4),     # N=32   exactly one chunk
    (11, 3),    # N=33   one chunk plus a tail
    (19, 5),    # N=95   ring one row short of full
    (12, 8),    # N=96   ring exactly full (32·P)
    (97, 1),    # N=97   ring full plus one row
    (32, 5),    # N=160  first size that enters the steady-state loop
    (128, 5),   # N=640  the flagship
]
CASES = ([(b, s, 64, False) for b, s in SHAPES_H64] +
         [(3, 5, 32, False), (11, 3, 32, False),
          (3, 5, 128, False), (11, 3, 128, False),
          (11, 3, 64, True)])


def test_ring_shapes_match_the_kernel_constants():
    """The shape table above is built for a 32-row chunk and a 3-deep ring;
    if the kernel's constants move, the table has to move with them."""
    import re
    from pathlib import Path

    import pdrl_amd.ops as ops_pkg

    src = (Path(ops_pkg.__file__).parent / "csrc" / "wgrad_body.h").read_text()
    u = int(re.search(r"constexpr int kWgU = (\d+);", src).group(1))
    p = int(re.search(r"constexpr int kWgP = (\d+);", src).group(1))
    assert (4 * u, p) == (CHUNK, RING)
    ns = {b * s for b, s in SHAPES_H64}
    assert {CHUNK * RING - 1, CHUNK * RING, CHUNK * RING + 1,
            CHUNK * (2 * RING - 1)} <= ns


@pytest.mark.parametrize("B,S,H,dual", CASES)
def test_wgrad_direct_vs_float64(B, S, H, dual):
    e = _ext()
    t = _inputs(B, S, H, dual, seed=1000 * B + S)
    got = e.seq_lstm_wgrad(t["x"], t["h0"], t["stash"], t["dgates"], t["dxb"],
                           t["gouts"], x2=t.get("x2"))
    ref = _reference(t, H)
    assert len(got) == len(ref) == (9 if dual else 7)
    for name, g_, r_ in zip(NAMES, got, ref):
        torch.testing.assert_close(g_.double(), r_, rtol=1e-4, atol=1e-5,
                                   msg=lambda m: f"{name} N={B * S}: {m}")


@pytest.mark.parametrize("B,S", [(11, 3), (128, 5)])
def test_wgrad_out_norm_sq(B, S):
    """One float atomicAdd per block: the accumulated ||grad||² equals the
    sum of squares of the seven outputs up to the rounding of a positive
    float sum in any order, n_blocks · 2⁻²⁴ relative."""
    e = _ext()
    H = 64
    t = _inputs(B, S, H, False, seed=77 + B)
    opt = dict(device=DEV, dtype=torch.float32)
    outs = [torch.empty(H, 4 * H, **opt), torch.empty(H, 4 * H, **opt),
            torch.empty(F_DIM, H, **opt), torch.empty(H, **opt),
            torch.empty(4 * H, **opt), torch.empty(H, D_OUT, **opt),
            torch.empty(D_OUT, **opt)]
    norm = torch.zeros(1, **opt)
    e.seq_lstm_wgrad_out(t["x"], t["h0"], t["stash"], t["dgates"], t["dxb"],
                         t["gouts"], *outs, norm)
    for name, g_, r_ in zip(NAMES, outs, _reference(t, H)):
        torch.testing.assert_close(g_.double(), r_, rtol=1e-4, atol=1e-5,
                                   msg=lambda m: f"{name}: {m}")
    want = sum(float((o.double() ** 2).sum()) for o in outs)
    gemm_blocks = 2 * (H // 16) * (4 * H // 64)
    small_waves = F_DIM * H + H + 4 * H + H * D_OUT + D_OUT
    n_blocks = gemm_blocks + (small_waves * 64 + 255) // 256
    rel = abs(float(norm) - want) / want
    print(f"norm_sq rel err {rel:.3e} bound {n_blocks * 2.0 ** -24:.3e}")
    assert rel <= n_blocks * 2.0 ** -24, (float(norm), want, rel)


def _params(algo, bsz, seq):
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo = algo
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = bsz, seq, 4, 2
    return p


@pytest.mark.parametrize("bsz,seq", [(1, 2), (7, 8), (16, 5)])
def test_fused_grads_impala_vs_autograd(bsz, seq):
    """seq_lstm_bwd_fin feeding the pipelined wgrad inside the fused step:
    gradients match eager autograd through the same forward, from a single
    row of two steps (wgrad tail only) to N = 80."""
    _ext()
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from tests.conftest import make_batch

    p = _params("IMPALA", bsz, seq)
    torch.manual_seed(3)
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    upd = ImpalaUpdater(model, p, DEV)
    assert upd.fused_step is not None
    batch = make_batch(p, seed=21, device=DEV)
    assert upd.fused_step.fits(batch)

    upd.fused_step.compute_grads_only(batch)
    fused = {n: q.grad.detach().clone() for n, q in model.named_parameters()}

    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in model.named_parameters():
        torch.testing.assert_close(fused[n], q.grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda m: f"{n}: {m}")


def test_fused_grads_vmpo_vs_autograd():
    """The V-MPO branch of seq_lstm_bwd_fin writes gouts in-kernel, runs the
    same row backward and feeds the same wgrad launch."""
    _ext()
    from pdrl_amd.agents.learner_module import VMPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from tests.conftest import make_batch

    p = _params("V-MPO", 16, 5)
    p.coef_alpha_below = p.coef_alpha_upper = 0.0075  # pin the sampled dual
    torch.manual_seed(5)
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    upd = VMPOUpdater(model, p, DEV)
    assert upd.fused_step is not None
    batch = make_batch(p, seed=31, device=DEV)
    assert upd.fused_step.fits(batch)

    upd.fused_step.compute_grads_only(batch)
    fused = {n: q.grad.detach().clone() for n, q in model.named_parameters()}

    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in model.named_parameters():
        torch.testing.assert_close(fused[n], q.grad, rtol=2e-4, atol=2e-6,
                                   msg=lambda m: f"{n}: {m}")
