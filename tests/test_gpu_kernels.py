"""GPU kernel parity tests: every HIP kernel vs the PyTorch fp32 eager
oracle (SURVEY.md §4's test mandate). All tests here require an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, S, F_DIM, H, A = 16, 5, 4, 64, 2


def _ops():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops


def make_core(heads, seed=0):
    from pdrl_amd.networks import SeqLSTMCore

    torch.manual_seed(seed)
    return SeqLSTMCore(F_DIM, H, heads).to(DEV)


def test_extension_loads_on_gpu():
    _ops()


def test_seq_lstm_forward_parity():
    _ops()
    core = make_core({"logits": A, "value": 1})
    torch.manual_seed(1)
    x = torch.randn(B, S, F_DIM, device=DEV)
    hx = torch.randn(B, H, device=DEV) * 0.3
    cx = torch.randn(B, H, device=DEV) * 0.3

    outs_f, h_f, c_f = core._forward_fused(x, hx, cx)
    outs_e, h_e, c_e = core._forward_eager(x, hx, cx)

    torch.testing.assert_close(h_f, h_e, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(c_f, c_e, rtol=1e-5, atol=1e-5)
    for k in outs_e:
        torch.testing.assert_close(outs_f[k], outs_e[k], rtol=1e-5, atol=1e-5)


def test_async_weight_publisher_gpu():
    """AsyncWeightPublisher (the learner's pipelined broadcast): payloads
    decode back to the exact actor weights; close() joins cleanly."""
    _ops()
    import time

    from pdrl_amd.agents.learner import AsyncWeightPublisher
    from pdrl_amd.buffers.wire import unpack_weights
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import Protocol, decode

    torch.manual_seed(2)
    model = MlpLSTMSingle(4, 2, 5, 64).to(DEV)
    got = []
    pub = AsyncWeightPublisher(model.actor, DEV,
                               lambda h, p: got.append((h, p)))
    for _ in range(5):
        with torch.no_grad():
            for q in model.actor.parameters():
                q.add_(0.01)
        pub.publish()  # may coalesce (double-buffered) — that's the design
    # quiesce, then publish the FINAL weights once and wait for it
    deadline = time.monotonic() + 10
    while pub._free.qsize() < 2 and time.monotonic() < deadline:
        time.sleep(0.02)
    n_before = len(got)
    pub.publish()
    while len(got) <= n_before and time.monotonic() < deadline:
        time.sleep(0.02)
    pub.close()
    assert len(got) > n_before, "final broadcast did not arrive"
    proto, obj = decode(*got[-1])
    assert proto is Protocol.Model
    state = unpack_weights(obj)
    sd = model.actor.state_dict()
    for k, v in state.items():
        torch.testing.assert_close(v.to(DEV), sd[k], rtol=0, atol=0)


def test_split_graph_multirank_path():
    """The multi-rank split-graph machinery (capture [fwd..wgrad] and
    [optimizer] separately, collective stream-ordered between) must produce
    the single-rank trajectory when the reducer is a no-op — exercised on
    one GPU so the driver's first real 8-GPU run isn't its first run."""
    _ops()
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.parallel import GradReducer
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.algo = "IMPALA"
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 32, 5, 4, 2
    upd_cls, model_cls = switch_module("IMPALA")

    torch.manual_seed(13)
    model_a = model_cls(4, 2, p.seq_len, p.hidden_size)
    torch.manual_seed(13)
    model_b = model_cls(4, 2, p.seq_len, p.hidden_size)

    reducer = GradReducer()  # dist not initialized → enabled=False (no-op)
    assert not reducer.enabled
    upd_a = upd_cls(model_a, p, DEV, grad_reducer=reducer)
    upd_b = upd_cls(model_b, p, DEV)

    batch = make_batch(p, seed=41, device=DEV)
    for _ in range(3):
        sa = upd_a.step(batch)
        sb = upd_b.step(batch)
    assert getattr(upd_a.fused_step, "_split_graphs", None) is not None, \
        "split-graph capture must engage on the multi-rank path"
    torch.testing.assert_close(upd_a.optimizer.flat_param,
                               upd_b.optimizer.flat_param,
                               rtol=1e-4, atol=1e-6)
    for k in sa:
        assert abs(float(sa[k]) - float(sb[k])) < 1e-3, (k,)


def test_dual_body_core_parity():
    """Dual-body SeqLSTMCore (continuous-critic topology: obs/action
    encoders straight into the LSTM): fused forward AND full autograd
    backward — dx, dx2, both encoder weight grads — vs the eager oracle."""
    _ops()
    from pdrl_amd.networks import SeqLSTMCore

    torch.manual_seed(5)
    core_f = SeqLSTMCore(3, H, {"q": 1}, input2_dim=2).to(DEV)
    torch.manual_seed(5)
    core_e = SeqLSTMCore(3, H, {"q": 1}, input2_dim=2).to(DEV)

    torch.manual_seed(9)
    x = torch.randn(B, S, 3, device=DEV)
    x2 = torch.randn(B, S, 2, device=DEV)
    hx = torch.randn(B, H, device=DEV) * 0.2
    cx = torch.randn(B, H, device=DEV) * 0.2
    w = torch.randn(B, S, 1, device=DEV)

    xf = x.clone().requires_grad_()
    x2f = x2.clone().requires_grad_()
    xe = x.clone().requires_grad_()
    x2e = x2.clone().requires_grad_()

    outs_f, hf, cf = core_f._forward_fused(xf, hx, cx, x2f)
    outs_e, he, ce = core_e._forward_eager(xe, hx, cx, x2e)
    torch.testing.assert_close(outs_f["q"], outs_e["q"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(hf, he, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(cf, ce, rtol=1e-5, atol=1e-5)

    ((outs_f["q"] * w).sum() + 0.1 * hf.sum()).backward()
    ((outs_e["q"] * w).sum() + 0.1 * he.sum()).backward()
    torch.testing.assert_close(xf.grad, xe.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(x2f.grad, x2e.grad, rtol=1e-4, atol=1e-5)
    for (n, pf), pe in zip(core_f.named_parameters(), core_e.parameters()):
        torch.testing.assert_close(pf.grad, pe.grad, rtol=2e-4, atol=1e-5,
                                   msg=lambda m: f"{n}: {m}")


def test_seq_lstm_backward_parity():
    _ops()
    for seed in (0, 7):
        core_f = make_core({"logits": A, "value": 1}, seed=seed)
        core_e = make_core({"logits": A, "value": 1}, seed=seed)
        torch.manual_seed(seed + 100)
        x = torch.randn(B, S, F_DIM, device=DEV)
        hx = torch.randn(B, H, device=DEV, requires_grad=True) * 0.3
        cx = torch.randn(B, H, device=DEV) * 0.3
        xf = x.clone().requires_grad_(True)
        xe = x.clone().requires_grad_(True)
        hf = hx.detach().clone().requires_grad_(True)
        he = hx.detach().clone().requires_grad_(True)

        outs_f, hSf, _ = core_f._forward_fused(xf, hf, cx)
        outs_e, hSe, _ = core_e._forward_eager(xe, he, cx)
        # mixed loss touching both heads + the final state
        loss_f = (outs_f["logits"].square().mean() + outs_f["value"].abs().mean()
                  + hSf.mean())
        loss_e = (outs_e["logits"].square().mean() + outs_e["value"].abs().mean()
                  + hSe.mean())
        loss_f.backward()
        loss_e.backward()

        torch.testing.assert_close(xf.grad, xe.grad, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(hf.grad, he.grad, rtol=1e-4, atol=1e-5)
        for (n1, p1), (n2, p2) in zip(core_f.named_parameters(),
                                      core_e.named_parameters()):
            assert n1 == n2
            torch.testing.assert_close(p1.grad, p2.grad, rtol=1e-4, atol=1e-5,
                                       msg=lambda m: f"{n1}: {m}")


def test_gae_parity():
    _ops()
    from pdrl_amd.agents.learner_module.compute_loss import compute_gae

    torch.manual_seed(2)
    deltas = torch.randn(B, S - 1, 1, device=DEV)
    dones = (torch.rand(B, S - 1, 1, device=DEV) < 0.3).float()
    got = compute_gae(deltas, 0.99, 0.95, dones)  # dispatches to HIP on GPU
    want = compute_gae(deltas.cpu(), 0.99, 0.95, dones.cpu())
    torch.testing.assert_close(got.cpu(), want, rtol=1e-5, atol=1e-6)


def test_vtrace_parity():
    _ops()
    from pdrl_amd.agents.learner_module.compute_loss import compute_v_trace

    torch.manual_seed(3)
    behav = -torch.rand(B, S, 1, device=DEV)
    target = behav + 0.3 * torch.randn(B, S, 1, device=DEV)
    is_fir = (torch.rand(B, S, 1, device=DEV) < 0.2).float()
    rew = torch.randn(B, S, 1, device=DEV)
    val = torch.randn(B, S, 1, device=DEV)
    rhos_g, adv_g, vs_g = compute_v_trace(behav, target, is_fir, rew, val, 0.99)
    rhos_c, adv_c, vs_c = compute_v_trace(
        behav.cpu(), target.cpu(), is_fir.cpu(), rew.cpu(), val.cpu(), 0.99
    )
    torch.testing.assert_close(rhos_g.cpu(), rhos_c, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(vs_g.cpu(), vs_c, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(adv_g.cpu(), adv_c, rtol=1e-4, atol=1e-5)


def test_soft_update_parity():
    _ops()
    from pdrl_amd.agents.learner_module.compute_loss import soft_update
    from pdrl_amd.networks import MlpLSTMCritic

    torch.manual_seed(4)
    net = MlpLSTMCritic(F_DIM, A, S, H).to(DEV)
    tgt_g = MlpLSTMCritic(F_DIM, A, S, H).to(DEV)
    tgt_c = MlpLSTMCritic(F_DIM, A, S, H)
    tgt_c.load_state_dict({k: v.cpu() for k, v in tgt_g.state_dict().items()})
    net_c = MlpLSTMCritic(F_DIM, A, S, H)
    net_c.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})

    soft_update(net, tgt_g, 0.005)  # HIP multi-tensor path
    soft_update(net_c, tgt_c, 0.005)  # eager path
    for pg, pc in zip(tgt_g.parameters(), tgt_c.parameters()):
        torch.testing.assert_close(pg.cpu(), pc, rtol=1e-6, atol=1e-7)


def _clone_params(n=3, seed=5):
    torch.manual_seed(seed)
    shapes = [(64, 256), (37,), (4, 64)]
    base = [torch.randn(*s) * 0.1 for s in shapes]
    grads = [torch.randn(*s) for s in shapes]
    return base, grads


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_fused_optimizer_parity(kind):
    _ops()
    from pdrl_amd.ops.optim import FusedAdam, FusedRMSprop

    base, grads = _clone_params()
    max_norm = 1.5

    # fused (GPU)
    ps_f = [torch.nn.Parameter(b.clone().to(DEV)) for b in base]
    opt_f = (FusedRMSprop(ps_f, lr=1e-2, eps=1e-5, max_norm=max_norm)
             if kind == "rmsprop" else
             FusedAdam(ps_f, lr=1e-2, max_norm=max_norm))

    # reference (torch, CPU)
    ps_r = [torch.nn.Parameter(b.clone()) for b in base]
    opt_r = (torch.optim.RMSprop(ps_r, lr=1e-2, eps=1e-5)
             if kind == "rmsprop" else torch.optim.Adam(ps_r, lr=1e-2))

    for step in range(5):
        gs = [g * (0.5 + step) for g in grads]
        opt_f.zero_grad()
        for p, g in zip(ps_f, gs):
            p.grad.copy_(g.to(DEV))
        opt_f.step()

        for p, g in zip(ps_r, gs):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ps_r, max_norm)
        opt_r.step()

    for pf, pr in zip(ps_f, ps_r):
        torch.testing.assert_close(pf.detach().cpu(), pr.detach(),
                                   rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("algo,continuous", [
    ("PPO", False), ("IMPALA", False), ("V-MPO", False),
    ("SAC", False), ("SAC-Continuous", True), ("PPO-Continuous", True),
])
def test_updater_step_on_gpu(algo, continuous):
    _ops()
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    torch.manual_seed(0)
    p = load_params()
    p.algo = algo
    p.batch_size, p.seq_len = 16, 5
    p.obs_dim = 2 if continuous else 4
    p.n_actions = 1 if continuous else 2
    upd_cls, model_cls = switch_module(algo)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    upd = upd_cls(model, p, DEV)
    batch = make_batch(p, n_actions=p.n_actions, continuous=continuous, device=DEV)
    batch["obs"] = torch.randn(p.batch_size, p.seq_len, p.obs_dim, device=DEV)
    for _ in range(3):
        stats = upd.step(batch)
    assert all(np.isfinite(float(v)) for v in stats.values()), stats


def test_gpu_vs_cpu_updater_trajectories_match():
    """Full IMPALA update on GPU (fused kernels) vs CPU (eager) from identical
    init: parameters must agree to fp32 tolerance after 3 steps."""
    _ops()
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 16, 5, 4, 2
    p.lr = 1e-4  # trajectory tolerance is calibrated for this lr

    torch.manual_seed(42)
    model_g = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    torch.manual_seed(42)
    model_c = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)

    upd_g = ImpalaUpdater(model_g, p, DEV)
    upd_c = ImpalaUpdater(model_c, p, "cpu")
    batch_c = make_batch(p, seed=9)
    batch_g = {k: v.to(DEV) for k, v in batch_c.items()}
    for _ in range(3):
        sg = upd_g.step(batch_g)
        sc = upd_c.step(batch_c)
    # RMSprop normalizes near-zero grads to full lr-scale steps, so ~1e-6
    # fp differences (fast-math exp, GEMM reduction order) show as ~1e-3
    # param deltas; tight parity is asserted on GRADIENTS in
    # test_fused_grad_parity_vs_autograd below.
    for (n, pg), pc in zip(model_g.named_parameters(), model_c.parameters()):
        torch.testing.assert_close(pg.detach().cpu(), pc.detach(), rtol=0.1,
                                   atol=4e-3, msg=lambda m: f"{n}: {m}")
    assert abs(float(sg["loss-total"]) - float(sc["loss-total"])) < 1e-2


def test_fused_step_engaged_and_ppo_parity():
    """PPO on GPU runs the fused whole-step DAG; parameters track the CPU
    eager oracle across 3 updates."""
    _ops()
    from pdrl_amd.agents.learner_module import PPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 16, 5, 4, 2
    p.lr = 1e-4  # trajectory tolerance is calibrated for this lr

    torch.manual_seed(7)
    model_g = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    torch.manual_seed(7)
    model_c = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)

    upd_g = PPOUpdater(model_g, p, DEV)
    assert upd_g.fused_step is not None, "fused step must engage on GPU"
    upd_c = PPOUpdater(model_c, p, "cpu")
    batch_c = make_batch(p, seed=11)
    batch_g = {k: v.to(DEV) for k, v in batch_c.items()}
    for _ in range(3):
        sg = upd_g.step(batch_g)
        sc = upd_c.step(batch_c)
    for (n, pg), pc in zip(model_g.named_parameters(), model_c.parameters()):
        torch.testing.assert_close(pg.detach().cpu(), pc.detach(), rtol=0.1,
                                   atol=4e-3, msg=lambda m: f"{n}: {m}")
    for k in ("loss-total", "loss-policy", "loss-value", "entropy",
              "ratio-avg", "ratio-min", "ratio-max"):
        assert abs(float(sg[k]) - float(sc[k])) < 5e-2, (k, float(sg[k]), float(sc[k]))


@pytest.mark.parametrize("algo", ["IMPALA", "PPO"])
def test_fused_grad_parity_vs_autograd(algo):
    """The fused whole-step DAG's gradients (loss bwd + BPTT + MFMA wgrad)
    must match GPU eager autograd through the same fused forward."""
    _ops()
    from pdrl_amd.agents.learner_module import ImpalaUpdater, PPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.algo = algo
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 16, 5, 4, 2
    torch.manual_seed(3)
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    cls = ImpalaUpdater if algo == "IMPALA" else PPOUpdater
    upd = cls(model, p, DEV)
    assert upd.fused_step is not None
    batch = make_batch(p, seed=21, device=DEV)

    # fused analytic grads into the flat buffer
    upd.fused_step.compute_grads_only(batch)
    fused = {n: q.grad.detach().clone() for n, q in model.named_parameters()}

    # eager autograd through the same fused forward kernels
    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in model.named_parameters():
        torch.testing.assert_close(fused[n], q.grad, rtol=1e-4, atol=1e-6,
                                   msg=lambda m: f"{n}: {m}")


@pytest.mark.parametrize("bsz,fwdloss", [
    (16, "1"), (16, "0"),   # fused rows vs separate launches
    (1024, "1"),            # BT=4096: vmpo_mid's multi-pass strided loops
])
def test_vmpo_fused_grad_parity_vs_autograd(bsz, fwdloss):
    """Fused V-MPO loss (top-half selection + duals + analytic bwd) vs GPU
    eager autograd, with the sampled dual coefficient pinned. Covers both
    launch sequences: row-local pre/grad phases fused into the fwd/bwd
    launches (PDRL_FWDLOSS=1) and the separate launches (PDRL_FWDLOSS=0)."""
    _ops()
    import os

    from pdrl_amd.agents.learner_module import VMPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = bsz, 5, 4, 2
    p.coef_alpha_below = p.coef_alpha_upper = 0.0075  # pin the sampled dual
    # at BT=4096 the psi softmax sums 2048 exp terms: fp32 accumulation
    # order alone moves head grads ~5e-4 rel (selection + loss identical)
    rtol, atol = (1e-3, 2e-5) if bsz >= 512 else (2e-4, 2e-6)
    os.environ["PDRL_FWDLOSS"] = fwdloss
    try:
        torch.manual_seed(5)
        model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
        upd = VMPOUpdater(model, p, DEV)
        assert upd.fused_step is not None
        batch = make_batch(p, seed=31, device=DEV)
        assert upd.fused_step.fits(batch)

        upd.fused_step.compute_grads_only(batch)
        fused = {n: q.grad.detach().clone()
                 for n, q in model.named_parameters()}
        fused_eta = upd.log_eta.grad.detach().clone()
        fused_alpha = upd.log_alpha.grad.detach().clone()

        upd.optimizer.zero_grad()
        loss, stats_e = upd.compute_losses(batch)
        loss.backward()
        for n, q in model.named_parameters():
            torch.testing.assert_close(fused[n], q.grad, rtol=rtol,
                                       atol=atol,
                                       msg=lambda m: f"{n}: {m}")
        torch.testing.assert_close(fused_eta.squeeze(),
                                   upd.log_eta.grad.squeeze(),
                                   rtol=1e-3, atol=1e-5)
        torch.testing.assert_close(fused_alpha.squeeze(),
                                   upd.log_alpha.grad.squeeze(),
                                   rtol=1e-3, atol=1e-5)
        # loss value parity
        upd.fused_step._body(batch, update=False)
        torch.testing.assert_close(upd.fused_step.stats_buf[0],
                                   loss.detach(), rtol=1e-3, atol=1e-4)
    finally:
        os.environ.pop("PDRL_FWDLOSS", None)


def test_ppo_continuous_fused_grad_parity():
    """Fused Gaussian-policy PPO loss (K5) vs GPU eager autograd."""
    _ops()
    from pdrl_amd.agents.learner_module import PPOUpdater
    from pdrl_amd.networks import MlpLSTMSingleContinuous
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.algo = "PPO-Continuous"
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 16, 5, 2, 1
    torch.manual_seed(9)
    model = MlpLSTMSingleContinuous(2, 1, p.seq_len, p.hidden_size)
    upd = PPOUpdater(model, p, DEV)
    assert upd.fused_step is not None and upd.fused_step.algo == "PPO-C"
    batch = make_batch(p, n_actions=1, continuous=True, device=DEV, seed=41)
    batch["obs"] = torch.randn(p.batch_size, p.seq_len, 2, device=DEV)
    assert upd.fused_step.fits(batch)

    upd.fused_step.compute_grads_only(batch)
    fused = {n: q.grad.detach().clone() for n, q in model.named_parameters()}

    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in model.named_parameters():
        torch.testing.assert_close(fused[n], q.grad, rtol=2e-4, atol=2e-6,
                                   msg=lambda m: f"{n}: {m}")
    upd.fused_step._body(batch, update=False)
    torch.testing.assert_close(upd.fused_step.stats_buf[0], loss.detach(),
                               rtol=1e-3, atol=1e-4)


def test_batch_stager_roundtrip_gpu():
    """Packed pinned-buffer staging delivers exact field contents with
    STABLE device tensors across calls (zero-copy graph replay contract)."""
    _ops()
    from pdrl_amd.agents import BatchStager

    st = BatchStager(DEV)
    rng = np.random.default_rng(0)
    b1 = {k: rng.standard_normal((4, 5, d)).astype(np.float32)
          for k, d in [("obs", 4), ("rew", 1), ("hx", 64)]}
    out1 = st.stage(b1)
    for k in b1:
        torch.testing.assert_close(out1[k].cpu(), torch.from_numpy(b1[k]))
    b2 = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in b1.items()}
    out2 = st.stage(b2)
    for k in b2:
        assert out2[k].data_ptr() == out1[k].data_ptr()  # stable views
        torch.testing.assert_close(out2[k].cpu(), torch.from_numpy(b2[k]))


@pytest.mark.parametrize("B,S,A", [(1, 5, 2), (16, 2, 2), (7, 8, 5), (16, 5, 16)])
def test_fused_impala_shape_sweep(B, S, A):
    """Fused-step gradient parity across odd shapes (tail paths: B*S % 32,
    single-row batches, minimum seq, wide action spaces)."""
    _ops()
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = B, S, 4, A
    torch.manual_seed(B * 100 + S * 10 + A)
    model = MlpLSTMSingle(4, A, S, p.hidden_size)
    upd = ImpalaUpdater(model, p, DEV)
    assert upd.fused_step is not None
    batch = make_batch(p, n_actions=A, device=DEV, seed=B + S + A)

    upd.fused_step.compute_grads_only(batch)
    fused = {n: q.grad.detach().clone() for n, q in model.named_parameters()}
    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in model.named_parameters():
        torch.testing.assert_close(fused[n], q.grad, rtol=2e-4, atol=2e-6,
                                   msg=lambda m: f"shape {(B,S,A)} {n}: {m}")


def test_fused_impala_large_shape_fallback():
    """Large shapes, BOTH launch sequences vs eager autograd: the loss
    fused into the forward launch and — with PDRL_FWDLOSS=0 — the
    separate forward / loss / backward launches. The row-local loss has
    no shape cap on either."""
    _ops()
    import os

    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 640, 5, 4, 2
    for fwdloss in ("1", "0"):
        os.environ["PDRL_FWDLOSS"] = fwdloss
        try:
            torch.manual_seed(2)
            model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
            upd = ImpalaUpdater(model, p, DEV)
            batch = make_batch(p, device=DEV, seed=77)
            upd.fused_step.compute_grads_only(batch)
            fused = {n: q.grad.detach().clone()
                     for n, q in model.named_parameters()}
            upd.optimizer.zero_grad()
            loss, _ = upd.compute_losses(batch)
            loss.backward()
            for n, q in model.named_parameters():
                torch.testing.assert_close(
                    fused[n], q.grad, rtol=2e-4, atol=2e-6,
                    msg=lambda m: f"fwdloss={fwdloss} {n}: {m}")
        finally:
            os.environ.pop("PDRL_FWDLOSS", None)


def _onpolicy_updater(algo, hidden, bsz, seq, n_act=2, seed=3):
    """(updater, batch) of an on-policy algorithm on the GPU, with V-MPO's
    sampled dual coefficient pinned."""
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    continuous = algo.endswith("Continuous")
    p = load_params()
    p.algo = algo
    p.batch_size, p.seq_len, p.hidden_size = bsz, seq, hidden
    p.obs_dim = 2 if continuous else 4
    p.n_actions = 1 if continuous else n_act
    p.coef_alpha_below = p.coef_alpha_upper = 0.0075
    upd_cls, model_cls = switch_module(algo)
    torch.manual_seed(seed)
    model = model_cls(p.obs_dim, p.n_actions, seq, hidden)
    upd = upd_cls(model, p, DEV)
    batch = make_batch(p, n_actions=p.n_actions, continuous=continuous,
                       device=DEV, seed=seed + 40)
    return upd, batch


def _assert_fused_grads_match_autograd(upd, batch, rtol, atol, tag):
    """compute_grads_only vs compute_losses().backward() on the same GPU."""
    fs = upd.fused_step
    assert fs is not None and fs.fits(batch)
    named = list(upd.model.named_parameters())
    duals = list(upd.extra_params().items())  # V-MPO: log_eta, log_alpha

    fs.compute_grads_only(batch)
    fused = {n: q.grad.detach().clone() for n, q in named + duals}
    upd.optimizer.zero_grad()
    loss, _ = upd.compute_losses(batch)
    loss.backward()
    for n, q in named:
        torch.testing.assert_close(fused[n], q.grad, rtol=rtol, atol=atol,
                                   msg=lambda m: f"{tag} {n}: {m}")
    for n, q in duals:
        torch.testing.assert_close(fused[n].squeeze(), q.grad.squeeze(),
                                   rtol=1e-3, atol=1e-5,
                                   msg=lambda m: f"{tag} {n}: {m}")


@pytest.mark.parametrize("algo,hidden,bsz,seq,n_act", [
    (algo, hidden, 3, 3, 2)
    for algo in ("IMPALA", "PPO", "PPO-Continuous", "V-MPO")
    for hidden in (32, 128)
] + [
    (algo, 32, bsz, seq, n_act)
    for algo in ("IMPALA", "PPO")
    # (1, 2): T=1, a one-step scan with BT=1; (7, 8, 5): odd sizes
    for bsz, seq, n_act in ((1, 2, 2), (7, 8, 5))
])
def test_general_path_grad_parity_vs_autograd(algo, hidden, bsz, seq, n_act):
    """H≠64 runs the row-local losses as separate launches (forward,
    loss rows, stats reduce / V-MPO mid + grad rows, backward): gradients
    must match GPU eager autograd for every algorithm."""
    _ops()
    upd, batch = _onpolicy_updater(algo, hidden, bsz, seq, n_act)
    assert not upd.fused_step.fused_rows
    _assert_fused_grads_match_autograd(
        upd, batch, rtol=2e-4, atol=2e-6,
        tag=f"{algo} H={hidden} {(bsz, seq, n_act)}")


@pytest.mark.parametrize("fwdloss", ["1", "0"])
@pytest.mark.parametrize("algo", ["IMPALA", "PPO", "PPO-Continuous", "V-MPO"])
def test_fused_stats_match_eager(algo, fwdloss):
    """Every stat the fused step reports (the per-row partials + one-block
    reduce, or vmpo_mid's) vs the eager loss, on both launch sequences."""
    _ops()
    import os

    os.environ["PDRL_FWDLOSS"] = fwdloss
    try:
        upd, batch = _onpolicy_updater(algo, 64, 16, 5)
    finally:
        os.environ.pop("PDRL_FWDLOSS", None)
    fs = upd.fused_step
    assert fs is not None and fs.fits(batch)
    assert fs.fused_rows == (fwdloss == "1")

    fs._body(batch, update=False)
    got = {n: fs.stats_buf[i].clone() for i, n in enumerate(fs.stat_names)}
    _, want = upd.compute_losses(batch)
    shared = [n for n in fs.stat_names if n in want]
    must = {"V-MPO": {"eta", "alpha", "kl"},
            "IMPALA": {"rho-avg"}}.get(algo, {"ratio-min", "ratio-max"})
    assert must | {"loss-total", "loss-policy", "loss-value"} <= set(shared)
    for n in shared:
        torch.testing.assert_close(
            got[n], want[n].detach().float().reshape(()), rtol=1e-3,
            atol=1e-4, msg=lambda m: f"{algo} fwdloss={fwdloss} {n}: {m}")


@pytest.mark.parametrize("algo", ["PPO-Continuous", "V-MPO"])
def test_fused_path_width_beyond_old_loss_cap(algo):
    """B=1024, S=5 at H=32: beyond the (2BS+2BT)*4 / (2BS+3BT)*4 <= 56 KiB
    LDS caps the single-block loss kernels had; the row-local losses only
    keep vmpo_mid's 2*BT*4 cap and the wgrad row table (B*S <= 8192)."""
    _ops()
    upd, batch = _onpolicy_updater(algo, 32, 1024, 5)
    _assert_fused_grads_match_autograd(upd, batch, rtol=1e-3, atol=2e-5,
                                       tag=f"{algo} B=1024")


def test_impala_gates_on_fits_beyond_wgrad_table():
    """B*S > 8192 exceeds the wgrad kernels' row-pointer table: IMPALA must
    see fits() == False (and so take the eager step), like the others."""
    _ops()
    upd, batch = _onpolicy_updater("IMPALA", 64, 2048, 5)
    assert upd.fused_step is not None
    assert not upd.fused_step.fits(batch)

    def no_launch(_batch):
        raise AssertionError("fused step launched on a shape fits() rejects")

    upd.fused_step.run = no_launch
    stats = upd.step(batch)  # the eager step
    assert all(np.isfinite(float(v)) for v in stats.values()), stats
    upd_ok, batch_ok = _onpolicy_updater("IMPALA", 64, 1638, 5)  # 8190 rows
    assert upd_ok.fused_step.fits(batch_ok)


@pytest.mark.parametrize("fast8", ["1", "0"])
def test_sac_fused_step_parity(fast8):
    """Fused SAC-discrete DAG vs the eager updater: identical parameter
    trajectories from identical init over 3 updates (gradients are analytic,
    no sampling in the discrete SAC step). Covers the 8-launch restructured
    DAG (PDRL_SAC8=1) and the legacy 10-launch sequence."""
    _ops()
    import os

    from pdrl_amd.agents.learner_module import SACUpdater
    from pdrl_amd.networks import MlpLSTMSeperate
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    os.environ["PDRL_SAC8"] = fast8
    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 16, 5, 4, 2
    p.lr = 1e-4

    torch.manual_seed(11)
    model_f = MlpLSTMSeperate(4, 2, p.seq_len, p.hidden_size)
    torch.manual_seed(11)
    model_e = MlpLSTMSeperate(4, 2, p.seq_len, p.hidden_size)

    upd_f = SACUpdater(model_f, p, DEV)
    assert upd_f.fused_step is not None, "fused SAC step must engage"
    upd_e = SACUpdater(model_e, p, DEV)
    upd_e.fused_step = None  # force the eager path on the same GPU

    batch = make_batch(p, seed=55, device=DEV)
    for _ in range(3):
        sf = upd_f.step(batch)
        se = upd_e.step(batch)
    for (n, pf), pe in zip(model_f.named_parameters(), model_e.parameters()):
        torch.testing.assert_close(pf.detach(), pe.detach(), rtol=5e-3,
                                   atol=5e-4, msg=lambda m: f"{n}: {m}")
    torch.testing.assert_close(upd_f.log_alpha.detach(), upd_e.log_alpha.detach(),
                               rtol=1e-3, atol=1e-5)
    for k in ("loss-actor", "loss-value", "loss-alpha", "alpha", "entropy"):
        assert abs(float(sf[k]) - float(se[k])) < 5e-2, (k, float(sf[k]), float(se[k]))
    # target critics moved in both
    try:
        for tf, te in zip(upd_f.target_critic.parameters(),
                          upd_e.target_critic.parameters()):
            torch.testing.assert_close(tf.detach(), te.detach(), rtol=5e-3,
                                       atol=5e-4)
    finally:
        os.environ.pop("PDRL_SAC8", None)


# --------------------------------------------------------------------------- #
# SAC-Continuous fused kernels (csrc/sacc_loss.hip; math derivation verified
# on CPU in tests/test_sacc_analytic.py)
# --------------------------------------------------------------------------- #
LOG_STD_MIN, LOG_STD_MAX, EPS_A = -20.0, 2.0, 1e-7


def _sacc_logpi(mu, ls_raw, eps):
    import math

    ls = ls_raw.clamp(LOG_STD_MIN, LOG_STD_MAX)
    a = torch.tanh(mu + ls.exp() * eps)
    lp = (-0.5 * eps.pow(2) - ls - 0.5 * math.log(2 * math.pi)
          - torch.log(1.0 - a.pow(2) + EPS_A)).sum(-1, keepdim=True)
    return a, lp


@pytest.mark.gpu
def test_sacc_sample_kernel_consistency():
    _ops()
    from pdrl_amd.ops import ext

    e = ext()
    B, S, A = 64, 8, 2
    torch.manual_seed(4)
    moA = torch.randn(B, S, 2 * A, device=DEV)
    moA[..., A:] *= 3.0  # exercise the clamp band
    rng = torch.randint(1, 1 << 30, (1,), dtype=torch.int32, device=DEV)
    eps = torch.empty(B, S, A, device=DEV)
    act = torch.empty(B, S, A, device=DEV)
    logpi = torch.empty(B, S, 1, device=DEV)
    e.sacc_sample(moA, rng, eps, act, logpi)
    mu, ls = moA[..., :A], moA[..., A:]
    a_ref, lp_ref = _sacc_logpi(mu, ls, eps)
    torch.testing.assert_close(act, a_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(logpi, lp_ref, rtol=1e-4, atol=1e-4)
    # eps is standard-normal-ish and fresh per call (device-resident seed)
    assert abs(float(eps.mean())) < 0.15
    assert 0.8 < float(eps.std()) < 1.2
    eps2 = torch.empty_like(eps)
    e.sacc_sample(moA, rng, eps2, act, logpi)
    assert not torch.allclose(eps, eps2)


@pytest.mark.gpu
def test_sacc_actor_grad_kernel_vs_autograd():
    _ops()
    from pdrl_amd.ops import ext

    e = ext()
    B, S, A = 16, 5, 2
    N = B * S
    torch.manual_seed(5)
    moA = torch.randn(B, S, 2 * A, device=DEV)
    moA[0, 0, A:] = 3.0  # clamped high → masked dlog_std
    rng = torch.randint(1, 1 << 30, (1,), dtype=torch.int32, device=DEV)
    eps = torch.empty(B, S, A, device=DEV)
    act = torch.empty(B, S, A, device=DEV)
    logpi = torch.empty(B, S, 1, device=DEV)
    e.sacc_sample(moA, rng, eps, act, logpi)
    g = torch.randn(B, S, A, device=DEV)  # stand-in dminQ/da
    q1 = torch.randn(N, device=DEV)
    q2 = torch.randn(N, device=DEV)
    log_alpha = torch.tensor([-0.4], device=DEV)
    target_entropy = -float(A)

    dmoA = torch.empty_like(moA)
    g_alpha = torch.zeros(1, device=DEV)
    stats = torch.zeros(4, device=DEV)
    e.sacc_actor_grad(moA, eps, act, g, q1, q2, log_alpha, dmoA, g_alpha,
                      stats, None, None, target_entropy)

    mu = moA[..., :A].detach().requires_grad_(True)
    ls = moA[..., A:].detach().requires_grad_(True)
    a_ref, lp_ref = _sacc_logpi(mu, ls, eps)
    alpha = float(log_alpha.exp())
    # surrogate: the q path's action gradient is exactly -g/N
    loss = (alpha * lp_ref).mean() - (a_ref * g).sum() / N
    loss.backward()
    torch.testing.assert_close(dmoA[..., :A], mu.grad, rtol=2e-4, atol=1e-6)
    torch.testing.assert_close(dmoA[..., A:], ls.grad, rtol=2e-4, atol=1e-6)
    # temperature grad + stats
    lp_mean = float(lp_ref.mean())
    assert abs(float(g_alpha) - (-(lp_mean + target_entropy))) < 1e-4
    l_ref = float((alpha * lp_ref.squeeze(-1)
                   - torch.min(q1, q2).view(B, S)).mean())
    assert abs(float(stats[0]) - l_ref) < 1e-4
    assert abs(float(stats[2]) - alpha) < 1e-6
    assert abs(float(stats[3]) + lp_mean) < 1e-4


@pytest.mark.gpu
def test_sacc_critic_loss_kernel_vs_torch():
    _ops()
    from pdrl_amd.ops import ext

    e = ext()
    B, S = 16, 6
    N = B * S
    torch.manual_seed(6)
    q1 = torch.randn(N, device=DEV, requires_grad=True)
    q2 = torch.randn(N, device=DEV, requires_grad=True)
    tq1 = torch.randn(N, device=DEV) * 3
    tq2 = torch.randn(N, device=DEV) * 3
    lp_next = torch.randn(N, device=DEV)
    rew = torch.rand(B, S, device=DEV)
    fir = (torch.rand(B, S, device=DEV) < 0.2).float()
    log_alpha = torch.tensor([-1.1], device=DEV)
    gamma, scale = 0.997, 0.7

    gq1 = torch.empty(N, device=DEV)
    gq2 = torch.empty(N, device=DEV)
    stats1 = torch.zeros(1, device=DEV)
    e.sacc_critic_loss(q1.detach(), q2.detach(), tq1, tq2, lp_next, rew, fir,
                       log_alpha, gq1, gq2, stats1, None, gamma, scale)

    alpha = float(log_alpha.exp())
    q1v = q1.view(B, S, 1)
    q2v = q2.view(B, S, 1)
    v_next = (torch.min(tq1, tq2).view(B, S, 1)
              - alpha * lp_next.view(B, S, 1))[:, 1:]
    y = scale * rew.view(B, S, 1)[:, :-1] + gamma * (
        1.0 - fir.view(B, S, 1)[:, 1:]) * v_next
    loss = torch.nn.functional.smooth_l1_loss(q1v[:, :-1], y) + \
        torch.nn.functional.smooth_l1_loss(q2v[:, :-1], y)
    loss.backward()
    assert abs(float(stats1[0]) - float(loss)) < 1e-4
    torch.testing.assert_close(gq1.view(B, S, 1), q1.grad.view(B, S, 1),
                               rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(gq2.view(B, S, 1), q2.grad.view(B, S, 1),
                               rtol=1e-4, atol=1e-7)


@pytest.mark.gpu
def test_sacc_fused_step_runs_and_learns():
    """Fused SAC-Continuous DAG: engages on GPU, stats finite, parameters
    and temperature move, targets Polyak-track. (Trajectory parity vs eager
    is not defined — the reparameterized sample differs per RNG — so the
    kernels are parity-tested individually above and the composition reuses
    the already-parity-tested core/wgrad/optimizer kernels.)"""
    _ops()
    from pdrl_amd.agents.learner_module import SACContinuousUpdater
    from pdrl_amd.networks import MlpLSTMSeperateContinuous
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 16, 5, 2, 1
    p.continuous = True
    p.lr = 1e-3

    torch.manual_seed(12)
    model = MlpLSTMSeperateContinuous(2, 1, p.seq_len, p.hidden_size)
    upd = SACContinuousUpdater(model, p, DEV)
    assert upd.fused_step is not None, "fused SAC-C step must engage"

    before = [q.detach().clone() for q in model.parameters()]
    t_before = [t.detach().clone() for t in upd.target_critic.parameters()]
    alpha_before = float(upd.log_alpha.detach())
    batch = make_batch(p, n_actions=1, continuous=True, device=DEV, seed=77)
    for _ in range(3):
        stats = upd.step(batch)
    for k in ("loss-actor", "loss-value", "loss-alpha", "alpha", "entropy"):
        assert torch.isfinite(torch.as_tensor(float(stats[k]))), k
    moved = sum(int(not torch.allclose(a, b.detach()))
                for a, b in zip(before, model.parameters()))
    assert moved > len(before) // 2
    assert float(upd.log_alpha.detach()) != alpha_before
    t_moved = sum(int(not torch.allclose(a, b.detach()))
                  for a, b in zip(t_before, upd.target_critic.parameters()))
    assert t_moved > 0


@pytest.mark.parametrize("hidden", [32, 128])
def test_updater_step_nonflagship_hidden(hidden):
    """H≠64 widths: the fused SeqLSTM core kernels (templated 32/64/128)
    drive autograd while the losses take the general path — one update
    must run and produce finite grads/params."""
    _ops()
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    torch.manual_seed(3)
    p = load_params()
    p.algo = "IMPALA"
    p.batch_size, p.seq_len, p.obs_dim, p.n_actions = 16, 5, 4, 2
    p.hidden_size = hidden
    upd_cls, model_cls = switch_module(p.algo)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, hidden)
    upd = upd_cls(model, p, DEV)
    batch = make_batch(p, device=DEV)
    for _ in range(2):
        stats = upd.step(batch)
    assert all(torch.isfinite(q).all() for q in model.parameters())
    assert all(abs(float(v)) < 1e6 for v in stats.values())


def test_weight_publisher_begin_finish_gpu_roundtrip():
    """WeightPublisher.begin()/finish() (the staged-bench pipelined split):
    payload matches the weights captured at begin() even if they change
    before finish()."""
    _ops()
    from pdrl_amd.agents.learner import WeightPublisher
    from pdrl_amd.buffers.wire import unpack_weights
    from pdrl_amd.networks import MlpLSTMSingle

    torch.manual_seed(2)
    m = MlpLSTMSingle(4, 2, 5, 64).to(DEV)
    pub = WeightPublisher(m.actor, DEV)
    ref = {k: v.detach().clone() for k, v in m.actor.state_dict().items()}
    pub.begin()
    # mutate AFTER begin: the D2H snapshot must hold the begin-time values
    with torch.no_grad():
        for q in m.actor.parameters():
            q.add_(1.0)
    sd = unpack_weights(pub.finish())
    for k in ref:
        torch.testing.assert_close(sd[k], ref[k].cpu())
