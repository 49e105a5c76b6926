"""Multi-network split-K weight gradients (csrc/wgrad_split_multi.hip): exact
against a float64 reference on integer inputs (single- and dual-body cores,
several networks per launch), the shared norm accumulator, the SAC actor tail
against the sweep kernel's, and the two fused SAC steps built on it, past the
sweep kernels' 8192-row cap included. All tests here require an MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPT = dict(device=DEV, dtype=torch.float32)


def _ext():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops.ext()


def _inputs(nets, B, S, H, F, F2, D, seed, integer):
    """Shared x / h0 / x2 and one {stash, dgates, dxb, gouts} per network:
    small integers in {-2..2} (every partial sum is an integer below 2^24, so
    fp32 is exact in any order) or random at training magnitudes."""
    g = torch.Generator(device="cpu").manual_seed(seed)

    def mk(*shape, scale):
        if integer:
            return torch.randint(-2, 3, shape, generator=g).float().to(DEV)
        return (torch.randn(*shape, generator=g) * scale).to(DEV)

    shared = dict(x=mk(B, S, F, scale=1.0), h0=mk(B, H, scale=0.5),
                  x2=mk(B, S, F2, scale=1.0) if F2 else None)
    per_net = [dict(stash=mk(B, S, 7 * H, scale=0.5),
                    dgates=mk(B, S, 4 * H, scale=0.1),
                    dxb=mk(B, S, H, scale=0.1), gouts=mk(B, S, D, scale=0.1))
               for _ in range(nets)]
    return shared, per_net


def _reference(shared, t, H, half):
    """float64 einsums over n = (b, s), in the table's output order: dw_ih,
    dw_hh, dbody_w, dbody_b, db_g, dheads_w, dheads_b [, dbody2_w, dbody2_b].
    hprev is h0 at t = 0 and the stash h field of the step before."""
    d = {k: v.double() for k, v in {**shared, **t}.items() if v is not None}
    xb, h = d["stash"][..., :H], d["stash"][..., 6 * H:]
    hprev = torch.cat([d["h0"][:, None, :], h[:, :-1, :]], dim=1)
    ref = [
        torch.einsum("bsm,bsg->mg", xb, d["dgates"]),
        torch.einsum("bsm,bsg->mg", hprev, d["dgates"]),
        torch.einsum("bsf,bsj->fj", d["x"], d["dxb"][..., :half]),
        d["dxb"][..., :half].sum((0, 1)),
        d["dgates"].sum((0, 1)),
        torch.einsum("bsk,bsd->kd", h, d["gouts"]),
        d["gouts"].sum((0, 1)),
    ]
    if half < H:
        ref += [torch.einsum("bsf,bsj->fj", d["x2"], d["dxb"][..., half:]),
                d["dxb"][..., half:].sum((0, 1))]
    return ref


def _outputs(H, F, F2, D, half):
    shapes = [(H, 4 * H), (H, 4 * H), (F, half), (half,), (4 * H,), (H, D),
              (D,)] + ([(F2, H - half), (H - half,)] if half < H else [])
    return [torch.full(s, float("nan"), **OPT) for s in shapes]


def _table(per_net, outs, norm):
    rows = []
    for t, o in zip(per_net, outs):
        o = o + [None] * (9 - len(o))
        ptr = [t["stash"], t["dgates"], t["dxb"], t["gouts"], *o[:7], norm,
               o[7], o[8]]
        rows.append([0 if v is None else v.data_ptr() for v in ptr])
    return torch.tensor(rows, dtype=torch.int64).to(DEV)


def _launch(e, shared, tab, nets, dims, slab_rows):
    """(run, tickets) for one shape; the tickets are zeroed here once."""
    B, S, H, F, F2, D, half = dims
    floats, n_tickets = e.seq_lstm_wgrad_split_multi_workspace(
        B * S, H, F, F2, D, nets, slab_rows)
    ws = torch.empty(max(floats, 1), **OPT)
    tickets = torch.zeros(n_tickets, device=DEV, dtype=torch.int32)
    dual = dict(x2=shared["x2"], F2=F2, half=half) if F2 else {}

    def run():
        e.seq_lstm_wgrad_split_multi(shared["x"], shared["h0"], tab, nets, D,
                                     ws, tickets, slab_rows, **dual)
    return run, tickets


@pytest.mark.parametrize("nets,B,S,H,F,F2,D,slab_rows", [
    (1, 3, 5, 64, 4, 0, 3, 0),      # one slab: direct write, no ticket
    (2, 11, 3, 64, 4, 0, 2, 8),     # ragged multi-slab, last slab 1 row
    (2, 8, 4, 64, 3, 1, 1, 6),      # dual, boundaries mid-sequence, half 32
    (2, 11, 3, 32, 3, 2, 1, 8),     # dual, half = 16: one tile per body
    (2, 5, 7, 128, 3, 1, 1, 12),    # dual, H = 128
    (2, 1640, 5, 64, 3, 1, 1, 0),   # dual, N = 8200 > 8192, host heuristic
])
def test_split_multi_vs_float64_exact(nets, B, S, H, F, F2, D, slab_rows):
    e = _ext()
    half = H // 2 if F2 else H
    shared, per_net = _inputs(nets, B, S, H, F, F2, D, seed=1000 * B + S,
                              integer=True)
    outs = [_outputs(H, F, F2, D, half) for _ in range(nets)]
    run, tickets = _launch(e, shared, _table(per_net, outs, None), nets,
                           (B, S, H, F, F2, D, half), slab_rows)
    refs = [_reference(shared, t, H, half) for t in per_net]
    for call in (1, 2):  # the second call proves the tickets reset themselves
        for o in outs:
            for g_ in o:
                g_.fill_(float("nan"))
        run()
        for c, (o, ref) in enumerate(zip(outs, refs)):
            for i, (g_, r_) in enumerate(zip(o, ref)):
                assert torch.equal(g_.double(), r_), (c, i, call)
    assert int(tickets.abs().sum()) == 0


def test_split_multi_norm_sq_shared():
    """Two dual-body networks add into ONE norm scalar, as the twin critics
    do: one float atomicAdd per finishing workgroup, each of a float sum of
    squares. The total equals the float64 sum of squares of the outputs up to
    the any-order rounding of a sum of M positive terms, M * 2^-24 relative,
    M the number of gradient elements (the bound of test_split_norm_sq)."""
    e = _ext()
    nets, B, S, H, F, F2, D, slab_rows = 2, 11, 3, 64, 3, 1, 1, 8
    half = H // 2
    shared, per_net = _inputs(nets, B, S, H, F, F2, D, seed=88, integer=False)
    outs = [_outputs(H, F, F2, D, half) for _ in range(nets)]
    norm = torch.zeros(1, **OPT)
    run, _ = _launch(e, shared, _table(per_net, outs, norm), nets,
                     (B, S, H, F, F2, D, half), slab_rows)
    run()
    for o, t in zip(outs, per_net):
        for g_, r_ in zip(o, _reference(shared, t, H, half)):
            torch.testing.assert_close(g_.double(), r_, rtol=1e-4, atol=1e-5)
    want = sum(float((g_.double() ** 2).sum()) for o in outs for g_ in o)
    bound = sum(g_.numel() for o in outs for g_ in o) * 2.0 ** -24
    rel = abs(float(norm) - want) / want
    print(f"shared norm_sq rel err {rel:.3e} bound {bound:.3e}")
    assert rel <= bound, (float(norm), want, rel)


def test_sac_actor_tail_matches_sweep():
    """sac_actor_wgrad_split against sac_actor_wgrad on the same partials,
    log_alpha and clock: the tail is the same device function, so g_alpha,
    stats4 and the clock agree bit for bit; the seven gradients are exact
    against float64 on integer inputs (7 slabs of 16 rows)."""
    e = _ext()
    B, S, H, F, D, slab_rows = 37, 3, 64, 4, 3, 16
    shared, (t,) = _inputs(1, B, S, H, F, 0, D, seed=37, integer=True)
    g = torch.Generator(device="cpu").manual_seed(5)
    part = torch.randn(B, 2, generator=g).to(DEV)
    log_alpha = torch.tensor([-0.7], **OPT)
    floats, n_tickets = e.seq_lstm_wgrad_split_multi_workspace(
        B * S, H, F, 0, D, 1, slab_rows)
    tickets = torch.zeros(n_tickets, device=DEV, dtype=torch.int32)
    got = {}
    for kernel in ("sweep", "split"):
        outs = _outputs(H, F, 0, D, H)
        tail = dict(g_alpha=torch.zeros(1, **OPT), stats4=torch.zeros(4, **OPT),
                    clock=torch.tensor([3.0, 0.5, 0.25], **OPT),
                    norm=torch.zeros(1, **OPT))
        args = (shared["x"], shared["h0"], t["stash"], t["dgates"], t["dxb"],
                t["gouts"], *outs, tail["norm"], part, log_alpha,
                tail["g_alpha"], tail["stats4"], None, tail["clock"], 0.35,
                0.9, 0.999)
        if kernel == "split":
            e.sac_actor_wgrad_split(*args, torch.empty(max(floats, 1), **OPT),
                                    tickets, slab_rows)
        else:
            e.sac_actor_wgrad(*args)
        got[kernel] = (outs, tail)
    for k in ("g_alpha", "stats4", "clock"):
        assert torch.equal(got["split"][1][k], got["sweep"][1][k]), k
    assert float(got["split"][1]["clock"][0]) == 4.0
    for i, (g_, r_) in enumerate(zip(got["split"][0],
                                     _reference(shared, t, H, H))):
        assert torch.equal(g_.double(), r_), i
    assert int(tickets.abs().sum()) == 0


def _sac_updater(algo, bsz, wgrad_kernel, seed, lr=None):
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    continuous = algo.endswith("Continuous")
    p = load_params()
    p.algo, p.wgrad_kernel = algo, wgrad_kernel
    p.batch_size, p.seq_len, p.hidden_size = bsz, 5, 64
    p.obs_dim, p.n_actions = (3, 1) if continuous else (4, 2)
    if lr is not None:
        p.lr = lr
    upd_cls, model_cls = switch_module(algo)
    torch.manual_seed(seed)  # the model and, for SAC-C, the step's rng
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    upd = upd_cls(model, p, DEV)
    assert upd.fused_step is not None, "fused SAC step must engage"
    batch = make_batch(p, n_actions=p.n_actions, continuous=continuous,
                       device=DEV, seed=55)
    return upd, model, batch


@pytest.mark.parametrize("fast", ["1", "0"])
@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
def test_sac_steps_split_vs_sweep(algo, fast, monkeypatch):
    """One update (no graph: a captured step warms up with three more) of
    the same updater with either kernel, B = 64, S = 5: N = 320 rows, several
    slabs under the heuristic. Optimizer gradients at the project's figure
    for split against autograd (1e-4, 1e-6); measured maxima are in
    profiles/sac_split.md."""
    _ext()
    monkeypatch.setenv("PDRL_SAC8", fast)
    monkeypatch.setenv("PDRL_USE_GRAPH", "0")
    ups = {}
    for kernel in ("sweep", "split"):
        upd, _, batch = _sac_updater(algo, 64, kernel, seed=7)
        assert upd.fused_step.wgrad_kernel == kernel
        upd.step(batch)
        ups[kernel] = upd
    for name in ("actor_optimizer", "critic_optimizer"):
        a = getattr(ups["split"], name).flat_grad
        b = getattr(ups["sweep"], name).flat_grad
        err = (a - b).abs()
        print(f"{algo} fast={fast} {name}: max abs {float(err.max()):.3e} "
              f"max |g| {float(b.abs().max()):.3e}")
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6,
                                   msg=lambda m: f"{algo} {name}: {m}")
    # absolute floor: one fp32 ulp at 1 (loss-alpha = log(alpha) * dlog_alpha
    # may cancel to nearly 0, where a relative bound alone means nothing)
    torch.testing.assert_close(ups["split"].fused_step.stats_buf,
                               ups["sweep"].fused_step.stats_buf,
                               rtol=1e-5, atol=2.0 ** -23)


def test_sac_past_cap_tracks_eager():
    """B = 2048, S = 5 (N = 10240 > 8192): the split step fits and engages,
    and three updates track the eager updater from the same init (protocol
    and tolerances of test_sac_fused_step_parity; Adam at lr = 1e-4 bounds
    the movement, the sharp checks are the tests above)."""
    _ext()
    upd_f, model_f, batch = _sac_updater("SAC", 2048, "split", 11, lr=1e-4)
    upd_e, model_e, _ = _sac_updater("SAC", 2048, "split", 11, lr=1e-4)
    assert upd_f.fused_step.fits(batch)
    upd_e.fused_step = None  # force the eager path on the same GPU
    for _ in range(3):
        sf = upd_f.step(batch)
        se = upd_e.step(batch)
    for (n, pf), pe in zip(model_f.named_parameters(), model_e.parameters()):
        torch.testing.assert_close(pf.detach(), pe.detach(), rtol=5e-3,
                                   atol=5e-4, msg=lambda m: f"{n}: {m}")
    torch.testing.assert_close(upd_f.log_alpha.detach(),
                               upd_e.log_alpha.detach(), rtol=1e-3, atol=1e-5)
    for k in ("loss-actor", "loss-value", "loss-alpha", "alpha", "entropy"):
        assert abs(float(sf[k]) - float(se[k])) < 5e-2, (k, sf[k], se[k])
    for tf, te in zip(upd_f.target_critic.parameters(),
                      upd_e.target_critic.parameters()):
        torch.testing.assert_close(tf.detach(), te.detach(), rtol=5e-3,
                                   atol=5e-4)


def test_sacc_past_cap_engages():
    """SAC-Continuous at N = 10240 rows: fits, one step, finite stats,
    parameters and target critic moved."""
    _ext()
    upd, model, batch = _sac_updater("SAC-Continuous", 2048, "split", 13)
    assert upd.fused_step.fits(batch)
    before = [q.detach().clone() for q in model.parameters()]
    target = [q.detach().clone() for q in upd.target_critic.parameters()]
    stats = upd.step(batch)
    assert all(math.isfinite(float(v)) for v in stats.values()), stats
    for name, old, new in (("model", before, model.parameters()),
                           ("target", target,
                            upd.target_critic.parameters())):
        moved = sum(float((a - b.detach()).abs().sum())
                    for a, b in zip(old, new))
        assert moved > 0.0, name
