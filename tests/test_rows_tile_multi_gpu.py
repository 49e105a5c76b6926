"""Multi-network row-tile kernels (csrc/seq_lstm_tile_multi.hip): the forward
against float64 cores, forward + BPTT through the weight gradients they feed
(and dx2) against float64 autograd, and the two fused SAC steps under
``rows_kernel="tile"`` against ``"row"``. Measured maxima are in
profiles/sac_tile.md. All tests here require an MI355X."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPT = dict(device=DEV, dtype=torch.float32)
H = 64
HALF = H // 2
SENTINEL = -12345.0
PAD = 16  # spare rows behind B: a ragged tile must leave them alone
NAN = float("nan")


def _ext():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops.ext()


def _t64(rows):
    return torch.tensor([[0 if v is None else v.data_ptr() for v in r]
                         for r in rows], dtype=torch.int64).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(C, B, S, F, F2, D):
    """C cores with their own weights (and, dual body, their own x2), their
    float64 copies, and the shared x, hx, cx ((B, S, H): the kernels get the
    [:, 0] views, as in the steps)."""
    from pdrl_amd.networks.models import SeqLSTMCore

    torch.manual_seed(1000 * B + 10 * S + C)
    cores = [SeqLSTMCore(F, H, {"q": D}, input2_dim=F2 or None).to(DEV)
             for _ in range(C)]
    x = torch.randn(B, S, F, **OPT)
    hx = torch.randn(B, S, H, **OPT) * 0.5
    cx = torch.randn(B, S, H, **OPT) * 0.5
    x2s = [torch.randn(B, S, F2, **OPT) if F2 else None for _ in range(C)]
    return cores, [copy.deepcopy(c).double() for c in cores], x, hx, cx, x2s


def _forward(e, cores, x, hx, cx, x2s, F2):
    """One tile launch for all cores into NaN-filled outputs; outs and stash
    sit in front of PAD sentinel rows. Returns one dict per network."""
    B, S, _ = x.shape
    D = cores[0].out_dim
    nets = []
    for _ in cores:
        outs_all = torch.full((B + PAD, S, D), SENTINEL, **OPT)
        stash_all = torch.full((B + PAD, S, 7 * H), SENTINEL, **OPT)
        outs_all[:B] = NAN
        stash_all[:B] = NAN
        nets.append(dict(outs_all=outs_all, stash_all=stash_all,
                         outs=outs_all[:B], stash=stash_all[:B],
                         hS=torch.full((B, H), NAN, **OPT),
                         cS=torch.full((B, H), NAN, **OPT)))
    core_tab = _t64([[c.body_w, c.body_b, c.w_ih, c.w_hh, c.b_g, c.heads_w,
                      c.heads_b, c.body2_w, c.body2_b, x2]
                     for c, x2 in zip(cores, x2s)])
    out_tab = _t64([[n["outs"], n["hS"], n["cS"], n["stash"]] for n in nets])
    e.seq_lstm_fwd_tile_multi(x, hx[:, 0], cx[:, 0], core_tab, out_tab,
                              len(cores), D, F2=F2, half=HALF if F2 else 0)
    for n in nets:
        assert bool((n["outs_all"][B:] == SENTINEL).all()), "outs past B"
        assert bool((n["stash_all"][B:] == SENTINEL).all()), "stash past B"
    return nets


def _eager64(core64, x, hx, cx, x2):
    heads, h, c = core64._forward_eager(
        x.double(), hx[:, 0].double(), cx[:, 0].double(), x2)
    return heads["q"], h, c


@pytest.mark.parametrize("C,B,S,F,F2,D", [
    (5, 40, 5, 4, 0, 2),   # the SAC launch; two full tiles and one of 8 rows
    (2, 16, 1, 3, 1, 1),   # dual body; exactly one tile; S = 1 (no refill)
    (4, 17, 3, 3, 2, 1),   # the SAC-Continuous launch; one row in tile two
    (1, 33, 2, 4, 0, 3),   # a one-row table
])
def test_fwd_tile_multi_vs_float64(C, B, S, F, F2, D):
    e = _ext()
    cores, cores64, x, hx, cx, x2s = _case(C, B, S, F, F2, D)
    nets = _forward(e, cores, x, hx, cx, x2s, F2)
    for k, (n, c64, x2) in enumerate(zip(nets, cores64, x2s)):
        with torch.no_grad():
            ref = _eager64(c64, x, hx, cx, None if x2 is None else x2.double())
        for name, want in zip(("outs", "hS", "cS"), ref):
            got = n[name].double()
            print(f"net {k} {name}: max err "
                  f"{float((got - want).abs().max()):.3e}")
            torch.testing.assert_close(got, want, rtol=0.0, atol=1e-5,
                                       msg=lambda m: f"net {k} {name}: {m}")


def _backward(e, cores, nets, gouts, x, cx, dx2s, F2, accum):
    """One tile BPTT launch for all cores; dgates/dxb NaN-filled."""
    B, S, _ = x.shape
    for n in nets:
        n["dgates"] = torch.full((B, S, 4 * H), NAN, **OPT)
        n["dxb"] = torch.full((B, S, H), NAN, **OPT)
    in_tab = _t64([[g_, n["stash"], c.w_ih, c.w_hh, c.heads_w, c.body_w,
                    c.body2_w] for c, n, g_ in zip(cores, nets, gouts)])
    out_tab = _t64([[n["dgates"], n["dxb"], d_] for n, d_ in zip(nets, dx2s)])
    e.seq_lstm_bwd_tile_multi(x, cx[:, 0], in_tab, out_tab, len(cores),
                              cores[0].out_dim, F2=F2,
                              half=HALF if F2 else 0, accum_dx2=accum)


def _autograd64(c64, x, hx, cx, x2, gouts):
    """Gradients of (outs * gouts).sum() in the wgrad table's order, and
    x2.grad."""
    c64.zero_grad()
    x2d = None if x2 is None else x2.double().requires_grad_()
    outs, _, _ = _eager64(c64, x, hx, cx, x2d)
    (outs * gouts.double()).sum().backward()
    ps = [c64.w_ih, c64.w_hh, c64.body_w, c64.body_b, c64.b_g, c64.heads_w,
          c64.heads_b] + ([c64.body2_w, c64.body2_b] if x2 is not None else [])
    return [p.grad.clone() for p in ps], None if x2 is None else x2d.grad


@pytest.mark.parametrize("C,B,S,F,F2,D", [(2, 40, 5, 4, 0, 2),
                                          (2, 17, 3, 3, 2, 1)])
def test_fwd_bwd_tile_multi_vs_float64(C, B, S, F, F2, D):
    e = _ext()
    cores, cores64, x, hx, cx, x2s = _case(C, B, S, F, F2, D)
    gouts = [torch.randn(B, S, D, **OPT) * 0.1 for _ in cores]
    nets = _forward(e, cores, x, hx, cx, x2s, F2)
    dx2s = [torch.full((B, S, F2), NAN, **OPT) if F2 else None for _ in cores]
    _backward(e, cores, nets, gouts, x, cx, dx2s, F2, accum=False)
    names = ("dw_ih", "dw_hh", "dbody_w", "dbody_b", "db_g", "dheads_w",
             "dheads_b", "dbody2_w", "dbody2_b")
    for k, (c, c64, n) in enumerate(zip(cores, cores64, nets)):
        want, want_dx2 = _autograd64(c64, x, hx, cx, x2s[k], gouts[k])
        grads = [torch.full(w.shape, NAN, **OPT) for w in want]
        tab = _t64([[n["stash"], n["dgates"], n["dxb"], gouts[k], *grads[:7],
                     None, *(grads[7:] if F2 else (None, None))]])
        dual = dict(x2=x2s[k], F2=F2, half=HALF) if F2 else {}
        e.seq_lstm_wgrad_multi(x, hx[:, 0], tab, 1, D, **dual)
        if F2:
            grads.append(dx2s[k])
            want.append(want_dx2)
        for name, g_, w_ in zip(names + ("dx2",), grads, want):
            print(f"net {k} {name}: max err "
                  f"{float((g_.double() - w_).abs().max()):.3e}")
            torch.testing.assert_close(g_.double(), w_, rtol=1e-4, atol=1e-5,
                                       msg=lambda m: f"net {k} {name}: {m}")
    if not F2:
        return
    # the twin critics: one shared x2, both networks add into one zeroed dx2
    shared = [x2s[0]] * C
    nets = _forward(e, cores, x, hx, cx, shared, F2)
    dact = torch.zeros(B, S, F2, **OPT)
    _backward(e, cores, nets, gouts, x, cx, [dact] * C, F2, accum=True)
    want = sum(_autograd64(c64, x, hx, cx, x2s[0], g_)[1]
               for c64, g_ in zip(cores64, gouts))
    print(f"accumulated dx2: max err "
          f"{float((dact.double() - want).abs().max()):.3e}")
    torch.testing.assert_close(dact.double(), want, rtol=1e-4, atol=1e-5)


def _sac_updater(algo, rows_kernel, wgrad_kernel):
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    continuous = algo.endswith("Continuous")
    p = load_params()
    p.algo, p.rows_kernel, p.wgrad_kernel = algo, rows_kernel, wgrad_kernel
    p.batch_size, p.seq_len, p.hidden_size = 40, 5, 64
    p.obs_dim, p.n_actions = (3, 1) if continuous else (4, 2)
    upd_cls, model_cls = switch_module(algo)
    torch.manual_seed(7)  # the model and, for SAC-C, the step's rng
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    upd = upd_cls(model, p, DEV)
    assert upd.fused_step is not None, "fused SAC step must engage"
    assert upd.fused_step.rows_kernel == rows_kernel
    batch = make_batch(p, n_actions=p.n_actions, continuous=continuous,
                       device=DEV, seed=55)
    return upd, batch


@pytest.mark.parametrize("wgrad_kernel", ["sweep", "split"])
@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
def test_sac_steps_tile_vs_row(algo, wgrad_kernel, monkeypatch):
    """One update (no graph) of the same updater with either rows_kernel,
    B = 40 (two full tiles and one of 8 rows), S = 5, at the figures of
    test_sac_steps_split_vs_sweep."""
    _ext()
    monkeypatch.setenv("PDRL_USE_GRAPH", "0")
    ups = {}
    for rows_kernel in ("row", "tile"):
        upd, batch = _sac_updater(algo, rows_kernel, wgrad_kernel)
        upd.step(batch)
        ups[rows_kernel] = upd
    for name in ("actor_optimizer", "critic_optimizer"):
        a = getattr(ups["tile"], name).flat_grad
        b = getattr(ups["row"], name).flat_grad
        print(f"{algo} {wgrad_kernel} {name}: max abs "
              f"{float((a - b).abs().max()):.3e} max |g| "
              f"{float(b.abs().max()):.3e}")
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6,
                                   msg=lambda m: f"{algo} {name}: {m}")
    sa, sb = ups["tile"].fused_step.stats_buf, ups["row"].fused_step.stats_buf
    print(f"{algo} {wgrad_kernel} stats: tile {sa.tolist()} row {sb.tolist()}")
    torch.testing.assert_close(sa, sb, rtol=1e-5, atol=2.0 ** -23)
