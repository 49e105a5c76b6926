"""Multi-network row-tile kernels at hidden size 128
(csrc/seq_lstm_tile128_multi.hip): the forward against float64 cores, forward
+ BPTT through the weight gradients they feed (and dx2) against float64
autograd, and the two fused SAC steps under ``rows_kernel="tile"`` against
``"row"`` at hidden size 128. Measured maxima are in profiles/sac_tile128.md.
All tests here require an MI355X."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPT = dict(device=DEV, dtype=torch.float32)
H = 128
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
    """One tile launch for all cores into NaN-filled outputs; outs, stash and
    the scratch sit in front of PAD sentinel rows. One dict per network."""
    B, S, _ = x.shape
    D = cores[0].out_dim
    nets = []
    for _ in cores:
        n = {k: torch.full((B + PAD, S, W), SENTINEL, **OPT)
             for k, W in (("outs_all", D), ("stash_all", 7 * H),
                          ("xw_all", 4 * H))}
        for k in ("outs", "stash", "xw"):
            n[k] = n[k + "_all"][:B].fill_(NAN)
        n["hS"] = torch.full((B, H), NAN, **OPT)
        n["cS"] = torch.full((B, H), NAN, **OPT)
        nets.append(n)
    core_tab = _t64([[c.body_w, c.body_b, c.w_ih, c.w_hh, c.b_g, c.heads_w,
                      c.heads_b, c.body2_w, c.body2_b, x2]
                     for c, x2 in zip(cores, x2s)])
    out_tab = _t64([[n["outs"], n["hS"], n["cS"], n["stash"]] for n in nets])
    xw_tab = _t64([[n["xw"] for n in nets]])[0]
    e.seq_lstm_fwd_tile128_multi(x, hx[:, 0], cx[:, 0], core_tab, out_tab,
                                 xw_tab, len(cores), D, F2=F2,
                                 half=HALF if F2 else 0)
    for n in nets:
        for k in ("outs", "stash", "xw"):
            assert bool((n[k + "_all"][B:] == SENTINEL).all()), f"{k} past B"
    return nets


def _eager(core, x, hx, cx, x2):
    dt = core.w_ih.dtype
    heads, h, c = core._forward_eager(
        x.to(dt), hx[:, 0].to(dt), cx[:, 0].to(dt),
        None if x2 is None else x2.to(dt))
    return heads["q"], h, c


@pytest.mark.parametrize("C,B,S,F,F2,D", [
    (5, 40, 5, 4, 0, 2),   # the SAC launch; two full tiles and one of 8 rows
    (2, 16, 1, 3, 1, 1),   # dual body; one tile; S = 1: no refill, no read-ahead
    (4, 17, 3, 3, 2, 1),   # the SAC-Continuous launch; one row in tile two
    (1, 33, 2, 4, 0, 3),   # a one-row table
    (2, 17, 40, 3, 2, 1),  # dual body; a sequence past 32 steps
])
def test_fwd_tile128_multi_vs_float64(C, B, S, F, F2, D):
    e = _ext()
    cores, cores64, x, hx, cx, x2s = _case(C, B, S, F, F2, D)
    nets = _forward(e, cores, x, hx, cx, x2s, F2)
    for k, (n, c, c64, x2) in enumerate(zip(nets, cores, cores64, x2s)):
        with torch.no_grad():
            ref = _eager(c64, x, hx, cx, x2)
            atol = 1e-5
            if S > 32:  # another summation order over 128 terms, 40 steps deep
                err = max(float((a.double() - r).abs().max())
                          for a, r in zip(_eager(c, x, hx, cx, x2), ref))
                atol = max(atol, 4.0 * err)
        for name, want in zip(("outs", "hS", "cS"), ref):
            got = n[name].double()
            print(f"net {k} {name}: max err "
                  f"{float((got - want).abs().max()):.3e}, atol {atol:.3e}")
            torch.testing.assert_close(got, want, rtol=0.0, atol=atol,
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
    e.seq_lstm_bwd_tile128_multi(x, cx[:, 0], in_tab, out_tab, len(cores),
                                 cores[0].out_dim, F2=F2,
                                 half=HALF if F2 else 0, accum_dx2=accum)


def _autograd64(c64, x, hx, cx, x2, gouts):
    """Gradients of (outs * gouts).sum() in the wgrad table's order, and
    x2.grad."""
    c64.zero_grad()
    x2d = None if x2 is None else x2.double().requires_grad_()
    outs, _, _ = _eager(c64, x, hx, cx, x2d)
    (outs * gouts.double()).sum().backward()
    ps = [c64.w_ih, c64.w_hh, c64.body_w, c64.body_b, c64.b_g, c64.heads_w,
          c64.heads_b] + ([c64.body2_w, c64.body2_b] if x2 is not None else [])
    return [p.grad.clone() for p in ps], None if x2 is None else x2d.grad


@pytest.mark.parametrize("C,B,S,F,F2,D", [(2, 40, 5, 4, 0, 2),
                                          (2, 17, 3, 3, 2, 1)])
def test_fwd_bwd_tile128_multi_vs_float64(C, B, S, F, F2, D):
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
    p.batch_size, p.seq_len, p.hidden_size = 40, 5, H
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
def test_sac_steps_tile_vs_row_hidden_128(algo, wgrad_kernel, monkeypatch):
    """One update (no graph) of the same updater with either rows_kernel,
    B = 40 (two full tiles and one of 8 rows), S = 5, at the figures of
    test_sac_steps_tile_vs_row."""
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
