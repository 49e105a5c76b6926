"""seq_lstm_row_step (forward + loss + BPTT per row in one launch, stats
reduce in the wgrad launch) against the two-launch pair it replaces,
seq_lstm_fwd_loss + seq_lstm_bwd_fin. Both sides run the same device
functions in the same order, so every array must be equal BIT FOR BIT; a
difference is an ordering bug, not rounding. All tests here require an
MI355X."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 64
ALGO_ID = {"IMPALA": 0, "PPO": 1, "PPO-C": 2}
# gamma, lmbda, rho_bar, rho_min, c_bar, rew_scale, cp, cv, ce, eps_clip, creg
HYPER = (0.99, 0.95, 0.8, 0.1, 1.0, 0.1, 1.0, 0.5, 0.01, 0.2, 1e-3)
COEFS = (HYPER[6], HYPER[7], HYPER[8], HYPER[10])  # cp, cv, ce, creg
GRADS = ("dw_ih", "dw_hh", "dbody_w", "dbody_b", "db_g", "dheads_w",
         "dheads_b")
ARRAYS = ("outs", "hS", "cS", "stash", "gouts", "dgates", "dxb")

# (B, S, A) for IMPALA and PPO, obs 4
DISCRETE_SHAPES = [
    (1, 2, 2),    # T = 1, and the only block is block 0
    (3, 3, 2),    # small plain case
    (7, 8, 5),    # S·H = 512 > 256 threads: every strided loop runs twice
    (16, 5, 2),   # the flagship row shape
    (300, 2, 2),  # B > 256: the stats reduce strides
]
CASES = ([(algo, *shape) for algo in ("IMPALA", "PPO")
          for shape in DISCRETE_SHAPES] +
         [("PPO-C", 3, 3, 1), ("PPO-C", 7, 8, 3)])  # obs 2


def _ext():
    from pdrl_amd import ops

    assert ops.available(), "HIP extension must be loaded on a GPU box"
    return ops.ext()


@functools.lru_cache(maxsize=None)
def _inputs(algo, B, S, A):
    """Seeded random operands at training magnitudes; read-only."""
    g = torch.Generator(device="cpu").manual_seed(1000 * B + 10 * S + A)
    cont = algo == "PPO-C"
    F = 2 if cont else 4
    D = 2 * A + 1 if cont else A + 1

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(DEV)

    t = dict(
        x=rnd(B, S, F),
        # row views with stride S·H, as the step takes them from the batch
        h0=rnd(B, S, H, scale=0.5)[:, 0], c0=rnd(B, S, H, scale=0.5)[:, 0],
        body_w=rnd(F, H, scale=0.5), body_b=rnd(H, scale=0.1),
        w_ih=rnd(H, 4 * H, scale=0.125), w_hh=rnd(H, 4 * H, scale=0.125),
        b_g=rnd(4 * H, scale=0.1), heads_w=rnd(H, D, scale=0.125),
        heads_b=rnd(D, scale=0.1),
        behav=rnd(B, S, scale=0.3) - 0.7, rew=rnd(B, S),
        fir=(torch.rand(B, S, generator=g) < 0.2).float().to(DEV),
    )
    if cont:
        t["act"] = rnd(B, S, A).reshape(-1)
    else:
        t["act"] = torch.randint(0, A, (B * S,), generator=g).float().to(DEV)
    return t, D


def _workspace(B, S, D):
    def mk(*shape):
        return torch.full(shape, -7.0, device=DEV)

    ws = dict(outs=mk(B, S, D), hS=mk(B, H), cS=mk(B, H),
              stash=mk(B, S, 7 * H), gouts=mk(B, S, D), dgates=mk(B, S, 4 * H),
              dxb=mk(B, S, H), stats_part=mk(B, 8), stats=mk(8))
    return ws


def _grad_bufs(F, D):
    shapes = dict(dw_ih=(H, 4 * H), dw_hh=(H, 4 * H), dbody_w=(F, H),
                  dbody_b=(H,), db_g=(4 * H,), dheads_w=(H, D),
                  dheads_b=(D,))
    return {n: torch.full(shapes[n], -7.0, device=DEV) for n in GRADS}


def _weights(t):
    return (t["body_w"], t["body_b"], t["w_ih"], t["w_hh"], t["b_g"],
            t["heads_w"], t["heads_b"])


@functools.lru_cache(maxsize=None)
def _pair(algo, B, S, A):
    """The reference: seq_lstm_fwd_loss + seq_lstm_bwd_fin + wgrad_out,
    computed once per case and left unchanged."""
    e = _ext()
    t, D = _inputs(algo, B, S, A)
    ws = _workspace(B, S, D)
    e.seq_lstm_fwd_loss(
        t["x"], t["h0"], t["c0"], *_weights(t), ws["outs"], ws["hS"],
        ws["cS"], ws["stash"], t["act"], t["behav"], t["rew"], t["fir"],
        ws["gouts"], ws["stats_part"], None, ALGO_ID[algo], *HYPER)
    e.seq_lstm_bwd_fin(
        ws["gouts"], ws["stash"], t["x"], t["c0"], t["body_w"], t["w_ih"],
        t["w_hh"], t["heads_w"], ws["dgates"], ws["dxb"], ws["stats"],
        ws["stats_part"], ALGO_ID[algo], *COEFS)
    grads = _grad_bufs(t["x"].size(2), D)
    e.seq_lstm_wgrad_out(t["x"], t["h0"], ws["stash"], ws["dgates"],
                         ws["dxb"], ws["gouts"], *[grads[n] for n in GRADS],
                         None)
    torch.cuda.synchronize()
    return ws, grads


def _row_step(algo, B, S, A, norm_sq):
    e = _ext()
    t, D = _inputs(algo, B, S, A)
    ws = _workspace(B, S, D)
    e.seq_lstm_row_step(
        t["x"], t["h0"], t["c0"], *_weights(t), ws["outs"], ws["hS"],
        ws["cS"], ws["stash"], t["act"], t["behav"], t["rew"], t["fir"],
        ws["gouts"], ws["stats_part"], norm_sq, ws["dgates"], ws["dxb"],
        ALGO_ID[algo], *HYPER)
    grads = _grad_bufs(t["x"].size(2), D)
    cp, cv, ce, creg = COEFS
    e.seq_lstm_wgrad_out(t["x"], t["h0"], ws["stash"], ws["dgates"],
                         ws["dxb"], ws["gouts"], *[grads[n] for n in GRADS],
                         None, stats_part=ws["stats_part"], stats=ws["stats"],
                         algo=ALGO_ID[algo], B=B, cp=cp, cv=cv, ce=ce,
                         creg=creg)
    torch.cuda.synchronize()
    return ws, grads


@pytest.mark.parametrize("algo,B,S,A", CASES)
def test_row_step_equals_two_launch_pair(algo, B, S, A):
    ref_ws, ref_grads = _pair(algo, B, S, A)
    nstat = 5 if algo == "IMPALA" else 7  # written stat columns / entries

    norm = torch.full((1,), 3.5, device=DEV)
    ws, grads = _row_step(algo, B, S, A, norm)
    _assert_same(ws, grads, ref_ws, ref_grads, nstat)
    assert norm.item() == 0.0, "block 0 must zero norm_sq"


def _assert_same(ws, grads, ref_ws, ref_grads, nstat):
    for n in ARRAYS:
        assert torch.equal(ws[n], ref_ws[n]), f"{n} differs"
    assert torch.equal(ws["stats_part"][:, :nstat],
                       ref_ws["stats_part"][:, :nstat]), "stats_part differs"
    assert torch.equal(ws["stats"][:nstat], ref_ws["stats"][:nstat]), \
        f"stats differ: {ws['stats'][:nstat]} vs {ref_ws['stats'][:nstat]}"
    for n in GRADS:
        assert torch.equal(grads[n], ref_grads[n]), f"{n} differs"


@pytest.mark.parametrize("algo,B,S,A", [("IMPALA", 3, 3, 2),
                                        ("PPO-C", 3, 3, 1)])
def test_row_step_without_norm_buffer(algo, B, S, A):
    """norm_sq=None: block 0 has nothing to zero, every result is the same."""
    ref_ws, ref_grads = _pair(algo, B, S, A)
    ws, grads = _row_step(algo, B, S, A, None)
    _assert_same(ws, grads, ref_ws, ref_grads, 5 if algo == "IMPALA" else 7)


def test_row_step_rejects_vmpo():
    e = _ext()
    t, D = _inputs("IMPALA", 3, 3, 2)
    ws = _workspace(3, 3, D)
    with pytest.raises(RuntimeError, match="V-MPO"):
        e.seq_lstm_row_step(
            t["x"], t["h0"], t["c0"], *_weights(t), ws["outs"], ws["hS"],
            ws["cS"], ws["stash"], t["act"], t["behav"], t["rew"], t["fir"],
            ws["gouts"], ws["stats_part"], None, ws["dgates"], ws["dxb"], 3,
            *HYPER)


# The row step parks S*(D + act_per + 3) floats of loss inputs in LDS behind
# the forward's buffers. At S = 100 with 28 actions (D = 29) that is 65,936
# bytes, over the 64 KiB of a launch, while the two-launch pair needs 54,272.
LONG_WIDE = dict(B=2, S=100, A=28)


def test_row_step_lds_need_and_limit():
    e = _ext()
    # flagship: BPTT's (2*S*H + 12*H) floats are the largest phase
    assert e.seq_lstm_row_step_lds_bytes(5, 3, 0) == (2 * 5 * 64 + 12 * 64) * 4
    S, D = LONG_WIDE["S"], LONG_WIDE["A"] + 1
    need = (2 * S * 64 + 6 * 64 + S * (D + 1 + 3)) * 4
    assert need > 64 * 1024
    assert e.seq_lstm_row_step_lds_bytes(S, D, 0) == need
    t, D = _inputs("IMPALA", *LONG_WIDE.values())
    ws = _workspace(LONG_WIDE["B"], S, D)
    with pytest.raises(RuntimeError, match="LDS"):
        e.seq_lstm_row_step(
            t["x"], t["h0"], t["c0"], *_weights(t), ws["outs"], ws["hS"],
            ws["cS"], ws["stash"], t["act"], t["behav"], t["rew"], t["fir"],
            ws["gouts"], ws["stats_part"], None, ws["dgates"], ws["dxb"], 0,
            *HYPER)


def test_fused_step_falls_back_to_pair_beyond_lds():
    """A shape the two-launch pair runs but the row step's LDS does not fit:
    the fused step must route to the pair (same bits as forcing the pair)."""
    _ext()
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params
    from tests.conftest import make_batch

    p = load_params()
    p.algo = "IMPALA"
    p.batch_size, p.seq_len, p.hidden_size = LONG_WIDE["B"], LONG_WIDE["S"], H
    p.obs_dim, p.n_actions = 4, LONG_WIDE["A"]
    torch.manual_seed(5)
    model = MlpLSTMSingle(4, p.n_actions, p.seq_len, H)
    upd = ImpalaUpdater(model, p, DEV)
    batch = make_batch(p, n_actions=p.n_actions, device=DEV, seed=9)
    fs = upd.fused_step
    assert fs is not None and fs.row_step and fs.fits(batch)
    e = _ext()
    n_cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    D = p.n_actions + 1
    assert fs._runs_row_step(e, n_cus, 5, 3)        # a CU for every row
    assert not fs._runs_row_step(e, n_cus + 1, 5, 3)  # rows share CUs: pair
    assert not fs._runs_row_step(e, p.batch_size, p.seq_len, D)  # LDS

    def grads_and_stats():
        upd.optimizer.zero_grad()
        fs.stats_buf.fill_(-7.0)
        fs.compute_grads_only(batch)
        torch.cuda.synchronize()
        return ([q.grad.detach().clone() for q in model.parameters()],
                fs.stats_buf[:5].clone())

    got, got_stats = grads_and_stats()
    fs.row_step = False  # the two-launch pair, whatever the shape
    want, want_stats = grads_and_stats()
    for g, w in zip(got, want):
        assert torch.isfinite(g).all() and torch.equal(g, w)
    assert torch.equal(got_stats, want_stats)
