"""Greedy device evaluation on the GPU: the evaluation kernels against the
eager fp32 reference (same weights, same counter-hash start states), their
live-weight / storage / argument contracts, and the learner end to end."""
import copy
import functools
import math

import pytest
import torch

from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.networks.models import (MlpLSTMSeperateContinuous,
                                      MlpLSTMSingleContinuous)
from pdrl_amd.ops.evaluate import DeviceEvaluator

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CART, CAR = "CartPole-v1", "MountainCarContinuous-v0"
S = 5
MAX_STEPS = 40  # the 40-tick regime of profiles/device_rollout.md
MARGIN = 1e-4  # envs whose smallest decision margin is below this are excluded
EVAL_SEED = 1


def _cartpole_model(hidden, scale):
    """Model seed 0 with ``body_w *= scale`` and zero head biases: an
    untrained core never changes its arg-max action, this one does."""
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, S, hidden)
    with torch.no_grad():
        model.actor.core.body_w *= scale
        model.actor.core.heads_b.zero_()
    return model


def _car_model(cls):
    torch.manual_seed(0)
    return cls(2, 1, S, 64)


def _threshold_states(n_envs):
    """The preset states of test_device_rollout_continuous_gpu.py: the first
    half runs into the goal, the second half into the left wall."""
    half = n_envs // 2
    i = torch.arange(half, dtype=torch.float32)
    goal = torch.stack([0.30 + 0.14 * i / half, torch.full((half,), 0.04)], 1)
    wall = torch.stack([-1.19 + 0.12 * i / half, torch.full((half,), -0.04)], 1)
    return torch.cat([goal, wall]).contiguous()


def _evaluator(model, env, n_envs, episodes, device):
    return DeviceEvaluator(model.actor.core, env, n_envs, episodes, device,
                           EVAL_SEED, max_episode_steps=MAX_STEPS)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, env, reference evaluator after its one evaluate(), start) on
    the CPU — computed once per case and shared, never modified."""
    preset = None
    if name == "cartpole-h64":
        model, env, n, e = _cartpole_model(64, 30.0), CART, 64, 3
    elif name == "cartpole-h32":
        model, env, n, e = _cartpole_model(32, 10.0), CART, 3, 2
    elif name == "cartpole-h128":
        model, env, n, e = _cartpole_model(128, 10.0), CART, 5, 2
    else:
        kind, starts = name.split("/")
        cls = MlpLSTMSingleContinuous if kind == "car-ppo" else MlpLSTMSeperateContinuous
        model, env, n, e = _car_model(cls), CAR, 64, 2
        if starts == "thresholds":
            preset = _threshold_states(n)
    ref = _evaluator(model, env, n, e, "cpu")
    assert ref.eager
    ref.evaluate(preset)
    return model, env, ref, preset


def _check_parity(name, max_excluded):
    """Kernel vs eager reference, whole episodes.

    One float rounding can flip an arg-max or a termination test, after which
    the trajectories legitimately diverge; so the reference alone computes,
    per env, the smallest margin over all live steps (top-1 minus top-2
    logit, distance of |x| / |theta| from its threshold; for the car the
    distances to the wall, the goal and, past it, zero velocity) and envs
    below MARGIN are excluded. On the kept envs the lengths must be equal;
    CartPole returns (a count) too, MountainCar returns (a float sum of at
    most 40 rewards) within 1e-4 absolute.

    Reference figures measured on the CPU (eval seed 1, model seed 0,
    max_episode_steps 40; ended = terminated + truncated episodes of the
    kept envs, switches = action changes inside an episode):
      cartpole-h64  N=64 E=3: 5 excluded, min margin 1.8e-5, 122 + 55 ended,
                              3966 switches in 59 kept envs
      cartpole-h32  N=3  E=2: 0 excluded, min margin 4.5e-4, 6 + 0 ended,
                              17 switches in 3 envs
      cartpole-h128 N=5  E=2: 0 excluded, min margin 1.0e-3, 10 + 0 ended,
                              45 switches in 5 envs
      car-ppo/random          : 0 excluded, min margin 5.3e-1, 0 + 128 ended
      car-sac/random          : 0 excluded, min margin 5.0e-1, 0 + 128 ended
      car-ppo/thresholds      : 0 excluded, min margin 6.6e-4, 32 + 96 ended
      car-sac/thresholds      : 0 excluded, min margin 4.4e-4, 32 + 96 ended
    """
    model, env, ref, preset = _case(name)
    want = ref.result
    gmodel = copy.deepcopy(model).to(DEV)
    ker = _evaluator(gmodel, env, ref.N, ref.E, DEV)
    assert not ker.eager
    got = ker.evaluate(None if preset is None else preset.to(DEV))
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in got.items()}

    keep = ref.margin >= MARGIN
    terminated = int((want["lengths"][keep] < MAX_STEPS).sum())
    truncated = int((want["lengths"][keep] == MAX_STEPS).sum())
    print(f"{name} N={ref.N} E={ref.E}: min margin {float(ref.margin.min()):.3e}, "
          f"excluded {int((~keep).sum())}, ended {terminated} + {truncated}, "
          f"switches {int(ref.switches[keep].sum())} in "
          f"{int((ref.switches[keep] > 0).sum())} kept envs")
    assert int((~keep).sum()) <= max_excluded
    len_diff = int((got["lengths"][keep] != want["lengths"][keep]).sum())
    ret_err = float((got["returns"][keep] - want["returns"][keep]).abs().max())
    print(f"  lengths differing {len_diff}, returns max abs err {ret_err:.3e}")
    assert torch.equal(got["lengths"][keep], want["lengths"][keep])
    if env == CART:
        assert torch.equal(got["returns"][keep], want["returns"][keep])
    else:
        assert ret_err <= 1e-4
    return ref, keep, terminated, truncated


def test_parity_cartpole_switching_policy():
    ref, keep, terminated, truncated = _check_parity("cartpole-h64", max_excluded=8)
    assert int((ref.switches[keep] > 0).sum()) >= 50
    assert terminated >= 100 and truncated >= 30


@pytest.mark.parametrize("name", ["cartpole-h32", "cartpole-h128"])
def test_parity_small_shapes(name):
    # H=128 keeps only w_hh in registers and streams w_ih: its own code path
    _check_parity(name, max_excluded=0)


@pytest.mark.parametrize("kind", ["car-ppo", "car-sac"])
def test_parity_mountain_car_random_starts(kind):
    ref, keep, terminated, truncated = _check_parity(f"{kind}/random", max_excluded=0)
    assert terminated == 0 and truncated == ref.N * ref.E
    assert float(ref.margin.min()) >= 0.5


@pytest.mark.parametrize("kind", ["car-ppo", "car-sac"])
def test_parity_mountain_car_thresholds(kind):
    """A fresh car reaches neither the goal nor the wall in 40 steps, so
    episode 0 starts from a preset state that runs into them: in the
    reference all 32 goal runners terminate in episode 0."""
    ref, keep, terminated, truncated = _check_parity(f"{kind}/thresholds",
                                                     max_excluded=0)
    goal_runners = ref.result["lengths"][: ref.N // 2, 0]
    assert int((goal_runners < MAX_STEPS).sum()) == ref.N // 2
    assert terminated == ref.N // 2


# --------------------------------------------------------------------------- #
def _gpu_evaluator(n_envs=16, episodes=2):
    model = _cartpole_model(64, 30.0).to(DEV)
    return model, _evaluator(model, CART, n_envs, episodes, DEV)


def test_reads_live_weights():
    model, ev = _gpu_evaluator()
    before = {k: v.clone() for k, v in ev.evaluate().items()}
    assert int((before["lengths"] == MAX_STEPS).sum()) > 0  # some balance
    with torch.no_grad():
        model.actor.core.heads_b[0] += 50.0  # in place, as the optimizer does
    after = ev.evaluate()  # same evaluator: no rebuild
    # always pushing left: the pole falls in every episode
    assert int(after["lengths"].max()) < MAX_STEPS
    assert not torch.equal(after["lengths"], before["lengths"])
    assert torch.equal(after["returns"], after["lengths"].to(torch.float32))


def test_stable_storage_and_repeatable():
    _, ev = _gpu_evaluator()
    first = ev.evaluate()
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    snap = {k: v.clone() for k, v in first.items()}
    for _ in range(3):
        again = ev.evaluate()
        assert all(again[k] is first[k] for k in first)
        assert {k: v.data_ptr() for k, v in again.items()} == ptrs
        assert all(torch.equal(again[k], snap[k]) for k in snap)
    assert first["returns"].is_cuda and first["lengths"].dtype == torch.int32
    s = ev.summary()
    assert s["mean_return"] == pytest.approx(float(snap["returns"].mean()))
    assert s["mean_length"] == pytest.approx(float(snap["lengths"].float().mean()))


def test_kernel_rejects_bad_tensors():
    _, ev = _gpu_evaluator(n_envs=4)
    ev.lengths = ev.lengths[:, :1]  # wrong size, non-contiguous
    with pytest.raises(RuntimeError, match="ep_len"):
        ev.evaluate()
    _, ev = _gpu_evaluator(n_envs=4)
    ev.returns = ev.returns.to(torch.float64)
    with pytest.raises(RuntimeError, match="ep_ret"):
        ev.evaluate()
    _, ev = _gpu_evaluator(n_envs=4)
    with pytest.raises(RuntimeError, match="start_state"):
        ev.evaluate(torch.zeros(4, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="start_state"):
        ev.evaluate(torch.zeros(4, 4))  # on the host
    ev.max_episode_steps = (1 << 22) + 1
    with pytest.raises(RuntimeError, match="step loop bound"):
        ev.evaluate()


def test_eager_flag_runs_reference_on_gpu(monkeypatch):
    monkeypatch.setenv("PDRL_ROLLOUT_EAGER", "1")
    model, ev = _gpu_evaluator(n_envs=4)
    assert ev.eager
    res = ev.evaluate()
    assert res["returns"].is_cuda and ev.margin.is_cuda
    assert torch.equal(res["returns"], res["lengths"].to(torch.float32))
    monkeypatch.delenv("PDRL_ROLLOUT_EAGER")
    ker = _evaluator(model, CART, 4, 2, DEV)
    assert not ker.eager
    keep = ev.margin >= MARGIN
    assert torch.equal(ker.evaluate()["lengths"][keep], res["lengths"][keep])


@pytest.mark.parametrize("algo", ["IMPALA", "SAC-Continuous"])
def test_learner_device_mode_evaluates(params, algo):
    from pdrl_amd.agents import Learner

    p = params
    p.algo = algo
    if algo == "IMPALA":
        p.env, p.obs_dim, p.n_actions, p.continuous = CART, 4, 2, False
        lo, hi, max_len = 1.0, 500.0, 500
    else:
        p.env, p.obs_dim, p.n_actions, p.continuous = CAR, 2, 1, True
        lo, hi, max_len = -99.9, 100.0, 999
    p.batch_size, p.seq_len = 32, 5
    p.model_save_interval = 10_000
    p.actor_mode = "device"
    p.eval_interval = 5
    lrn = Learner(None, "127.0.0.1", 0, p, device=DEV)
    seen = []
    try:
        assert not lrn.device_rollout.eager and not lrn.evaluator.eager
        assert (lrn.evaluator.N, lrn.evaluator.E) == (p.eval_envs, p.eval_episodes)
        maybe = lrn.maybe_evaluate
        lrn.maybe_evaluate = lambda: (maybe(), seen.append(lrn.last_eval))
        lrn.run(max_updates=10)
        torch.cuda.synchronize()
        assert lrn.updater.update_count == 10
        assert [s and s["update"] for s in seen] == [None] * 4 + [5] * 5 + [10]
        last = lrn.last_eval
        assert all(math.isfinite(v) for v in last.values()), last
        assert lo <= last["min_return"] <= last["mean_return"] <= last["max_return"] <= hi
        assert 1.0 <= last["mean_length"] <= max_len
        # evaluation consumed no training ticks
        assert int(lrn.device_rollout.tick[0]) == 10 * p.seq_len
    finally:
        lrn.close()
