"""Device actor mode for continuous control, CPU side: the fp32 reference
dynamics of MountainCarContinuous-v0, the hash normal, the two Gaussian
sampling schemes and OU exploration of the eager reference path (which is
also the GPU kernel's oracle), and the learner integration."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdrl_amd.envs.mountain_car import MountainCarContinuousEnv
from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.networks.models import (MlpLSTMSeperateContinuous,
                                      MlpLSTMSingleContinuous)
from pdrl_amd.ops.rollout import (DEVICE_ENVS, DeviceRollout,
                                  MountainCarContDyn, normal, uniform)

ENV = "MountainCarContinuous-v0"
HALF_LOG_2PI = 0.9189385


# --------------------------------------------------------------------------- #
# dynamics
# --------------------------------------------------------------------------- #
def test_mountain_car_dynamics_match_env():
    assert DEVICE_ENVS[ENV] is MountainCarContDyn
    assert (MountainCarContDyn.env_id, MountainCarContDyn.obs_dim,
            MountainCarContDyn.act_dim, MountainCarContDyn.max_episode_steps) \
        == (1, 2, 1, 999)
    rng = np.random.default_rng(0)
    # states over the live region and a little past the wall and the goal
    pos = rng.uniform(-1.25, 0.62, size=64)
    vel = rng.uniform(-0.07, 0.07, size=64)
    act = rng.uniform(-1.5, 1.5, size=64)
    states = np.stack([pos, vel], 1).astype(np.float32)
    act = act.astype(np.float32)
    ref_next, ref_rew, ref_term = [], [], []
    for s, a in zip(states, act):
        env = MountainCarContinuousEnv()
        env.reset()
        env._state = s.astype(np.float64)
        nxt, rew, term, _, _ = env.step([float(a)])
        ref_next.append(nxt)
        ref_rew.append(rew)
        ref_term.append(term)
    nxt, rew, term = MountainCarContDyn.step(torch.tensor(states), torch.tensor(act))
    assert nxt.dtype == torch.float32 and rew.dtype == torch.float32
    np.testing.assert_allclose(nxt.numpy(), np.stack(ref_next), atol=1e-6, rtol=0)
    np.testing.assert_allclose(rew.numpy(), np.array(ref_rew), atol=1e-5, rtol=0)
    assert term.tolist() == ref_term
    assert any(ref_term) and not all(ref_term)


def test_threshold_margin_is_smallest_of_three_distances():
    # (pos, vel, action) -> expected margin, worked by hand from the update
    st = torch.tensor([[0.2, 0.0], [0.44, 0.02], [-1.19, -0.05]])
    a = torch.zeros(3)
    _, raw, pos, vel = MountainCarContDyn._advance(st, a)
    m = MountainCarContDyn.threshold_margin(st, a)
    # mid-valley: nearest is the goal; past the goal: |vel| counts; at the
    # wall: the unclamped position's distance from -1.2
    assert float(m[0]) == pytest.approx(float((pos[0] - 0.45).abs()))
    assert float(pos[1]) >= 0.45
    assert float(m[1]) == pytest.approx(min(float(pos[1] - 0.45), float(vel[1].abs())))
    assert float(raw[2]) < -1.2
    assert float(m[2]) == pytest.approx(float((raw[2] + 1.2).abs()))


# --------------------------------------------------------------------------- #
# normal draw
# --------------------------------------------------------------------------- #
def test_normal_matches_float64_formula():
    two_pi = float(np.float32(6.2831855))
    for seed, env, tick in [(1, 0, 1), (1, 5, 7), (1234, 63, 40)]:
        u5 = float(uniform(seed, torch.tensor([env]), tick, 5)[0])
        u6 = float(uniform(seed, torch.tensor([env]), tick, 6)[0])
        want = math.sqrt(-2.0 * math.log(1.0 - u5)) * math.cos(two_pi * u6)
        got = normal(seed, torch.tensor([env]), tick)
        assert got.dtype == torch.float32
        assert abs(float(got[0]) - want) < 1e-6
    # tensor ticks give the same stream as int ticks
    assert torch.equal(normal(1, torch.tensor([5]), torch.tensor([7])),
                       normal(1, torch.tensor([5]), 7))


def test_normal_moments():
    n = normal(7, torch.arange(100_000), 3)
    assert bool(torch.isfinite(n).all())
    assert abs(float(n.mean())) < 0.01
    assert abs(float(n.std()) - 1.0) < 0.01


# --------------------------------------------------------------------------- #
# rollout semantics (eager reference)
# --------------------------------------------------------------------------- #
N, S, CALLS, MAX_STEPS = 8, 5, 6, 7
T = S * CALLS


def _core(mode, hidden=64, n_outputs=1):
    torch.manual_seed(0)
    if mode == 0:
        return MlpLSTMSingleContinuous(2, n_outputs, S, hidden).actor.core
    return MlpLSTMSeperateContinuous(2, n_outputs, S, hidden).actor.core


def _run(mode, seed=1, max_steps=None, calls=CALLS, **kw):
    core = _core(mode)
    ro = DeviceRollout(core, ENV, N, S, "cpu", seed, time_horizon=500,
                       max_episode_steps=max_steps, **kw)
    chunks, objs = [], []
    for _ in range(calls):
        b = ro.rollout()
        objs.append({k: id(v) for k, v in b.items()})
        chunks.append({k: v.clone() for k, v in b.items()})
    cat = {k: torch.cat([c[k] for c in chunks], dim=1) for k in chunks[0]}
    return core, ro, cat, objs


@pytest.fixture(scope="module")
def runs():
    """Mode -> (core, rollout, 30 ticks) of a fresh start; computed once."""
    return {mode: _run(mode) for mode in (0, 1)}


@pytest.fixture(scope="module")
def truncated():
    return {mode: _run(mode, max_steps=MAX_STEPS) for mode in (0, 1)}


@pytest.mark.parametrize("mode", [0, 1])
def test_fields_and_stable_tensors(runs, mode):
    from pdrl_amd.buffers import rollout_fields

    _, ro, cat, objs = runs[mode]
    fields = rollout_fields(2, 1, 64, True)
    assert fields["logits"] == 2 and fields["act"] == 1
    assert list(cat) == list(fields) and ro.fields == fields
    for k, d in fields.items():
        assert cat[k].shape == (N, T, d) and cat[k].dtype == torch.float32
    assert all(o == objs[0] for o in objs)  # same tensor objects every call
    assert ro.mode == mode and ro.continuous


def test_mode0_log_prob_is_normal_density(runs):
    core, _, cat, _ = runs[0]
    assert core.head_names[:2] == ["mu", "std"]
    mu, std = cat["logits"][..., 0:1], cat["logits"][..., 1:2]
    dist = torch.distributions.Normal(torch.tanh(mu), F.softplus(std) + 1e-4)
    torch.testing.assert_close(cat["log_prob"], dist.log_prob(cat["act"]),
                               atol=1e-4, rtol=0)
    # act = mean + sd * n on the hash normal; stored unclipped
    n = torch.stack([normal(1, torch.arange(N), t + 1) for t in range(T)], 1)
    want = torch.tanh(mu[..., 0]) + (F.softplus(std[..., 0]) + 1e-4) * n
    torch.testing.assert_close(cat["act"][..., 0], want, atol=1e-6, rtol=0)


def test_mode1_log_prob_is_tanh_gaussian_density(runs):
    core, _, cat, _ = runs[1]
    assert core.head_names[:2] == ["mu", "log_std"]
    act = cat["act"]
    assert float(act.abs().max()) <= 1.0
    mu = cat["logits"][..., 0:1]
    ls = cat["logits"][..., 1:2].clamp(-20.0, 2.0)
    inner = act.abs() < 0.99
    assert bool(inner.any())
    # atanh is ill-conditioned towards |act| = 1: hence the looser bound
    z = torch.atanh(act.double())
    want = (torch.distributions.Normal(mu.double(), ls.double().exp()).log_prob(z)
            - torch.log(1.0 - act.double() ** 2 + 1e-7))
    assert float((cat["log_prob"].double() - want)[inner].abs().max()) <= 1e-3


# --------------------------------------------------------------------------- #
# OU exploration
# --------------------------------------------------------------------------- #
def _ou_actions(max_steps, theta=0.15, sigma=0.6):
    """tanh of the OU recursion on the hash normals, zeroed after a reset."""
    envs = torch.arange(N // 2)
    ou, out = torch.zeros(N // 2), []
    for t in range(T):
        n = normal(1, envs, t + 1)
        ou = ou - theta * ou + sigma * n
        out.append(torch.tanh(ou))
        if max_steps and (t + 1) % max_steps == 0:
            ou = torch.zeros_like(ou)
    return torch.stack(out, 1)


@pytest.mark.parametrize("max_steps", [None, MAX_STEPS])
def test_ou_explorers_follow_the_recursion(runs, truncated, max_steps):
    _, ro, cat, _ = _run(1, max_steps=max_steps, ou_envs=N // 2)
    half = N // 2
    assert torch.equal(cat["act"][:half, :, 0], _ou_actions(max_steps))
    # the other envs sample from the policy, exactly as without explorers
    plain = (truncated if max_steps else runs)[1][2]
    for k in cat:
        assert torch.equal(cat[k][half:], plain[k][half:]), k
    assert not torch.equal(cat["act"][:half], plain["act"][:half])
    # log-prob: the policy's density at the OU action
    mu = cat["logits"][:half, :, 0]
    ls = cat["logits"][:half, :, 1].clamp(-20.0, 2.0)
    a = cat["act"][:half, :, 0]
    keep = a.abs() < 0.99
    z = torch.atanh(a.double())
    want = (-0.5 * ((z - mu.double()) / ls.double().exp()) ** 2 - ls.double()
            - HALF_LOG_2PI - torch.log(1.0 - a.double() ** 2 + 1e-7))
    assert float((cat["log_prob"][:half, :, 0].double() - want)[keep].abs().max()) <= 1e-3
    assert bool((ro.ou_state[half:] == 0).all())
    assert bool((ro.ou_state[:half] != 0).all())


def test_ou_state_is_zero_after_every_reset():
    core = _core(1)
    ro = DeviceRollout(core, ENV, N, MAX_STEPS, "cpu", 1, time_horizon=500,
                       max_episode_steps=MAX_STEPS, ou_envs=N // 2,
                       warmup_steps=3)
    for _ in range(3):  # every call ends on a truncation
        ro.rollout()
        assert bool((ro.is_fir == 1).all())
        assert torch.count_nonzero(ro.ou_state) == 0
    # warm-up: every env explores while tick <= 3 (first call only)
    ro2 = DeviceRollout(core, ENV, N, MAX_STEPS, "cpu", 1, time_horizon=500,
                        max_episode_steps=MAX_STEPS, warmup_steps=3)
    first = ro2.rollout()["act"][:, :, 0].clone()
    envs, ou = torch.arange(N), torch.zeros(N)
    for t in range(3):
        ou = ou - 0.15 * ou + 0.6 * normal(1, envs, t + 1)
        assert torch.equal(first[:, t], torch.tanh(ou))
    plain = DeviceRollout(core, ENV, N, MAX_STEPS, "cpu", 1, time_horizon=500,
                          max_episode_steps=MAX_STEPS).rollout()["act"][:, :, 0]
    assert not torch.equal(first[:, :3], plain[:, :3])


def test_ou_with_on_policy_core_raises():
    with pytest.raises(ValueError, match="OU exploration"):
        DeviceRollout(_core(0), ENV, N, S, "cpu", 1, 500, ou_envs=2)
    with pytest.raises(ValueError, match="OU exploration"):
        DeviceRollout(_core(0), ENV, N, S, "cpu", 1, 500, warmup_steps=10)


# --------------------------------------------------------------------------- #
# reset, truncation, horizon, stats
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("mode", [0, 1])
def test_reset_semantics(truncated, mode):
    core, ro, cat, _ = truncated[mode]
    # the car cannot reach the goal within 7 steps of a valley start, so every
    # episode is truncated at exactly MAX_STEPS: resets after ticks 7, 14, ...
    fir = cat["is_fir"][:, :, 0]
    expect = torch.tensor([1.0 if t % MAX_STEPS == 0 else 0.0 for t in range(T)])
    assert torch.equal(fir, expect.expand(N, T))
    first = fir.bool()
    assert torch.count_nonzero(cat["hx"][first]) == 0
    assert torch.count_nonzero(cat["cx"][first]) == 0
    start = cat["obs"][first]
    assert float(start[:, 0].min()) >= -0.6 and float(start[:, 0].max()) < -0.4
    assert torch.count_nonzero(start[:, 1]) == 0
    envs = torch.arange(N)
    for t in range(0, T, MAX_STEPS):  # hash lane 1 of the tick that reset
        assert torch.equal(cat["obs"][:, t, 0], -0.6 + 0.2 * uniform(1, envs, t, 1))
    # carried env and recurrent state between resets; rewards of the dynamics
    with torch.no_grad():
        for t in range(T - 1):
            nxt, rew, term = MountainCarContDyn.step(cat["obs"][:, t], cat["act"][:, t, 0])
            assert not term.any()
            assert torch.equal(cat["rew"][:, t, 0], rew)
            if (t + 1) % MAX_STEPS != 0:
                assert torch.equal(cat["obs"][:, t + 1], nxt)
                _, h, c = core._forward_eager(
                    cat["obs"][:, t : t + 1], cat["hx"][:, t], cat["cx"][:, t])
                torch.testing.assert_close(cat["hx"][:, t + 1], h, atol=1e-6, rtol=0)
                torch.testing.assert_close(cat["cx"][:, t + 1], c, atol=1e-6, rtol=0)
    games, mean50 = ro.episode_stats()
    assert games == N * (T // MAX_STEPS)
    assert -0.1 * MAX_STEPS <= mean50 < 0.0  # returns are negative here
    assert ro.episode_stats() == (games, mean50)


def test_time_horizon_resets_without_done():
    ro = DeviceRollout(_core(1, hidden=32), ENV, 3, S, "cpu", 5, time_horizon=3)
    fir = torch.cat([ro.rollout()["is_fir"].clone() for _ in range(2)], 1)[:, :, 0]
    expect = torch.tensor([1.0 if t % 3 == 0 else 0.0 for t in range(2 * S)])
    assert torch.equal(fir, expect.expand(3, 2 * S))
    assert ro.episode_stats()[0] == 3 * 3


@pytest.mark.parametrize("mode", [0, 1])
def test_seed_reproduces_and_differs(runs, mode):
    cat = runs[mode][2]
    again = _run(mode, seed=1)[2]
    for k in cat:
        assert torch.equal(cat[k], again[k]), k
    other = _run(mode, seed=2)[2]
    assert not torch.equal(cat["obs"], other["obs"])
    assert not torch.equal(cat["act"], other["act"])


def test_rejects_unsupported_configurations():
    with pytest.raises(ValueError, match="Gaussian policy"):
        DeviceRollout(MlpLSTMSingle(2, 3, S, 64).actor.core, ENV, 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="does not match"):
        DeviceRollout(_core(0, n_outputs=2), ENV, 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="does not match"):
        DeviceRollout(_core(1, n_outputs=2), ENV, 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="hidden size"):
        DeviceRollout(_core(1, hidden=48), ENV, 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="first head"):  # Gaussian core, discrete env
        DeviceRollout(_core(0), "CartPole-v1", 4, S, "cpu", 0, 500)


# --------------------------------------------------------------------------- #
# learner integration
# --------------------------------------------------------------------------- #
def _device_params(params, algo):
    params.algo = algo
    params.env = ENV
    params.obs_dim, params.n_actions, params.continuous = 2, 1, True
    params.actor_mode = "device"
    return params


def test_learner_device_mode_ppo_continuous(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params, "PPO-Continuous")
    p.explore_ou_envs = 2  # ignored: on-policy
    seen = []
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        assert lrn.pub is None  # no weight plane in device mode
        assert lrn.device_replay is None  # trains on the rollout in place
        assert lrn.device_rollout.mode == 0 and lrn.device_rollout.ou_envs == 0
        step = lrn.updater.step
        lrn.updater.step = lambda b: seen.append(step(b)) or seen[-1]
        lrn.run(max_updates=3)
        assert lrn.updater.update_count == 3 and len(seen) == 3
        for stats in seen:
            assert all(math.isfinite(float(v)) for v in stats.values())
        assert lrn.device_rollout.N == p.batch_size
        assert int(lrn.device_rollout.tick[0]) == 3 * p.seq_len
    finally:
        lrn.close()


def test_learner_device_mode_sac_continuous_uses_replay_and_ou(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params, "SAC-Continuous")
    p.device_envs = 4  # fewer envs than the batch: replay warm-up path
    p.explore_ou_envs = 2
    p.explore_ou_theta, p.explore_ou_sigma = 0.2, 0.5
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        ro = lrn.device_rollout
        assert (ro.mode, ro.ou_envs, ro.warmup_steps) == (1, 2, 0)
        assert (ro.ou_theta, ro.ou_sigma) == (0.2, 0.5)
        lrn.run(max_updates=2)
        assert lrn.updater.update_count == 2
        assert lrn.device_replay.size >= p.batch_size
        assert bool((ro.ou_state[:2] != 0).all()) and bool((ro.ou_state[2:] == 0).all())
    finally:
        lrn.close()


def test_learner_device_mode_rejects_discrete_algo(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params, "PPO")
    p.continuous, p.n_actions = False, 3
    with pytest.raises(ValueError, match="continuous policies only"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")
