"""Device envs whose observation is not their state, CPU side: the fp32
oracles of Acrobot-v1 and Pendulum-v1 against the native float64 envs, the
obs / state split of ``DeviceRollout`` and ``DeviceEvaluator`` on the eager
path, and the identity default of the existing envs."""
import math

import numpy as np
import pytest
import torch

from pdrl_amd.envs.acrobot import AcrobotEnv
from pdrl_amd.envs.pendulum import PendulumEnv
from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.networks.models import (MlpLSTMSeperateContinuous,
                                      MlpLSTMSingleContinuous)
from pdrl_amd.ops.evaluate import DeviceEvaluator
from pdrl_amd.ops.rollout import (DEVICE_ENVS, AcrobotDyn, CartPoleDyn,
                                  DeviceRollout, MountainCarContDyn,
                                  PendulumDyn, has_device_env,
                                  is_continuous_env, uniform, wrap_angle)
from tests.test_device_rollout_gpu import STATE, check_split_launches

ACRO, PEN = "Acrobot-v1", "Pendulum-v1"
S = 5


def test_registry_and_shapes():
    assert DEVICE_ENVS[ACRO] is AcrobotDyn and DEVICE_ENVS[PEN] is PendulumDyn
    assert has_device_env(ACRO) and has_device_env(PEN)
    assert not is_continuous_env(ACRO) and is_continuous_env(PEN)
    assert (AcrobotDyn.env_id, AcrobotDyn.obs_dim, AcrobotDyn.state_dim,
            AcrobotDyn.n_actions, AcrobotDyn.reset_draws,
            AcrobotDyn.max_episode_steps) == (2, 6, 4, 3, 4, 500)
    assert (PendulumDyn.env_id, PendulumDyn.obs_dim, PendulumDyn.state_dim,
            PendulumDyn.act_dim, PendulumDyn.reset_draws,
            PendulumDyn.max_episode_steps) == (3, 3, 2, 1, 2, 200)


@pytest.mark.parametrize("dyn", [CartPoleDyn, MountainCarContDyn])
def test_existing_envs_observe_their_state(dyn):
    assert dyn.state_dim == dyn.obs_dim
    state = torch.randn(5, dyn.state_dim)
    assert dyn.observe(state) is state


def test_wrap_angle_fp32():
    x = torch.tensor([0.0, 3.0, -3.0, 3.5, -3.5, 10.0, -10.0])
    w = wrap_angle(x)
    assert w.dtype == torch.float32
    assert float(w.min()) >= -3.1415927 - 1e-6 and float(w.max()) < 3.1415927
    k = (x - w) / (2 * math.pi)
    torch.testing.assert_close(k, k.round(), atol=1e-6, rtol=0)


# --------------------------------------------------------------------------- #
# fp32 oracle against the native float64 env: 256 random states, one step
# --------------------------------------------------------------------------- #
def test_acrobot_oracle_matches_native_env():
    rng = np.random.default_rng(0)
    states = np.stack([rng.uniform(-math.pi, math.pi, 256),
                       rng.uniform(-math.pi, math.pi, 256),
                       rng.uniform(-4.0, 4.0, 256),
                       rng.uniform(-9.0, 9.0, 256)], 1).astype(np.float32)
    acts = rng.integers(0, 3, 256)
    want_obs, want_rew, want_term, height = [], [], [], []
    for s, a in zip(states, acts):
        env = AcrobotEnv()
        env.reset()
        env._state = s.astype(np.float64)
        obs, rew, term, _, _ = env.step(int(a))
        want_obs.append(obs)
        want_rew.append(rew)
        want_term.append(term)
        t1, t2 = env._state[:2]
        height.append(-math.cos(t1) - math.cos(t1 + t2))
    st = torch.tensor(states)
    nxt, rew, term = AcrobotDyn.step(st, torch.tensor(acts))
    obs = AcrobotDyn.observe(nxt)
    assert nxt.dtype == obs.dtype == rew.dtype == torch.float32
    assert nxt.shape == (256, 4) and obs.shape == (256, 6)
    np.testing.assert_allclose(obs.numpy(), np.stack(want_obs), atol=1e-5, rtol=0)
    clear = np.abs(np.array(height) - 1.0) > 1e-4
    assert clear.sum() >= 250
    assert (term.numpy() == np.array(want_term))[clear].all()
    np.testing.assert_allclose(rew.numpy()[clear], np.array(want_rew)[clear],
                               atol=1e-5, rtol=0)
    assert any(want_term) and not all(want_term)
    # the margin is the tip height's distance from 1
    np.testing.assert_allclose(AcrobotDyn.threshold_margin(nxt).numpy(),
                               np.abs(np.array(height) - 1.0), atol=1e-5)
    # the observation of the pre-step state, too
    np.testing.assert_allclose(
        AcrobotDyn.observe(st).numpy(),
        np.stack([np.cos(states[:, 0]), np.sin(states[:, 0]),
                  np.cos(states[:, 1]), np.sin(states[:, 1]),
                  states[:, 2], states[:, 3]], 1), atol=1e-6)


def test_pendulum_oracle_matches_native_env():
    rng = np.random.default_rng(1)
    states = np.stack([rng.uniform(-3 * math.pi, 3 * math.pi, 256),
                       rng.uniform(-8.0, 8.0, 256)], 1).astype(np.float32)
    acts = rng.uniform(-1.5, 1.5, 256).astype(np.float32)
    want_obs, want_rew = [], []
    for s, a in zip(states, acts):
        env = PendulumEnv()
        env.reset()
        env._state = s.astype(np.float64)
        obs, rew, term, _, _ = env.step([float(a)])
        assert not term
        want_obs.append(obs)
        want_rew.append(rew)
    nxt, rew, term = PendulumDyn.step(torch.tensor(states), torch.tensor(acts))
    obs = PendulumDyn.observe(nxt)
    assert nxt.shape == (256, 2) and obs.shape == (256, 3)
    assert obs.dtype == rew.dtype == torch.float32 and term.dtype == torch.bool
    assert not term.any()
    np.testing.assert_allclose(obs.numpy(), np.stack(want_obs), atol=1e-5, rtol=0)
    # the reward reaches -16.3: relative
    np.testing.assert_allclose(rew.numpy(), np.array(want_rew), atol=0, rtol=1e-5)
    assert float(rew.min()) < -12.0
    assert (np.abs(nxt.numpy()[:, 1]) == 8.0).any()  # the speed clip acted
    margin = PendulumDyn.threshold_margin(torch.tensor(states), torch.tensor(acts))
    assert bool(torch.isinf(margin).all())


def test_fixed_points():
    nxt, rew, term = AcrobotDyn.step(torch.zeros(2, 4), torch.ones(2, dtype=torch.int64))
    assert torch.count_nonzero(nxt) == 0
    assert rew.tolist() == [-1.0, -1.0] and not term.any()
    nxt, rew, term = PendulumDyn.step(torch.zeros(2, 2), torch.zeros(2))
    assert torch.count_nonzero(nxt) == 0
    assert rew.tolist() == [0.0, 0.0] and not term.any()


def test_resets_cover_the_published_ranges():
    u = torch.stack([uniform(1, torch.arange(4096), 0, k) for k in range(1, 5)], 1)
    s = AcrobotDyn.reset(u)
    assert s.shape == (4096, 4)
    assert float(s.min()) >= -0.1 and float(s.max()) < 0.1
    assert float(s.min()) < -0.099 and float(s.max()) > 0.099
    s = PendulumDyn.reset(u[:, :2])
    assert s.shape == (4096, 2)
    assert -3.1415927 <= float(s[:, 0].min()) < -3.13
    assert 3.13 < float(s[:, 0].max()) < 3.1415927
    assert -1.0 <= float(s[:, 1].min()) < -0.99 and 0.99 < float(s[:, 1].max()) < 1.0


# --------------------------------------------------------------------------- #
# DeviceRollout / DeviceEvaluator on the CPU
# --------------------------------------------------------------------------- #
def _acrobot_core(hidden=64):
    torch.manual_seed(0)
    return MlpLSTMSingle(6, 3, S, hidden).actor.core


def _pendulum_core(mode, hidden=64):
    torch.manual_seed(0)
    cls = MlpLSTMSingleContinuous if mode == 0 else MlpLSTMSeperateContinuous
    return cls(3, 1, S, hidden).actor.core


def _cases():
    return [(ACRO, AcrobotDyn, _acrobot_core(), {}),
            (PEN, PendulumDyn, _pendulum_core(0), {}),
            (PEN, PendulumDyn, _pendulum_core(1), dict(ou_envs=2))]


@pytest.mark.parametrize("case", range(3))
def test_rollout_records_the_observation_of_the_state(case):
    env, dyn, core, kw = _cases()[case]
    N = 8
    ro = DeviceRollout(core, env, N, S, "cpu", 3, time_horizon=500,
                       max_episode_steps=7, **kw)
    assert ro.eager and ro.env_state.shape == (N, dyn.state_dim)
    assert ro.fields["obs"] == dyn.obs_dim
    # the first state is the reset of tick 0
    assert torch.equal(ro.env_state, dyn.reset(ro._reset_uniforms(0)))
    for call in range(4):
        before = ro.env_state.clone()
        b = ro.rollout()
        assert b["obs"].shape == (N, S, dyn.obs_dim)
        assert ro.env_state.shape == (N, dyn.state_dim)
        # replay the dynamics from the recorded actions: obs[:, t] is the
        # observation of the state before step t
        state = before
        for t in range(S):
            assert torch.equal(b["obs"][:, t], dyn.observe(state)), (call, t)
            act = b["act"][:, t, 0]
            nxt, rew, term = dyn.step(
                state, act if ro.continuous else act.to(torch.int64))
            assert torch.equal(b["rew"][:, t, 0], rew)
            tick = call * S + t + 1
            fresh = dyn.reset(ro._reset_uniforms(tick))
            reset = term | torch.tensor([tick % 7 == 0] * N)
            if t + 1 < S:
                assert torch.equal(b["is_fir"][:, t + 1, 0], reset.float())
            state = torch.where(reset[:, None], fresh, nxt)
        assert torch.equal(ro.env_state, state)
    games, mean50 = ro.episode_stats()
    assert games >= 2 * N and mean50 < 0.0


def test_acrobot_samples_all_three_actions():
    ro = DeviceRollout(_acrobot_core(), ACRO, 64, S, "cpu", 3, time_horizon=500)
    acts = torch.cat([ro.rollout()["act"].clone() for _ in range(4)], 1)
    counts = torch.bincount(acts.flatten().to(torch.int64), minlength=3)
    assert counts.shape == (3,) and int(counts.min()) >= 300
    assert bool(torch.isfinite(ro.margin).all()) and float(ro.margin.min()) >= 0


def test_pendulum_margin_is_infinite():
    ro = DeviceRollout(_pendulum_core(1), PEN, 8, S, "cpu", 3, time_horizon=500)
    ro.rollout()
    assert bool(torch.isinf(ro.margin).all())


@pytest.mark.parametrize("case", range(3))
def test_split_launches_equal_one_launch(case):
    env, _, core, kw = _cases()[case]
    state = STATE + (("ou_state",) if kw else ())
    check_split_launches(
        lambda seq_len: DeviceRollout(core, env, 3, seq_len, "cpu", 1,
                                      time_horizon=500, max_episode_steps=7,
                                      **kw),
        min_episodes=6, state=state)


def test_evaluator_uses_the_state_vector():
    ev = DeviceEvaluator(_acrobot_core(), ACRO, 4, 2, "cpu", seed=5,
                         max_episode_steps=12)
    assert ev.start_states(0).shape == (4, 4)
    assert torch.equal(ev.start_states(1), AcrobotDyn.reset(ev._reset_uniforms(1)))
    with pytest.raises(ValueError, match=r"start_state must be \(4, 4\)"):
        ev.evaluate(torch.zeros(4, 6))  # (N, obs_dim) is not the state
    # hanging at rest never swings up: both episodes run to the limit
    res = ev.evaluate(ev.start_states(0))
    assert res["lengths"].tolist() == [[12, 12]] * 4
    assert res["returns"].tolist() == [[-12.0, -12.0]] * 4
    assert torch.equal(ev.evaluate()["returns"], res["returns"])
    # a state that is about to swing over the bar terminates early, reward 0
    # on the last step; the second episode starts from the hash reset again
    up = torch.tensor([[2.0, 0.0, 2.5, 1.0]]).expand(4, 4).contiguous()
    res = ev.evaluate(up)
    assert int(res["lengths"][:, 0].max()) < 12
    assert torch.equal(res["returns"][:, 0], 1.0 - res["lengths"][:, 0].float())
    assert res["lengths"][:, 1].tolist() == [12] * 4

    pe = DeviceEvaluator(_pendulum_core(1), PEN, 4, 2, "cpu", seed=5,
                         max_episode_steps=9)
    assert pe.start_states(0).shape == (4, 2)
    with pytest.raises(ValueError, match=r"start_state must be \(4, 2\)"):
        pe.evaluate(torch.zeros(4, 3))
    res = pe.evaluate()
    assert res["lengths"].tolist() == [[9, 9]] * 4
    assert bool((res["returns"] < 0).all())
    assert bool(torch.isinf(pe.margin).all())


# --------------------------------------------------------------------------- #
# learner integration
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("algo,env,dims,continuous", [
    ("PPO", ACRO, (6, 3), False),
    ("PPO-Continuous", PEN, (3, 1), True),
])
def test_learner_device_mode(params, algo, env, dims, continuous):
    from pdrl_amd.agents import Learner

    p = params
    p.algo, p.env, p.continuous = algo, env, continuous
    p.obs_dim, p.n_actions = dims
    p.actor_mode = "device"
    p.eval_interval, p.eval_envs = 2, 4
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        ro = lrn.device_rollout
        assert ro.env_state.shape == (p.batch_size, DEVICE_ENVS[env].state_dim)
        lrn.run(max_updates=2)
        assert lrn.updater.update_count == 2
        assert int(ro.tick[0]) == 2 * p.seq_len
        assert lrn.last_eval["update"] == 2
        assert math.isfinite(lrn.last_eval["mean_return"])
        assert lrn.last_eval["mean_return"] < 0.0
    finally:
        lrn.close()


def test_learner_device_mode_keeps_the_policy_kind_errors(params):
    from pdrl_amd.agents import Learner

    p = params
    p.algo, p.env, p.continuous = "PPO", PEN, False
    p.obs_dim, p.n_actions = 3, 3
    p.actor_mode = "device"
    with pytest.raises(ValueError, match="continuous policies only"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")
    p.algo, p.env, p.continuous = "PPO-Continuous", ACRO, True
    p.obs_dim, p.n_actions = 6, 1
    with pytest.raises(ValueError, match="discrete policies only"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")
