"""Native Pendulum-v1 and Acrobot-v1 physics (float64, published Gymnasium
dynamics; Pendulum with the normalised action)."""
import math

import numpy as np
import pytest

from pdrl_amd import envs
from pdrl_amd.envs.acrobot import AcrobotEnv
from pdrl_amd.envs.pendulum import PendulumEnv, wrap_angle


def test_registered_with_spaces():
    pen = envs.make("Pendulum-v1")
    assert isinstance(pen, PendulumEnv)
    assert isinstance(pen.observation_space, envs.Box)
    assert pen.observation_space.shape == (3,)
    assert isinstance(pen.action_space, envs.Box)
    assert pen.action_space.low.tolist() == [-1.0]
    assert pen.action_space.high.tolist() == [1.0]
    acro = envs.make("Acrobot-v1")
    assert isinstance(acro, AcrobotEnv)
    assert acro.observation_space.shape == (6,)
    assert isinstance(acro.action_space, envs.Discrete)
    assert acro.action_space.n == 3
    assert (PendulumEnv.MAX_EPISODE_STEPS, AcrobotEnv.MAX_EPISODE_STEPS) == (200, 500)


def test_wrap_angle():
    assert wrap_angle(0.0) == 0.0
    assert wrap_angle(math.pi) == pytest.approx(-math.pi)
    assert wrap_angle(-math.pi) == pytest.approx(-math.pi)
    assert wrap_angle(3 * math.pi + 0.25) == pytest.approx(-math.pi + 0.25)
    assert wrap_angle(-7.0) == pytest.approx(-7.0 + 2 * math.pi)


# --------------------------------------------------------------------------- #
# Pendulum
# --------------------------------------------------------------------------- #
def test_pendulum_reset_distribution_and_obs():
    env = PendulumEnv(seed=0)
    thetas, speeds = [], []
    for _ in range(200):
        obs, info = env.reset()
        theta, theta_dot = env._state
        thetas.append(theta)
        speeds.append(theta_dot)
        assert obs.dtype == np.float32 and obs.shape == (3,) and info == {}
        np.testing.assert_allclose(
            obs, [math.cos(theta), math.sin(theta), theta_dot], atol=1e-6)
    assert -math.pi <= min(thetas) < -2.5 and 2.5 < max(thetas) < math.pi
    assert -1.0 <= min(speeds) < -0.8 and 0.8 < max(speeds) < 1.0


def test_pendulum_upright_is_a_fixed_point():
    env = PendulumEnv(seed=0)
    env.reset()
    env._state = np.zeros(2)
    for _ in range(3):
        obs, reward, terminated, truncated, _ = env.step([0.0])
        assert env._state.tolist() == [0.0, 0.0]
        assert obs.tolist() == [1.0, 0.0, 0.0]
        assert reward == 0.0 and not terminated and not truncated


def test_pendulum_step_formulas():
    env = PendulumEnv(seed=0)
    env.reset()
    theta, theta_dot, a = 2.5, -1.5, 0.4
    env._state = np.array([theta, theta_dot])
    obs, reward, terminated, _, _ = env.step([a])
    u = 2.0 * a
    want_dot = theta_dot + (15.0 * math.sin(theta) + 3.0 * u) * 0.05
    want_theta = theta + want_dot * 0.05
    assert env._state[1] == pytest.approx(want_dot, abs=1e-12)
    assert env._state[0] == pytest.approx(want_theta, abs=1e-12)
    # cost on the pre-step state
    assert reward == pytest.approx(
        -(theta**2 + 0.1 * theta_dot**2 + 0.001 * u**2), abs=1e-12)
    assert not terminated
    np.testing.assert_allclose(
        obs, [math.cos(want_theta), math.sin(want_theta), want_dot], atol=1e-6)


def test_pendulum_theta_is_not_wrapped_but_the_cost_is():
    env = PendulumEnv(seed=0)
    env.reset()
    env._state = np.array([3.1, 8.0])
    _, reward, _, _, _ = env.step([1.0])
    assert env._state[0] > math.pi  # carried unwrapped
    assert env._state[1] == 8.0  # clipped at the max speed
    before = env._state.copy()
    _, reward, _, _, _ = env.step([0.0])
    assert reward == pytest.approx(
        -((before[0] - 2 * math.pi) ** 2 + 0.1 * 64.0), abs=1e-9)


def test_pendulum_clips_actions_to_unit_range():
    def after(a):
        env = PendulumEnv(seed=0)
        env.reset()
        env._state = np.array([0.3, 0.2])
        _, reward, _, _, _ = env.step([a])
        return env._state.copy(), reward

    for outside, edge in ((5.0, 1.0), (-3.0, -1.0)):
        (s_out, r_out), (s_edge, r_edge) = after(outside), after(edge)
        assert s_out.tolist() == s_edge.tolist() and r_out == r_edge
    # the largest cost: |wrap θ| = π, |θ̇| = 8, |u| = 2
    env = PendulumEnv(seed=0)
    env.reset()
    env._state = np.array([-math.pi, 8.0])
    _, reward, _, _, _ = env.step([1.0])
    assert reward == pytest.approx(-(math.pi**2 + 6.4 + 0.004))


def test_pendulum_truncates_at_200_and_never_terminates():
    env = PendulumEnv(seed=1)
    env.reset()
    rng = np.random.default_rng(0)
    for t in range(200):
        _, reward, terminated, truncated, _ = env.step([rng.uniform(-1, 1)])
        assert not terminated and -16.3 < reward <= 0.0
        assert truncated == (t == 199)
    assert abs(env._state[1]) <= 8.0


# --------------------------------------------------------------------------- #
# Acrobot
# --------------------------------------------------------------------------- #
def test_acrobot_reset_distribution_and_obs():
    env = AcrobotEnv(seed=0)
    lo, hi = np.full(4, np.inf), np.full(4, -np.inf)
    for _ in range(200):
        obs, info = env.reset()
        s = env._state
        lo, hi = np.minimum(lo, s), np.maximum(hi, s)
        assert obs.dtype == np.float32 and obs.shape == (6,) and info == {}
        np.testing.assert_allclose(
            obs, [math.cos(s[0]), math.sin(s[0]), math.cos(s[1]),
                  math.sin(s[1]), s[2], s[3]], atol=1e-6)
    assert (lo >= -0.1).all() and (lo < -0.08).all()
    assert (hi < 0.1).all() and (hi > 0.08).all()


def test_acrobot_hanging_at_rest_is_a_fixed_point():
    env = AcrobotEnv(seed=0)
    env.reset()
    env._state = np.zeros(4)
    for _ in range(3):
        obs, reward, terminated, truncated, _ = env.step(1)  # zero torque
        assert env._state.tolist() == [0.0] * 4
        assert obs.tolist() == [1.0, 0.0, 1.0, 0.0, 0.0, 0.0]
        assert reward == -1.0 and not terminated and not truncated


def test_acrobot_torque_is_action_minus_one():
    nxt = {}
    for a in (0, 1, 2):
        env = AcrobotEnv(seed=0)
        env.reset()
        env._state = np.zeros(4)
        env.step(a)
        nxt[a] = env._state.copy()
    # the torque acts on the second joint: opposite actions mirror the state
    assert nxt[2][3] > 0 and nxt[0][3] < 0
    np.testing.assert_allclose(nxt[0], -nxt[2], atol=1e-15)
    with pytest.raises(AssertionError):
        AcrobotEnv(seed=0).step(3)


def _numeric_gradient(s):
    g = np.zeros(4)
    for i in range(4):
        d = np.zeros(4)
        d[i] = 1e-6
        g[i] = (AcrobotEnv.energy(s + d) - AcrobotEnv.energy(s - d)) / 2e-6
    return g


def test_acrobot_energy_under_zero_torque():
    """The "book" equations are the Lagrangian ones, so without torque the
    total energy is conserved by the flow and changes over one step only by
    what RK4's local error does to it. The bound is measured, not chosen:
    the same 0.2 s taken as ten RK4 steps of 0.02 s in float64 (local error
    10^4 times smaller) gives the step's state error ``err``, and to first
    order the energy moves by at most |∇E|·|err| — asserted with a factor 1.5
    for the second-order term. The substepped run itself must conserve the
    energy 1000 times better, which is what shows E is the conserved
    quantity and not merely smooth."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(64):
        s = np.concatenate([rng.uniform(-math.pi, math.pi, 2),
                            rng.uniform(-2.0, 2.0, 2)])
        coarse = AcrobotEnv.rk4(s, 0.0, AcrobotEnv.DT)
        fine = s.copy()
        for _ in range(10):
            fine = AcrobotEnv.rk4(fine, 0.0, AcrobotEnv.DT / 10)
        e0 = AcrobotEnv.energy(s)
        drift = abs(AcrobotEnv.energy(coarse) - e0)
        drift_fine = abs(AcrobotEnv.energy(fine) - e0)
        bound = 1.5 * float(np.abs(_numeric_gradient(fine))
                            @ np.abs(coarse - fine)) + 1e-12
        assert drift <= bound, (s, drift, bound)
        assert drift_fine <= max(1e-3 * bound, 1e-12), (s, drift_fine, bound)
        worst = max(worst, drift)
    assert 0.0 < worst < 0.05  # RK4 at dt = 0.2 is good, not exact
    # a torque does work: the energy is not conserved then
    s = np.array([0.3, -0.2, 0.5, 1.0])
    pushed = AcrobotEnv.rk4(s, 1.0, AcrobotEnv.DT)
    assert abs(AcrobotEnv.energy(pushed) - AcrobotEnv.energy(s)) > 0.05


def test_acrobot_wraps_angles_and_bounds_speeds():
    env = AcrobotEnv(seed=0)
    env.reset()
    env._state = np.array([3.1, -3.1, 12.0, -28.0])
    env.step(2)
    s = env._state
    assert -math.pi <= s[0] < math.pi and -math.pi <= s[1] < math.pi
    assert abs(s[2]) <= 4 * math.pi and abs(s[3]) <= 9 * math.pi
    # unbounded step from the same state leaves the box: the bounds acted
    raw = AcrobotEnv.rk4(np.array([3.1, -3.1, 12.0, -28.0]), 1.0, 0.2)
    assert abs(raw[0]) > math.pi or abs(raw[1]) > math.pi


def test_acrobot_terminates_above_the_bar_with_reward_zero():
    env = AcrobotEnv(seed=0)
    env.reset()
    env._state = np.array([2.0, 0.0, 2.5, 1.0])  # swinging up fast
    terminated, steps = False, 0
    while not terminated and steps < 20:
        _, reward, terminated, _, _ = env.step(1)
        steps += 1
        s = env._state
        assert terminated == (-math.cos(s[0]) - math.cos(s[0] + s[1]) > 1.0)
        assert reward == (0.0 if terminated else -1.0)
    assert terminated


def test_acrobot_truncates_at_500():
    env = AcrobotEnv(seed=1)
    env.reset()
    for t in range(500):
        _, reward, terminated, truncated, _ = env.step(1)  # never swings up
        assert not terminated and reward == -1.0
        assert truncated == (t == 499)


# --------------------------------------------------------------------------- #
# workers mode: the per-env Python path (no C++ batched physics for these)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("env,algo,dims,per_worker", [
    ("Acrobot-v1", "PPO", (6, 3), 1),
    ("Pendulum-v1", "SAC-Continuous", (3, 1), 1),
    ("Pendulum-v1", "PPO-Continuous", (3, 1), 3),
])
def test_worker_collects_an_episode(env, algo, dims, per_worker):
    from pdrl_amd.agents import Worker
    from pdrl_amd.buffers.wire import is_packed, unpack_steps
    from pdrl_amd.networks import (MlpLSTMSeperateContinuous, MlpLSTMSingle,
                                   MlpLSTMSingleContinuous)
    from pdrl_amd.transport import Endpoint
    from pdrl_amd.utils import Protocol, decode, load_params

    p = load_params()
    p.env, p.algo = env, algo
    p.obs_dim, p.n_actions = dims
    p.continuous = env == "Pendulum-v1"
    p.seq_len = 5
    p.num_envs_per_worker = per_worker
    cls = {"PPO": MlpLSTMSingle, "PPO-Continuous": MlpLSTMSingleContinuous,
           "SAC-Continuous": MlpLSTMSeperateContinuous}[algo]
    mgr_sub = Endpoint(bind=("127.0.0.1", 0))
    model = cls(*dims, p.seq_len, p.hidden_size).actor
    w = Worker(model, 0, "127.0.0.1", mgr_sub.bound_port, "127.0.0.1", 1, p, seed=3)
    try:
        if per_worker > 1:
            assert w._make_batch_env() is None  # the Python loop takes over
        w.collect(max_episodes=1)
        steps = []
        while True:
            msg = mgr_sub.recv(timeout=2.0)
            if msg is None:
                break
            proto, data = decode(*msg)
            if proto is Protocol.Rollout:
                steps.extend(unpack_steps(data) if is_packed(data) else data)
        limit = 200 if env == "Pendulum-v1" else 500
        assert len(steps) >= limit  # an untrained policy runs to the limit
        for step in steps:
            assert np.asarray(step["obs"]).shape[-1] == dims[0]
            assert np.isfinite(step["log_prob"]).all()
            assert float(np.asarray(step["rew"]).reshape(-1)[0]) <= 0.0
    finally:
        w.close()
        mgr_sub.close()
