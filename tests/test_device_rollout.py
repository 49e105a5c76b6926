"""Device actor mode, CPU side: the counter hash, the fp32 reference
dynamics, the rollout semantics of the eager reference path (which is also
the GPU kernel's oracle), and the learner integration."""
import math
import multiprocessing

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pdrl_amd.envs.cartpole import CartPoleEnv
from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.networks.models import MlpLSTMCritic, MlpLSTMCriticContinuous
from pdrl_amd.ops.rollout import CartPoleDyn, DeviceRollout, uniform


# --------------------------------------------------------------------------- #
# hash
# --------------------------------------------------------------------------- #
def test_hash_hand_computed_values():
    # worked by hand (integer arithmetic): h >> 8, then * 2^-24
    cases = [((1, 0, 0, 1), 7726287), ((1, 5, 7, 0), 13308281),
             ((1234, 63, 40, 4), 10905770)]
    for (seed, env, tick, k), top24 in cases:
        u = uniform(seed, torch.tensor([env]), tick, k)
        assert u.dtype == torch.float32
        assert float(u[0]) == top24 / 16777216.0
    # tensor ticks give the same stream as int ticks
    u = uniform(1, torch.tensor([5]), torch.tensor([7]), 0)
    assert float(u[0]) == 13308281 / 16777216.0


def test_hash_range_and_mean():
    u = uniform(7, torch.arange(100_000), 3, 0)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert abs(float(u.mean()) - 0.5) < 0.01


# --------------------------------------------------------------------------- #
# dynamics
# --------------------------------------------------------------------------- #
def test_cartpole_dynamics_match_env():
    rng = np.random.default_rng(0)
    # states spread over the live region, some past the thresholds
    states = rng.uniform(-1.0, 1.0, size=(32, 4)) * np.array([2.6, 2.0, 0.23, 2.0])
    for action in (0, 1):
        ref_next, ref_term = [], []
        for s in states:
            env = CartPoleEnv()
            env.reset()
            env._state = s.astype(np.float32).astype(np.float64)
            nxt, rew, term, _, _ = env.step(action)
            assert rew == 1.0
            ref_next.append(nxt)
            ref_term.append(term)
        st = torch.tensor(states, dtype=torch.float32)
        nxt, rew, term = CartPoleDyn.step(st, torch.full((32,), action))
        assert nxt.dtype == torch.float32
        np.testing.assert_allclose(nxt.numpy(), np.stack(ref_next), atol=1e-6, rtol=0)
        assert term.tolist() == ref_term
        assert any(ref_term) and not all(ref_term)
        assert torch.equal(rew, torch.ones(32))


# --------------------------------------------------------------------------- #
# rollout semantics (eager reference)
# --------------------------------------------------------------------------- #
N, S, CALLS, MAX_STEPS = 8, 5, 6, 7


def _run(seed, calls=CALLS):
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, S, 64)
    ro = DeviceRollout(model.actor.core, "CartPole-v1", N, S, "cpu", seed,
                       time_horizon=500, max_episode_steps=MAX_STEPS)
    chunks, objs = [], []
    for _ in range(calls):
        b = ro.rollout()
        objs.append({k: id(v) for k, v in b.items()})
        chunks.append({k: v.clone() for k, v in b.items()})
    cat = {k: torch.cat([c[k] for c in chunks], dim=1) for k in chunks[0]}
    return model, ro, cat, objs


@pytest.fixture(scope="module")
def run1():
    return _run(seed=1)


def test_rollout_fields_and_stable_tensors(run1):
    from pdrl_amd.buffers import rollout_fields

    _, ro, cat, objs = run1
    fields = rollout_fields(4, 2, 64, False)
    assert list(cat) == list(fields)
    for k, d in fields.items():
        assert cat[k].shape == (N, S * CALLS, d) and cat[k].dtype == torch.float32
    assert all(o == objs[0] for o in objs)  # same tensor objects every call


def test_rollout_reset_semantics(run1):
    model, ro, cat, _ = run1
    T = S * CALLS
    # CartPole cannot fall within 7 steps of a [-0.05, 0.05) start, so every
    # episode is truncated at exactly MAX_STEPS: resets after ticks 7, 14, ...
    fir = cat["is_fir"][:, :, 0]
    expect = torch.tensor([1.0 if t % MAX_STEPS == 0 else 0.0 for t in range(T)])
    assert torch.equal(fir, expect.expand(N, T))
    first = fir.bool()
    assert torch.count_nonzero(cat["hx"][first]) == 0
    assert torch.count_nonzero(cat["cx"][first]) == 0
    assert cat["obs"][first].abs().max() <= 0.05
    assert torch.equal(cat["rew"], torch.ones(N, T, 1))
    # reset states come from lanes 1..4 of the tick that caused the reset
    envs = torch.arange(N)
    for t in range(0, T, MAX_STEPS):
        want = torch.stack([-0.05 + 0.1 * uniform(1, envs, t, k)
                            for k in range(1, 5)], 1)
        assert torch.equal(cat["obs"][:, t], want)

    core = model.actor.core
    with torch.no_grad():
        for t in range(T):
            outs, h, c = core._forward_eager(
                cat["obs"][:, t : t + 1], cat["hx"][:, t], cat["cx"][:, t])
            torch.testing.assert_close(outs["logits"][:, 0], cat["logits"][:, t],
                                       atol=1e-6, rtol=0)
            if t + 1 < T and (t + 1) % MAX_STEPS != 0:
                # carried recurrent state and env state
                torch.testing.assert_close(cat["hx"][:, t + 1], h, atol=1e-6, rtol=0)
                torch.testing.assert_close(cat["cx"][:, t + 1], c, atol=1e-6, rtol=0)
                nxt, _, term = CartPoleDyn.step(
                    cat["obs"][:, t], cat["act"][:, t, 0].long())
                assert not term.any()
                assert torch.equal(cat["obs"][:, t + 1], nxt)


def test_rollout_sampling_and_log_prob(run1):
    _, _, cat, _ = run1
    act = cat["act"].long()
    assert set(act.unique().tolist()) == {0, 1}
    logp = F.log_softmax(cat["logits"], dim=-1).gather(-1, act)
    torch.testing.assert_close(cat["log_prob"], logp, atol=1e-6, rtol=0)
    # inverse CDF: action 0 iff u < p(0), with u = lane 0 of the step's tick
    T = S * CALLS
    p0 = F.softmax(cat["logits"], dim=-1)[:, :, 0]
    u = torch.stack([uniform(1, torch.arange(N), t + 1, 0) for t in range(T)], 1)
    clear = (u - p0).abs() > 1e-5
    assert torch.equal((u >= p0)[clear], act[:, :, 0].bool()[clear])


def test_episode_stats_count_resets(run1):
    _, ro, cat, _ = run1
    T = S * CALLS
    resets = N * (T // MAX_STEPS)  # a reset after ticks 7, 14, 21, 28
    games, mean50 = ro.episode_stats()
    assert games == resets
    assert mean50 == float(MAX_STEPS)
    assert ro.episode_stats() == (games, mean50)  # idempotent without new calls


def test_episode_stats_survive_many_calls():
    # more calls than ep_ret slots between two reductions: nothing is lost
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, 1, 32)
    ro = DeviceRollout(model.actor.core, "CartPole-v1", 2, 1, "cpu", 3,
                       time_horizon=4)
    calls = DeviceRollout.STATS_SLOTS * 2 + 8
    for _ in range(calls):
        ro.rollout()
    games, mean50 = ro.episode_stats()
    assert games == 2 * (calls // 4)  # horizon reset every 4 steps
    assert mean50 == 4.0


def test_seed_reproduces_and_differs(run1):
    _, _, cat, _ = run1
    _, _, again, _ = _run(seed=1)
    for k in cat:
        assert torch.equal(cat[k], again[k]), k
    _, _, other, _ = _run(seed=2)
    assert not torch.equal(cat["obs"], other["obs"])
    assert not torch.equal(cat["act"], other["act"])


def test_time_horizon_resets_without_done():
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, S, 32)
    ro = DeviceRollout(model.actor.core, "CartPole-v1", 3, S, "cpu", 5,
                       time_horizon=3)
    fir = torch.cat([ro.rollout()["is_fir"].clone() for _ in range(2)], 1)[:, :, 0]
    expect = torch.tensor([1.0 if t % 3 == 0 else 0.0 for t in range(2 * S)])
    assert torch.equal(fir, expect.expand(3, 2 * S))
    assert ro.episode_stats() == (3 * 3, 3.0)


def test_rejects_unsupported_configurations():
    ok = MlpLSTMSingle(4, 2, S, 64).actor.core
    with pytest.raises(ValueError, match="no device dynamics"):
        DeviceRollout(ok, "MountainCar-v0", 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="dual-body"):
        DeviceRollout(MlpLSTMCriticContinuous(4, 2, S, 64).core,
                      "CartPole-v1", 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="first head"):
        DeviceRollout(MlpLSTMCritic(4, 2, S, 64).core,
                      "CartPole-v1", 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="hidden size"):
        DeviceRollout(MlpLSTMSingle(4, 2, S, 48).actor.core,
                      "CartPole-v1", 4, S, "cpu", 0, 500)
    with pytest.raises(ValueError, match="does not match"):
        DeviceRollout(MlpLSTMSingle(6, 3, S, 64).actor.core,
                      "CartPole-v1", 4, S, "cpu", 0, 500)


# --------------------------------------------------------------------------- #
# learner integration
# --------------------------------------------------------------------------- #
def _device_params(params, algo):
    params.algo = algo
    params.env = "CartPole-v1"
    params.obs_dim, params.n_actions, params.continuous = 4, 2, False
    params.actor_mode = "device"
    return params


def test_learner_device_mode_impala(params):
    from pdrl_amd.agents import Learner
    from pdrl_amd.buffers import SharedRolloutRing, rollout_fields

    p = _device_params(params, "IMPALA")
    fields = rollout_fields(p.obs_dim, p.n_actions, p.hidden_size, False)
    ring = SharedRolloutRing(fields, p.seq_len, p.batch_size, True)
    stat = multiprocessing.Array("d", 3)
    seen = []
    lrn = Learner(ring, "127.0.0.1", 0, p, device="cpu", shared_stat=stat)
    try:
        assert lrn.pub is None  # no weight plane in device mode
        step = lrn.updater.step
        lrn.updater.step = lambda b: seen.append(step(b)) or seen[-1]
        lrn.run(max_updates=3)
        assert lrn.updater.update_count == 3
        assert ring._head.value == 0 and ring.available() == 0
        assert len(seen) == 3
        for stats in seen:
            assert all(math.isfinite(float(v)) for v in stats.values())
        assert lrn.device_rollout.N == p.batch_size
        assert int(lrn.device_rollout.tick[0]) == 3 * p.seq_len
        assert stat[0] == lrn.device_rollout.episode_stats()[0]
    finally:
        lrn.close()


def test_learner_device_mode_sac_uses_replay(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params, "SAC")
    p.device_envs = 4  # fewer envs than the batch: replay warm-up path
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        lrn.run(max_updates=2)
        assert lrn.updater.update_count == 2
        assert lrn.device_replay.size >= p.batch_size
    finally:
        lrn.close()


def test_learner_device_mode_rejects_unsupported(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params, "PPO-Continuous")
    p.n_actions = 1
    with pytest.raises(ValueError, match="discrete policies only"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")
    p = _device_params(params, "PPO")
    p.env = "MountainCar-v0"
    p.obs_dim, p.n_actions = 2, 3
    with pytest.raises(ValueError, match="no device dynamics"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")
