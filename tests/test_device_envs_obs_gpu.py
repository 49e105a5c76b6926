"""Device envs whose observation is not their state, on the GPU: the rollout
and evaluation kernels on Acrobot-v1 and Pendulum-v1 against the eager fp32
reference (same weights, same counter-hash stream), split launches, the
binding's env_state check and the learner end to end."""
import copy
import functools
import math

import pytest
import torch

from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.networks.models import (MlpLSTMSeperateContinuous,
                                      MlpLSTMSingleContinuous)
from pdrl_amd.ops.evaluate import DeviceEvaluator
from pdrl_amd.ops.rollout import AcrobotDyn, DeviceRollout
from tests.test_device_rollout_gpu import STATE, check_split_launches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACRO, PEN = "Acrobot-v1", "Pendulum-v1"
S = 5
MARGIN = 1e-4  # envs whose smallest decision margin is below this are excluded
FIELDS = ("obs", "act", "rew", "logits", "log_prob", "is_fir", "hx", "cx")
ULP = 2.0 ** -23


def _collect(ro, calls):
    chunks = []
    for _ in range(calls):
        b = ro.rollout()
        chunks.append({k: b[k].detach().cpu().clone() for k in FIELDS})
    return {k: torch.cat([c[k] for c in chunks], dim=1) for k in FIELDS}


def _episode_returns(ro):
    """Every finished episode's return in time order (ring not yet drained)."""
    ret = ro._ep_ring[: ro._slot].transpose(1, 2).reshape(-1).cpu()
    return ret[ret > -0.5e30]


# --------------------------------------------------------------------------- #
# Acrobot: rollout parity
# --------------------------------------------------------------------------- #
ACRO_CALLS = 8


def _acrobot_model(hidden):
    torch.manual_seed(0)
    return MlpLSTMSingle(6, 3, S, hidden)


def _swing_up_states(n_envs):
    """Fast upward swings: every env terminates within the 40 ticks."""
    i = torch.arange(n_envs, dtype=torch.float32)
    return torch.stack([1.6 + 0.9 * i / n_envs, torch.zeros(n_envs),
                        torch.full((n_envs,), 2.5), torch.ones(n_envs)],
                       1).contiguous()


def _acrobot_rollout(model, device, n_envs, seed, max_steps, preset):
    ro = DeviceRollout(model.actor.core, ACRO, n_envs, S, device, seed,
                       time_horizon=500, max_episode_steps=max_steps)
    if preset:
        ro.env_state.copy_(_swing_up_states(n_envs))
    return ro


@functools.lru_cache(maxsize=None)
def acrobot_reference(hidden, n_envs, seed, max_steps, preset):
    """(model, reference rollout after its calls, its batch) on the CPU;
    computed once per case, never modified."""
    model = _acrobot_model(hidden)
    ref = _acrobot_rollout(model, "cpu", n_envs, seed, max_steps, preset)
    assert ref.eager
    return model, ref, _collect(ref, ACRO_CALLS)


def _check_acrobot(hidden, n_envs, seed=3, max_steps=None, preset=False,
                   min_episodes=0, min_terminations=0):
    """Kernel vs eager reference over 8 x 5 ticks.

    One float rounding can flip a sampled action or the termination test,
    after which the trajectories legitimately diverge; so the reference alone
    computes, per env, the smallest margin over all ticks (|u - cdf| over
    both boundaries, |tip height - 1|) and envs below MARGIN are excluded —
    at most one may be. A wrap flip moves an angle by 2π, which neither the
    observation nor the dynamics can see, so ``obs`` is compared and
    ``env_state`` never is. Reset observations hold cos / sin of a reset
    angle, where the device and the host libm may differ by an ulp: 5e-7,
    four ulp of 1.

    Reference figures measured on the CPU (model seed 0; terminations =
    steps with reward 0):
      H=64  N=64 seed 3             : min margin 1.1e-4, 0 excluded, 0 episode ends
      H=64  N=64 seed 3 max_steps=7 : min margin 1.1e-4, 0 excluded, 320 episode ends
      H=32  N=3  seed 3             : min margin 2.2e-3, 0 excluded
      H=128 N=5  seed 3             : min margin 9.9e-4, 0 excluded
      H=64  N=64 seed 1 preset      : min margin 3.0e-4, 0 excluded, 64 terminations
    (seeds 1 and 2 exclude one env in the first case, 1.1e-5 and 8.0e-5;
    seed 2 excludes two from the preset). The untrained policy picks the
    three actions 821 / 863 / 876 times in the first case.
    """
    model, ref, want = acrobot_reference(hidden, n_envs, seed, max_steps, preset)
    gmodel = copy.deepcopy(model).to(DEV)
    ker = _acrobot_rollout(gmodel, DEV, n_envs, seed, max_steps, preset)
    assert not ker.eager and ker.env_state.shape == (n_envs, 4)
    got = _collect(ker, ACRO_CALLS)
    torch.cuda.synchronize()

    keep = ref.margin >= MARGIN
    episodes = int(_episode_returns(ref).numel())
    terminations = int((want["rew"] == 0).sum())
    counts = torch.bincount(want["act"].flatten().to(torch.int64), minlength=3)
    print(f"H={hidden} N={n_envs} seed {seed}: min margin "
          f"{float(ref.margin.min()):.3e}, excluded {int((~keep).sum())}, "
          f"episodes {episodes}, terminations {terminations}, "
          f"actions {counts.tolist()}")
    assert int((~keep).sum()) <= 1
    assert episodes >= min_episodes and terminations >= min_terminations
    assert got["obs"].shape == (n_envs, ACRO_CALLS * S, 6)
    for k in ("act", "is_fir", "rew"):
        assert torch.equal(got[k][keep], want[k][keep]), k
    for k in ("obs", "logits", "log_prob", "hx", "cx"):
        err = float((got[k][keep] - want[k][keep]).abs().max())
        print(f"  {k}: max abs err {err:.3e}")
        assert err <= 1e-4, (k, err)
    # every first observation of an episode: the hash resets and tick 0
    # (a preset start is observed by the same code)
    first = want["is_fir"][keep][:, :, 0].bool()
    assert int(first.sum()) >= int(keep.sum()) + min_terminations
    reset_err = float((got["obs"][keep][first]
                       - want["obs"][keep][first]).abs().max())
    print(f"  reset obs: max abs err {reset_err:.3e} over {int(first.sum())}")
    assert reset_err <= 5e-7
    if bool(keep.all()):
        assert ker.episode_stats() == ref.episode_stats()


def test_acrobot_parity_h64_n64():
    _check_acrobot(64, 64)


def test_acrobot_parity_truncation_path():
    _check_acrobot(64, 64, max_steps=7, min_episodes=300)


def test_acrobot_parity_h32_n3():
    _check_acrobot(32, 3)


def test_acrobot_parity_h128_streamed_weights():
    _check_acrobot(128, 5)


def test_acrobot_parity_terminations():
    """A fresh acrobot does not swing above the bar in 40 ticks, so both
    rollouts start from a preset that does: every env terminates in the
    reference, with reward 0 on that step (figures in _check_acrobot)."""
    _check_acrobot(64, 64, seed=1, preset=True, min_terminations=32)


# --------------------------------------------------------------------------- #
# Pendulum: rollout parity
# --------------------------------------------------------------------------- #
PEN_CALLS = 4  # 20 ticks: see _check_pendulum


def _pendulum_model(mode, hidden):
    torch.manual_seed(0)
    cls = MlpLSTMSingleContinuous if mode == 0 else MlpLSTMSeperateContinuous
    return cls(3, 1, S, hidden)


def _fast_states(n_envs):
    """θ = π/2 at ∓7.9 rad/s: gravity pushes half of the envs into the speed
    clip at once."""
    half = n_envs // 2
    speed = torch.cat([torch.full((half,), 7.9), torch.full((n_envs - half,), -7.9)])
    return torch.stack([torch.full((n_envs,), math.pi / 2), speed], 1).contiguous()


def _pendulum_rollout(model, device, n_envs, seed, max_steps, preset, ou_envs):
    ro = DeviceRollout(model.actor.core, PEN, n_envs, S, device, seed,
                       time_horizon=500, max_episode_steps=max_steps,
                       ou_envs=ou_envs)
    if preset:
        ro.env_state.copy_(_fast_states(n_envs))
    return ro


def _log_squash(a):
    return torch.log(1.0 - a * a + 1e-7)


def _check_pendulum(mode, hidden, n_envs, seed=3, max_steps=None,
                    min_episodes=0, preset=False, ou_envs=0, min_clipped=0):
    """Kernel vs eager reference over 4 x 5 = 20 ticks.

    The pendulum has no discontinuity (the clips are continuous, wrap(θ)² is
    continuous at ±π), so its margin is infinite and no env is excluded. It
    is unstable about the upright position (growth e^(3.9 t)), so fp32
    rounding alone grows: a fp32-against-fp64 proxy over the reset
    distribution reads 3.5e-6 after 20 ticks but 1.6e-4 after 40, hence 20
    ticks under the project's 1e-4 bound.

    Mode 1's log-prob holds log(1 - a^2 + 1e-7), which amplifies a 1-ulp
    difference of tanhf by up to 2 / (1 - a^2 + 1e-7); it is therefore held
    against the reference re-evaluated at the kernel's own action, as in
    test_device_rollout_continuous_gpu.py. Episode returns are fp32 sums of
    L rewards each within 1e-4: L * (1e-4 + 2^-23 |return|).

    Reference figures measured on the CPU (rollout seed 3, model seed 0;
    clipped = (env, tick) pairs observed at |θ̇| = 8):
      mode 0 / 1 H=64 N=64            : 2 / 7 clipped, reward down to -15.9 / -16.3
      mode 0 / 1 H=64 N=64 max_steps=7: 128 episode ends
      mode 1 H=64 N=64, 32 OU envs    : 8 clipped
      mode 0 / 1 preset               : 199 / 245 clipped
    In mode 1 the largest 2 / (1 - a^2 + 1e-7) over these runs is 1493.
    """
    model = _pendulum_model(mode, hidden)
    ref = _pendulum_rollout(model, "cpu", n_envs, seed, max_steps, preset, ou_envs)
    assert ref.eager and ref.mode == mode
    want = _collect(ref, PEN_CALLS)
    gmodel = copy.deepcopy(model).to(DEV)
    ker = _pendulum_rollout(gmodel, DEV, n_envs, seed, max_steps, preset, ou_envs)
    assert not ker.eager and ker.mode == mode
    assert ker.env_state.shape == (n_envs, 2)
    got = _collect(ker, PEN_CALLS)
    torch.cuda.synchronize()

    want_ret, got_ret = _episode_returns(ref), _episode_returns(ker)
    clipped = int((want["obs"][:, :, 2].abs() == 8.0).sum())
    print(f"mode {mode} H={hidden} N={n_envs}: min margin "
          f"{float(ref.margin.min()):.3e}, episodes {want_ret.numel()}, "
          f"clipped {clipped}")
    assert bool(torch.isinf(ref.margin).all())  # no env is excluded
    assert want_ret.numel() >= min_episodes and clipped >= min_clipped
    assert got["obs"].shape == (n_envs, PEN_CALLS * S, 3)
    assert torch.equal(got["is_fir"], want["is_fir"])
    for k in ("obs", "act", "rew", "logits", "hx", "cx"):
        err = float((got[k] - want[k]).abs().max())
        print(f"  {k}: max abs err {err:.3e}")
        assert err <= 1e-4, (k, err)
    want_lp = want["log_prob"]
    if mode == 1:
        want_lp = want_lp + _log_squash(want["act"]) - _log_squash(got["act"])
    err = float((got["log_prob"] - want_lp).abs().max())
    print(f"  log_prob: max abs err {err:.3e}")
    assert err <= 1e-4, ("log_prob", err)
    first = want["is_fir"][:, :, 0].bool()
    if preset:  # cos / sin of θ = π/2 at tick 0 is no reset of the hash
        first[:, 0] = False
    if bool(first.any()):
        reset_err = float((got["obs"][first] - want["obs"][first]).abs().max())
        print(f"  reset obs: max abs err {reset_err:.3e}")
        assert reset_err <= 5e-7
    # episode statistics: the same episodes, returns within the summation
    # bound of their length, and so is the mean of the last 50
    assert got_ret.numel() == want_ret.numel()
    if want_ret.numel():
        length = max_steps or PEN_CALLS * S
        tol = length * (1e-4 + ULP * want_ret.abs())
        assert bool(((got_ret - want_ret).abs() <= tol).all())
        games, mean50 = ref.episode_stats()
        assert ker.episode_stats()[0] == games
        assert abs(ker.episode_stats()[1] - mean50) <= float(tol.max())


@pytest.mark.parametrize("mode", [0, 1])
def test_pendulum_parity_h64_n64(mode):
    _check_pendulum(mode, 64, 64)


@pytest.mark.parametrize("mode", [0, 1])
def test_pendulum_parity_truncation_path(mode):
    _check_pendulum(mode, 64, 64, max_steps=7, min_episodes=128)


@pytest.mark.parametrize("mode", [0, 1])
def test_pendulum_parity_h32_n3(mode):
    _check_pendulum(mode, 32, 3)


@pytest.mark.parametrize("mode", [0, 1])
def test_pendulum_parity_h128_streamed_weights(mode):
    _check_pendulum(mode, 128, 5)


def test_pendulum_parity_ou():
    _check_pendulum(1, 64, 64, ou_envs=32)


@pytest.mark.parametrize("mode", [0, 1])
def test_pendulum_parity_speed_clip(mode):
    """From θ = π/2 at ±7.9 rad/s the speed clip acts at once (figures in
    _check_pendulum)."""
    _check_pendulum(mode, 64, 64, preset=True, min_clipped=32)


# --------------------------------------------------------------------------- #
# split launches
# --------------------------------------------------------------------------- #
def test_acrobot_split_launches_equal_one_launch():
    core = _acrobot_model(32).to(DEV).actor.core
    check_split_launches(
        lambda seq_len: DeviceRollout(core, ACRO, 3, seq_len, DEV, 1,
                                      time_horizon=500, max_episode_steps=7),
        min_episodes=6)


@pytest.mark.parametrize("mode,explore", [
    (0, {}),
    (1, dict(ou_envs=1, warmup_steps=8)),
])
def test_pendulum_split_launches_equal_one_launch(mode, explore):
    core = _pendulum_model(mode, 32).to(DEV).actor.core
    check_split_launches(
        lambda seq_len: DeviceRollout(core, PEN, 3, seq_len, DEV, 1,
                                      time_horizon=500, max_episode_steps=7,
                                      **explore),
        min_episodes=6, state=STATE + ("ou_state",))


# --------------------------------------------------------------------------- #
# evaluation
# --------------------------------------------------------------------------- #
EVAL_SEED = 1


@functools.lru_cache(maxsize=None)
def acrobot_eval_reference(preset):
    model = _acrobot_model(64)
    ref = DeviceEvaluator(model.actor.core, ACRO, 64, 2, "cpu", EVAL_SEED,
                          max_episode_steps=40)
    ref.evaluate(_swing_up_states(64) if preset else None)
    return model, ref


@pytest.mark.parametrize("preset", [False, True])
def test_acrobot_evaluation_parity(preset):
    """E = 2 episodes of at most 40 steps in 64 envs, from the hash start
    states and from the swing-up preset as ``start_state``. The margin is
    the gap of the two largest logits and |tip height - 1|; on the kept envs
    lengths and returns (integers) are equal.

    Reference figures measured on the CPU (eval seed 1, model seed 0):
      hash starts : min margin 1.5e-2, 0 excluded, 0 terminations
      preset      : min margin 1.0e-2, 0 excluded, 64 terminations
    (the untrained policy never changes its arg-max action here).
    """
    model, ref = acrobot_eval_reference(preset)
    want = ref.result
    ker = DeviceEvaluator(copy.deepcopy(model).to(DEV).actor.core, ACRO, 64, 2,
                          DEV, EVAL_SEED, max_episode_steps=40)
    assert not ker.eager
    got = ker.evaluate(_swing_up_states(64).to(DEV) if preset else None)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in got.items()}
    keep = ref.margin >= MARGIN
    terminations = int((want["lengths"] < 40).sum())
    print(f"preset {preset}: min margin {float(ref.margin.min()):.3e}, "
          f"excluded {int((~keep).sum())}, terminations {terminations}")
    assert int((~keep).sum()) <= 1
    assert terminations >= (32 if preset else 0)
    assert torch.equal(got["lengths"][keep], want["lengths"][keep])
    assert torch.equal(got["returns"][keep], want["returns"][keep])
    # reward -1 per step, 0 on a terminating one
    ended = (want["lengths"] < 40).float()
    assert torch.equal(want["returns"], ended - want["lengths"].float())


@pytest.mark.parametrize("mode", [0, 1])
def test_pendulum_evaluation_parity(mode):
    model = _pendulum_model(mode, 64)
    ref = DeviceEvaluator(model.actor.core, PEN, 64, 2, "cpu", EVAL_SEED,
                          max_episode_steps=20)
    want = {k: v.clone() for k, v in ref.evaluate().items()}
    ker = DeviceEvaluator(copy.deepcopy(model).to(DEV).actor.core, PEN, 64, 2,
                          DEV, EVAL_SEED, max_episode_steps=20)
    assert not ker.eager
    got = {k: v.cpu() for k, v in ker.evaluate().items()}
    assert bool((want["lengths"] == 20).all()) and bool((got["lengths"] == 20).all())
    tol = 20 * (1e-4 + ULP * want["returns"].abs())
    err = (got["returns"] - want["returns"]).abs()
    print(f"mode {mode}: max return err {float(err.max()):.3e}, "
          f"returns in [{float(want['returns'].min()):.1f}, "
          f"{float(want['returns'].max()):.1f}]")
    assert bool((err <= tol).all())
    # a given start_state replaces the hash start of episode 0 only
    start = _fast_states(64)
    want2 = {k: v.clone() for k, v in ref.evaluate(start).items()}
    got2 = {k: v.cpu() for k, v in ker.evaluate(start.to(DEV)).items()}
    assert bool(((got2["returns"] - want2["returns"]).abs()
                 <= 20 * (1e-4 + ULP * want2["returns"].abs())).all())
    assert not torch.equal(want2["returns"][:, 0], want["returns"][:, 0])
    assert torch.equal(want2["returns"][:, 1], want["returns"][:, 1])


# --------------------------------------------------------------------------- #
# binding
# --------------------------------------------------------------------------- #
def test_binding_rejects_observation_wide_env_state():
    core = _acrobot_model(64).to(DEV).actor.core
    ro = DeviceRollout(core, ACRO, 4, S, DEV, 1, time_horizon=500)
    ro.rollout()
    ro.env_state = AcrobotDyn.observe(ro.env_state).contiguous()  # (N, 6)
    with pytest.raises(RuntimeError, match="env_state"):
        ro.rollout()
    ev = DeviceEvaluator(core, ACRO, 4, 1, DEV, 1, max_episode_steps=5)
    from pdrl_amd import ops

    with pytest.raises(RuntimeError, match="start_state"):
        ops.ext().rollout_eval_discrete(
            core.body_w.detach(), core.body_b.detach(), core.w_ih.detach(),
            core.w_hh.detach(), core.b_g.detach(), core.heads_w.detach(),
            core.heads_b.detach(), ev.returns, ev.lengths,
            torch.zeros(4, 6, device=DEV), AcrobotDyn.env_id, 1, 5)


# --------------------------------------------------------------------------- #
# learner end to end
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("algo,env", [
    ("PPO", ACRO), ("IMPALA", ACRO),
    ("PPO-Continuous", PEN), ("SAC-Continuous", PEN),
])
def test_learner_device_mode_end_to_end(params, algo, env):
    from pdrl_amd.agents import Learner

    p = params
    p.algo, p.env = algo, env
    p.continuous = env == PEN
    p.obs_dim, p.n_actions = (3, 1) if env == PEN else (6, 3)
    p.batch_size, p.seq_len = 32, 5
    p.time_horizon = 20  # episodes end inside the run
    p.model_save_interval = 10_000
    p.actor_mode = "device"
    if algo == "SAC-Continuous":
        p.replay_kernel = "fused"
        p.explore_ou_envs = 8
    lrn = Learner(None, "127.0.0.1", 0, p, device=DEV)
    seen = []
    try:
        assert not lrn.device_rollout.eager
        step = lrn.updater.step
        lrn.updater.step = lambda b: seen.append(step(b)) or seen[-1]
        lrn.run(max_updates=20)
        torch.cuda.synchronize()
        assert lrn.updater.update_count == 20 and len(seen) == 20
        for stats in seen:
            assert all(math.isfinite(float(v)) for v in stats.values()), stats
        games, mean50 = lrn.device_rollout.episode_stats()
        # 20-step episodes: Acrobot pays at most -1 a step, Pendulum at most
        # -(π² + 6.4 + 0.004) ≈ -16.3
        low = -330.0 if env == PEN else -20.0
        assert games >= 1 and low <= mean50 <= 0.0
        assert int(lrn.device_rollout.tick[0]) == 20 * p.seq_len
    finally:
        lrn.close()
