"""Continuous-control device actor on the GPU: the fused Gaussian rollout
kernel against the eager fp32 reference (same weights, same counter-hash
stream) for both sampling schemes, its storage / live weight contracts, and
the learner end to end."""
import copy
import math

import pytest
import torch

from pdrl_amd.networks.models import (MlpLSTMSeperateContinuous,
                                      MlpLSTMSingleContinuous)
from pdrl_amd.ops.rollout import DeviceRollout
from tests.test_device_rollout_gpu import STATE, check_split_launches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENV = "MountainCarContinuous-v0"
S, CALLS = 5, 8
MARGIN = 1e-4  # envs whose smallest decision margin is below this are excluded
FIELDS = ("obs", "act", "rew", "logits", "log_prob", "is_fir", "hx", "cx")


def _model(mode, hidden):
    torch.manual_seed(0)
    cls = MlpLSTMSingleContinuous if mode == 0 else MlpLSTMSeperateContinuous
    return cls(2, 1, S, hidden)


def _collect(ro):
    chunks = []
    for _ in range(CALLS):
        b = ro.rollout()
        chunks.append({k: b[k].detach().cpu().clone() for k in FIELDS})
    return {k: torch.cat([c[k] for c in chunks], dim=1) for k in FIELDS}


def _threshold_states(n_envs):
    """First half runs into the goal, second half into the left wall."""
    half = n_envs // 2
    i = torch.arange(half, dtype=torch.float32)
    goal = torch.stack([0.30 + 0.14 * i / half, torch.full((half,), 0.04)], 1)
    wall = torch.stack([-1.19 + 0.12 * i / half, torch.full((half,), -0.04)], 1)
    return torch.cat([goal, wall]).contiguous()


def _rollout(model, device, n_envs, seed, max_steps, preset, ou_envs):
    ro = DeviceRollout(model.actor.core, ENV, n_envs, S, device, seed,
                       time_horizon=500, max_episode_steps=max_steps,
                       ou_envs=ou_envs)
    if preset:
        ro.env_state.copy_(_threshold_states(n_envs))
    return ro


def _reference(mode, hidden, n_envs, seed, max_steps, preset=False, ou_envs=0):
    """(model, reference rollout after CALLS calls, its (N, CALLS*S, .) batch)
    on the CPU."""
    model = _model(mode, hidden)
    ref = _rollout(model, "cpu", n_envs, seed, max_steps, preset, ou_envs)
    assert ref.eager and ref.mode == mode
    return model, ref, _collect(ref)


def _log_squash(a):
    return torch.log(1.0 - a * a + 1e-7)


def _check_parity(mode, hidden, n_envs, seed=1, max_steps=None, min_episodes=0,
                  preset=False, ou_envs=0, min_goals=0, min_walls=0):
    """Kernel vs eager reference over CALLS x S ticks.

    A Gaussian sample has no decision boundary, but one float rounding can
    still move a trajectory across the left wall (velocity zeroing), the
    goal position or, past the goal, zero velocity; after that the
    trajectories legitimately diverge. So the reference alone computes, per
    env, the smallest such distance over all ticks and envs below MARGIN are
    excluded — at most one may be.

    Mode 1's log-prob holds log(1 - a^2 + 1e-7), which amplifies a 1-ulp
    difference of tanhf by up to 2 / (1 - a^2 + 1e-7) (hundreds); it is
    therefore held against the reference re-evaluated at the kernel's own
    action, want_lp + L(want_act) - L(got_act), and the action separately.

    Reference figures measured on the CPU (rollout seed 1, model seed 0;
    goals = terminations at the goal, walls = (env, tick) pairs observed at
    the left wall):
      mode 0 H=64  N=64            : min margin 4.8e-1, 0 excluded
      mode 1 H=64  N=64            : min margin 4.7e-1, 0 excluded
      mode 0 H=64  N=64 max_steps=7: 320 episode ends, min margin 6.0e-1, 0 excluded
      mode 1 H=64  N=64 max_steps=7: 320 episode ends, min margin 6.0e-1, 0 excluded
      mode 0 H=32  N=3             : min margin 5.6e-1, 0 excluded
      mode 1 H=32  N=3             : min margin 5.6e-1, 0 excluded
      mode 0 H=128 N=5             : min margin 6.2e-1, 0 excluded
      mode 1 H=128 N=5             : min margin 6.1e-1, 0 excluded
      mode 0 thresholds            : 32 goals, 32 walls, min margin 1.4e-4, 0 excluded
      mode 1 thresholds            : 32 goals, 32 walls, min margin 2.0e-5, 1 excluded
      mode 1 thresholds, 32 OU envs: 32 goals, 32 walls, min margin 2.0e-5, 1 excluded
    In mode 1 the largest 2 / (1 - a^2 + 1e-7) over these runs is 1615.
    """
    model, ref, want = _reference(mode, hidden, n_envs, seed, max_steps,
                                  preset, ou_envs)
    gmodel = copy.deepcopy(model).to(DEV)
    ker = _rollout(gmodel, DEV, n_envs, seed, max_steps, preset, ou_envs)
    assert not ker.eager and ker.mode == mode
    got = _collect(ker)
    torch.cuda.synchronize()

    keep = ref.margin >= MARGIN
    goals = int((want["rew"] > 50.0).sum())
    walls = int((want["obs"][:, :, 0] <= -1.2).sum())
    episodes = ref.episode_stats()[0]
    print(f"mode {mode} H={hidden} N={n_envs}: min margin "
          f"{float(ref.margin.min()):.3e}, excluded {int((~keep).sum())}, "
          f"episodes {episodes}, goals {goals}, walls {walls}")
    assert int((~keep).sum()) <= 1
    assert episodes >= min_episodes and goals >= min_goals and walls >= min_walls
    assert torch.equal(got["is_fir"][keep], want["is_fir"][keep])
    for k in ("obs", "act", "rew", "logits", "hx", "cx"):
        err = float((got[k][keep] - want[k][keep]).abs().max())
        print(f"  {k}: max abs err {err:.3e}")
        assert err <= 1e-4, (k, err)
    want_lp = want["log_prob"]
    if mode == 1:
        want_lp = want_lp + _log_squash(want["act"]) - _log_squash(got["act"])
    err = float((got["log_prob"][keep] - want_lp[keep]).abs().max())
    print(f"  log_prob: max abs err {err:.3e}")
    assert err <= 1e-4, ("log_prob", err)
    first = want["is_fir"][keep][:, :, 0].bool()
    reset_err = float((got["obs"][keep][first] - want["obs"][keep][first]).abs().max())
    print(f"  reset obs: max abs err {reset_err:.3e}")
    assert reset_err <= 1e-7
    # lazily reduced episode statistics (returns are float sums here)
    assert ker.episode_stats()[0] == episodes
    if bool(keep.all()):
        assert abs(ker.episode_stats()[1] - ref.episode_stats()[1]) <= 1e-3


@pytest.mark.parametrize("mode", [0, 1])
def test_parity_h64_n64(mode):
    _check_parity(mode, 64, 64)


@pytest.mark.parametrize("mode", [0, 1])
def test_parity_truncation_path(mode):
    _check_parity(mode, 64, 64, max_steps=7, min_episodes=300)


@pytest.mark.parametrize("mode", [0, 1])
def test_parity_h32_n3(mode):
    _check_parity(mode, 32, 3)


@pytest.mark.parametrize("mode", [0, 1])
def test_parity_h128_streamed_weights(mode):
    # H=128 keeps only w_hh in registers and streams w_ih: its own code path
    _check_parity(mode, 128, 5)


@pytest.mark.parametrize("mode", [0, 1])
def test_parity_thresholds(mode):
    """A fresh car reaches neither the goal nor the wall in 40 ticks, so both
    rollouts start from a preset state that runs into them: in the reference
    all 32 goal runners terminate and all 32 wall runners touch the wall
    (figures in _check_parity)."""
    _check_parity(mode, 64, 64, preset=True, min_goals=30, min_walls=30)


def test_parity_thresholds_ou():
    """The threshold case with the first 32 envs (the goal runners) on OU
    exploration (figures in _check_parity)."""
    _check_parity(1, 64, 64, preset=True, ou_envs=32, min_goals=30, min_walls=30)


@pytest.mark.parametrize("mode,explore", [
    (0, {}),
    # env 0 explores forever, the others until tick 8 (inside the second
    # launch): the OU state is carried over launches and zeroed by resets
    (1, dict(ou_envs=1, warmup_steps=8)),
])
def test_split_launches_equal_one_launch(mode, explore):
    # max_episode_steps=3: six truncations per env in 20 steps, one of them
    # on the last step of the third launch (is_fir = 1 carried over), and
    # ep_steps 2 and 1 carried over the first two boundaries
    core = _model(mode, 32).to(DEV).actor.core
    check_split_launches(
        lambda seq_len: DeviceRollout(core, ENV, 3, seq_len, DEV, 1,
                                      time_horizon=500, max_episode_steps=3,
                                      **explore),
        min_episodes=18, state=STATE + ("ou_state",))


# --------------------------------------------------------------------------- #
def _gpu_rollout(mode=1, n_envs=16, seed=3, model=None, **kw):
    if model is None:
        model = _model(mode, 64).to(DEV)
    return model, DeviceRollout(model.actor.core, ENV, n_envs, S, DEV, seed,
                                time_horizon=500, **kw)


@pytest.mark.parametrize("mode", [0, 1])
def test_stable_storage(mode):
    _, ro = _gpu_rollout(mode)
    first = ro.rollout()
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    for _ in range(3):
        again = ro.rollout()
        assert all(again[k] is first[k] for k in first)
        assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    assert int(ro.tick[0]) == 4 * S and int(ro.tick[-1]) == 4 * S


@pytest.mark.parametrize("mode", [0, 1])
def test_reads_live_weights(mode):
    model, a = _gpu_rollout(mode)
    mu_before = a.rollout()["logits"][:, 0, 0].clone()
    with torch.no_grad():
        model.actor.core.heads_b[0] += 0.5  # in place, as the optimizer does
    _, b = _gpu_rollout(mode, model=model)  # same seed: same first-step inputs
    mu_after = b.rollout()["logits"][:, 0, 0]
    torch.testing.assert_close(mu_after, mu_before + 0.5, atol=1e-5, rtol=0)


def test_eager_flag_runs_reference_on_gpu(monkeypatch):
    monkeypatch.setenv("PDRL_ROLLOUT_EAGER", "1")
    _, ro = _gpu_rollout(n_envs=4, ou_envs=2)
    assert ro.eager
    b = ro.rollout()
    assert b["obs"].is_cuda and bool((b["is_fir"][:, 0, 0] == 1).all())
    assert bool((b["act"].abs() <= 1).all()) and ro.margin.is_cuda
    assert bool((ro.ou_state[:2] != 0).all()) and bool((ro.ou_state[2:] == 0).all())


def test_kernel_rejects_bad_tensors():
    _, ro = _gpu_rollout(n_envs=4)
    ro.batch["hx"] = ro.batch["hx"][:, :, :32]  # wrong size, non-contiguous
    with pytest.raises(RuntimeError, match="hx"):
        ro.rollout()
    _, ro = _gpu_rollout(n_envs=4)
    ro.ou_state = ro.ou_state[:2]
    with pytest.raises(RuntimeError, match="ou_state"):
        ro.rollout()


@pytest.mark.parametrize("algo", ["PPO-Continuous", "SAC-Continuous"])
def test_learner_device_mode_end_to_end(params, algo):
    from pdrl_amd.agents import Learner

    p = params
    p.algo, p.env = algo, ENV
    p.obs_dim, p.n_actions, p.continuous = 2, 1, True
    p.batch_size, p.seq_len = 32, 5
    p.model_save_interval = 10_000
    p.actor_mode = "device"
    if algo == "SAC-Continuous":
        p.explore_ou_envs = 8
    lrn = Learner(None, "127.0.0.1", 0, p, device=DEV)
    seen = []
    try:
        assert not lrn.device_rollout.eager
        assert lrn.device_rollout.ou_envs == (8 if algo == "SAC-Continuous" else 0)
        step = lrn.updater.step
        lrn.updater.step = lambda b: seen.append(step(b)) or seen[-1]
        lrn.run(max_updates=20)
        torch.cuda.synchronize()
        assert lrn.updater.update_count == 20
        assert len(seen) == 20
        for stats in seen:
            assert all(math.isfinite(float(v)) for v in stats.values()), stats
        games, mean50 = lrn.device_rollout.episode_stats()
        # time_horizon = 64 ends every episode within the 100 ticks; a
        # <= 64-step episode returns between -0.1 * 64 and 100
        assert games >= 1 and -6.4 <= mean50 <= 100.0
        assert int(lrn.device_rollout.tick[0]) == 20 * p.seq_len
    finally:
        lrn.close()
