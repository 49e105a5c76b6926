"""Device actor mode on the GPU: the fused rollout kernel against the eager
fp32 reference (same weights, same counter-hash stream), its storage / live
weight contracts, and the learner end to end."""
import copy
import math

import pytest
import torch

from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.ops.rollout import DeviceRollout, uniform

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S, CALLS = 5, 8
MARGIN = 1e-4  # envs whose smallest decision margin is below this are excluded
FIELDS = ("obs", "act", "rew", "logits", "log_prob", "is_fir", "hx", "cx")


def _collect(ro):
    chunks = []
    for _ in range(CALLS):
        b = ro.rollout()
        chunks.append({k: b[k].detach().cpu().clone() for k in FIELDS})
    return {k: torch.cat([c[k] for c in chunks], dim=1) for k in FIELDS}


def _check_parity(hidden, n_envs, seed, max_steps, min_episodes):
    """Kernel vs eager reference over CALLS x S ticks.

    One float rounding can flip a sampled action or a termination, after
    which the trajectories legitimately diverge; so the reference alone
    computes, per env, the smallest margin over all ticks (|u - cdf
    boundary|, distance of |x| / |theta| from its threshold) and envs below
    MARGIN are excluded — at most one may be.

    Reference margins measured on the CPU (rollout seed 1, model seed 0):
      H=64  N=64            : 90 episode ends, min margin 2.3e-4, 0 excluded
      H=64  N=64 max_steps=7: 320 episode ends, min margin 4.3e-4, 0 excluded
      H=32  N=3             : min margin 9.5e-5, 1 excluded
      H=128 N=5             : 8 episode ends, min margin 1.2e-3, 0 excluded
    """
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, S, hidden)
    ref = DeviceRollout(model.actor.core, "CartPole-v1", n_envs, S, "cpu", seed,
                        time_horizon=500, max_episode_steps=max_steps)
    gmodel = copy.deepcopy(model).to(DEV)
    ker = DeviceRollout(gmodel.actor.core, "CartPole-v1", n_envs, S, DEV, seed,
                        time_horizon=500, max_episode_steps=max_steps)
    assert ref.eager and not ker.eager
    want, got = _collect(ref), _collect(ker)
    torch.cuda.synchronize()

    keep = ref.margin >= MARGIN
    print(f"H={hidden} N={n_envs}: min margin {float(ref.margin.min()):.3e}, "
          f"excluded {int((~keep).sum())}, episodes {ref.episode_stats()[0]}")
    assert int((~keep).sum()) <= 1
    assert ref.episode_stats()[0] >= min_episodes
    for k in ("act", "is_fir", "rew"):
        assert torch.equal(got[k][keep], want[k][keep]), k
    for k in ("obs", "logits", "log_prob", "hx", "cx"):
        err = float((got[k][keep] - want[k][keep]).abs().max())
        print(f"  {k}: max abs err {err:.3e}")
        assert err <= 1e-4, (k, err)
    first = want["is_fir"][keep][:, :, 0].bool()
    reset_err = float((got["obs"][keep][first] - want["obs"][keep][first]).abs().max())
    print(f"  reset obs: max abs err {reset_err:.3e}")
    assert reset_err <= 1e-7
    # lazily reduced episode statistics agree for the included envs' world
    if bool(keep.all()):
        assert ker.episode_stats() == ref.episode_stats()


def test_parity_h64_n64():
    _check_parity(64, 64, seed=1, max_steps=None, min_episodes=60)


def test_parity_h32_n3():
    _check_parity(32, 3, seed=1, max_steps=None, min_episodes=1)


def test_parity_truncation_path():
    _check_parity(64, 64, seed=1, max_steps=7, min_episodes=300)


def test_parity_h128_streamed_weights():
    # H=128 keeps only w_hh in registers and streams w_ih: its own code path
    _check_parity(128, 5, seed=1, max_steps=None, min_episodes=1)


STATE = ("env_state", "h", "c", "is_fir", "ep_steps", "ep_run", "tick")


def check_split_launches(make, min_episodes, state=STATE):
    """Four launches of 5 steps equal one launch of 20, bit for bit: a rollout
    is a pure function of the per-env state that one launch hands to the
    next, so no margin mask and no tolerance. ``make(seq_len)`` builds the
    rollout; both get the same core and seed."""
    split, whole = make(5), make(20)
    assert split.eager == whole.eager == (split.device.type == "cpu")
    chunks = [{k: v.clone() for k, v in split.rollout().items()}
              for _ in range(4)]
    want = whole.rollout()
    for k in want:
        assert torch.equal(torch.cat([c[k] for c in chunks], dim=1), want[k]), k
    for k in state:
        assert torch.equal(getattr(split, k), getattr(whole, k)), k
    games, mean50 = whole.episode_stats()
    assert games >= min_episodes  # resets inside and across the launches
    assert split.episode_stats() == (games, mean50)


def test_split_launches_equal_one_launch():
    # max_episode_steps=7: every env truncates at least twice in 20 steps,
    # with ep_steps 5, 3 and 1 (or less) carried over the three boundaries
    torch.manual_seed(0)
    core = MlpLSTMSingle(4, 2, S, 32).to(DEV).actor.core
    check_split_launches(
        lambda seq_len: DeviceRollout(core, "CartPole-v1", 3, seq_len, DEV, 1,
                                      time_horizon=500, max_episode_steps=7),
        min_episodes=6)


def test_host_hash_matches_reference():
    from pdrl_amd import ops

    for seed, env, tick, k in [(1, 0, 0, 1), (1, 5, 7, 0), (1234, 63, 40, 4),
                               (0xFFFFFFFF, 99999, 123456, 3)]:
        want = float(uniform(seed, torch.tensor([env]), tick, k)[0])
        assert ops.ext().rollout_uniform(seed, env, tick, k) == want


def _gpu_rollout(n_envs=16, seed=3, model=None):
    if model is None:
        torch.manual_seed(0)
        model = MlpLSTMSingle(4, 2, S, 64).to(DEV)
    return model, DeviceRollout(model.actor.core, "CartPole-v1", n_envs, S, DEV,
                                seed, time_horizon=500)


def test_stable_storage():
    _, ro = _gpu_rollout()
    first = ro.rollout()
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    for _ in range(3):
        again = ro.rollout()
        assert all(again[k] is first[k] for k in first)
        assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    assert int(ro.tick[0]) == 4 * S and int(ro.tick[-1]) == 4 * S


def test_reads_live_weights():
    model, a = _gpu_rollout()
    logits_before = a.rollout()["logits"][:, 0, 0].clone()
    with torch.no_grad():
        model.actor.core.heads_b[0] += 0.5  # in place, as the optimizer does
    _, b = _gpu_rollout(model=model)  # same seed: same first-step inputs
    logits_after = b.rollout()["logits"][:, 0, 0]
    torch.testing.assert_close(logits_after, logits_before + 0.5,
                               atol=1e-5, rtol=0)


def test_eager_flag_runs_reference_on_gpu(monkeypatch):
    monkeypatch.setenv("PDRL_ROLLOUT_EAGER", "1")
    _, ro = _gpu_rollout(n_envs=4)
    assert ro.eager
    b = ro.rollout()
    assert b["obs"].is_cuda and bool((b["is_fir"][:, 0, 0] == 1).all())


def test_kernel_rejects_bad_tensors():
    _, ro = _gpu_rollout(n_envs=4)
    ro.batch["hx"] = ro.batch["hx"][:, :, :32]  # wrong size, non-contiguous
    with pytest.raises(RuntimeError, match="hx"):
        ro.rollout()


@pytest.mark.parametrize("algo", ["IMPALA", "PPO"])
def test_learner_device_mode_end_to_end(params, algo):
    from pdrl_amd.agents import Learner

    p = params
    p.algo, p.env = algo, "CartPole-v1"
    p.obs_dim, p.n_actions, p.continuous = 4, 2, False
    p.batch_size, p.seq_len = 32, 5
    p.model_save_interval = 10_000
    p.actor_mode = "device"
    lrn = Learner(None, "127.0.0.1", 0, p, device=DEV)
    seen = []
    try:
        step = lrn.updater.step
        lrn.updater.step = lambda b: seen.append(step(b)) or seen[-1]
        lrn.run(max_updates=20)
        torch.cuda.synchronize()
        assert lrn.updater.update_count == 20
        assert len(seen) == 20
        for stats in seen:
            assert all(math.isfinite(float(v)) for v in stats.values()), stats
        games, mean50 = lrn.device_rollout.episode_stats()
        assert games >= 1 and 1.0 <= mean50 <= 500.0
        assert int(lrn.device_rollout.tick[0]) == 20 * p.seq_len
    finally:
        lrn.close()
