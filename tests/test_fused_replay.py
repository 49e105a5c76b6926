"""FusedDeviceReplay on the CPU: the hash-drawn index stream, ring semantics
against DeviceReplay, the class contract, and the learner wiring — all on
the pure-torch path that is the kernel's oracle (tests/test_fused_replay_gpu.py
holds the kernel against it)."""
import math

import pytest
import torch

from pdrl_amd.buffers.device_replay import (DeviceReplay, FusedDeviceReplay,
                                            replay_slots)
from pdrl_amd.ops.rollout import hash_bits, uniform

FIELDS = {"obs": 4, "act": 1, "rew": 1, "hx": 8}
S = 5


def make(n, start, fields=FIELDS, seq=S):
    """n trajectories whose every element is unique across calls when
    ``start`` advances by n: value = trajectory number + element / 1000."""
    out = {}
    for name, dim in fields.items():
        elem = torch.arange(seq * dim, dtype=torch.float32).view(1, seq, dim)
        traj = torch.arange(start, start + n, dtype=torch.float32).view(n, 1, 1)
        out[name] = traj + elem / 1000.0
    return out


# --------------------------------------------------------------------------- #
# index stream
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("draw,filled,expected", [
    (1, 8, [3, 6, 4, 5]),
    (2, 8, [7, 1, 4, 1]),
    (1, 2 ** 31 - 1, [847112714, 1800416035, 1187927306, 1587310447]),
])
def test_known_slots(draw, filled, expected):
    assert replay_slots(1234, 4, draw, filled).tolist() == expected


def test_slots_follow_the_documented_rule():
    rows = torch.arange(4, dtype=torch.int64)
    h = hash_bits(1234 ^ 0x5BD1E995, rows, 1, 7)
    assert h.dtype == torch.int64
    assert bool((h >= 0).all()) and bool((h < 2 ** 32).all())
    assert torch.equal((h * 8) >> 32, replay_slots(1234, 4, 1, 8))


def test_hash_bits_is_the_uniform_numerator():
    env = torch.arange(16, dtype=torch.int64)
    for seed, tick, k in ((0, 0, 0), (1234, 1, 7), (0xFFFFFFFF, 2 ** 29 - 1, 5),
                          (7, torch.arange(16) * 1000, 3)):
        h = hash_bits(seed, env, tick, k)
        assert bool((h >= 0).all()) and bool((h < 2 ** 32).all())
        u = (h >> 8).to(torch.float32) * (1.0 / 16777216.0)
        assert torch.equal(u, uniform(seed, env, tick, k))


def test_slot_distribution():
    counts = torch.zeros(64, dtype=torch.int64)
    for draw in range(1, 65):
        idx = replay_slots(1234, 128, draw, 64)
        assert int(idx.min()) >= 0 and int(idx.max()) < 64
        counts += torch.bincount(idx, minlength=64)
    assert int(counts.sum()) == 8192
    lo, hi = int(counts.min()), int(counts.max())
    print(f"slot counts: min {lo} max {hi} (expectation 128)")
    assert 80 <= lo and hi <= 176


# --------------------------------------------------------------------------- #
# ring semantics
# --------------------------------------------------------------------------- #
def test_ring_semantics_equal_device_replay():
    old = DeviceReplay(FIELDS, S, 11, "cpu")
    new = FusedDeviceReplay(FIELDS, S, 11, "cpu")
    # same starting bytes, so never-written slots compare equal too
    for name in FIELDS:
        old._store[name].zero_()
        new._store[name].zero_()
    start = 0
    for n in (4, 5, 11, 3):  # 5 wraps, 11 = capacity
        batch = make(n, start)
        start += n
        old.append_batch(batch)
        new.append_batch(batch)
        assert new.size == old.size
        for name in FIELDS:
            assert torch.equal(new._store[name], old._store[name]), (n, name)
    assert new.capacity == old.capacity == 11
    assert new.nbytes() == old.nbytes()


def test_numpy_and_flat_rows_are_accepted():
    a = FusedDeviceReplay(FIELDS, S, 8, "cpu")
    b = FusedDeviceReplay(FIELDS, S, 8, "cpu")
    batch = make(3, 0)
    a.append_batch(batch)
    b.append_batch({k: v.numpy().reshape(3, -1) for k, v in batch.items()})
    for name in FIELDS:
        assert torch.equal(a._store[name][:3], b._store[name][:3])


# --------------------------------------------------------------------------- #
# class behaviour
# --------------------------------------------------------------------------- #
def test_push_sample_returns_none_until_filled_but_pushes():
    rep = FusedDeviceReplay(FIELDS, S, 16, "cpu", seed=3)
    assert rep.sample(1) is None
    assert rep.push_sample(make(4, 0), 6) is None
    assert rep.size == 4 and rep._draws == 0
    assert torch.equal(rep._store["obs"][:4], make(4, 0)["obs"])
    out = rep.push_sample(make(2, 4), 6)  # filled == n_sample: enough
    assert out is not None and rep.size == 6 and rep._draws == 1
    assert out["hx"].shape == (6, S, 8)
    # the first produced batch is draw 1 at filled 6
    idx = replay_slots(3, 6, 1, 6)
    assert torch.equal(out["obs"], rep._store["obs"][idx])
    # push-only and empty pushes never advance the draw counter
    rep.append_batch(make(1, 6))
    rep.append_batch(make(0, 7))
    assert rep.size == 7 and rep._draws == 1
    assert rep.push_sample(None, 0) is None


def test_samples_come_from_filled_slots_only():
    rep = FusedDeviceReplay(FIELDS, S, 64, "cpu", seed=5)
    for t in rep._store.values():
        t.fill_(float("nan"))
    rep.append_batch(make(10, 0))
    for _ in range(20):
        out = rep.sample(10)
        for name, t in out.items():
            assert not bool(torch.isnan(t).any()), name
        traj = out["rew"][:, 0, 0]
        assert bool((traj >= 0).all()) and bool((traj < 10).all())


def test_fields_of_a_sampled_row_belong_to_one_trajectory():
    rep = FusedDeviceReplay(FIELDS, S, 8, "cpu", seed=9)
    out = rep.push_sample(make(8, 0), 8)
    base = out["rew"][:, 0, 0]
    for name in FIELDS:
        assert torch.equal(out[name][:, 0, 0], base)


def test_output_tensors_keep_their_identity():
    rep = FusedDeviceReplay(FIELDS, S, 16, "cpu")
    a = rep.push_sample(make(8, 0), 4)
    first = {k: v.clone() for k, v in a.items()}
    b = rep.push_sample(make(8, 8), 4)
    assert b is a
    for name in FIELDS:
        assert b[name] is a[name]
    assert any(not torch.equal(first[k], b[k]) for k in FIELDS)  # overwritten
    c = rep.sample(5)  # another size: its own tensors
    assert c is not a and c["obs"].shape[0] == 5
    assert rep.sample(4) is a


def _sequence(seed):
    rep = FusedDeviceReplay(FIELDS, S, 11, "cpu", seed=seed)
    outs = []
    start = 0
    for n in (6, 4, 5):
        out = rep.push_sample(make(n, start), 6)
        start += n
        outs.append(out["rew"][:, 0, 0].clone())
    outs.append(rep.sample(6)["rew"][:, 0, 0].clone())
    return torch.stack(outs)


def test_seed_reproduces_and_distinguishes():
    a, b, c = _sequence(1234), _sequence(1234), _sequence(1235)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert not torch.equal(a[0], a[3])  # the draw counter moves the stream


def test_value_errors():
    with pytest.raises(ValueError, match="capacity"):
        FusedDeviceReplay(FIELDS, S, 2 ** 31, "cpu")
    with pytest.raises(ValueError, match="fields"):
        FusedDeviceReplay({f"f{i}": 1 for i in range(13)}, S, 8, "cpu")
    FusedDeviceReplay({f"f{i}": 1 for i in range(12)}, S, 8, "cpu")
    rep = FusedDeviceReplay(FIELDS, S, 8, "cpu")
    with pytest.raises(ValueError, match="exceeds capacity"):
        rep.append_batch(make(9, 0))
    with pytest.raises(ValueError, match="exceeds capacity"):
        rep.push_sample(make(9, 0), 4)
    assert rep.size == 0


def test_eager_env_var_selects_the_oracle(monkeypatch):
    monkeypatch.setenv("PDRL_REPLAY_EAGER", "1")
    assert FusedDeviceReplay(FIELDS, S, 8, "cpu").eager


# --------------------------------------------------------------------------- #
# learner (oracle path)
# --------------------------------------------------------------------------- #
def _device_params(params, algo):
    params.algo = algo
    params.actor_mode = "device"
    if algo == "SAC":
        params.env = "CartPole-v1"
        params.obs_dim, params.n_actions, params.continuous = 4, 2, False
    else:
        params.env = "MountainCarContinuous-v0"
        params.obs_dim, params.n_actions, params.continuous = 2, 1, True
    return params


@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
@pytest.mark.parametrize("device_envs", [0, 3])
def test_learner_device_mode_fused_replay(params, algo, device_envs):
    from pdrl_amd.agents import Learner

    p = _device_params(params, algo)
    p.replay_kernel = "fused"
    p.device_envs = device_envs  # 3: fewer envs than the batch → warm-up path
    seen = []
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        assert isinstance(lrn.device_replay, FusedDeviceReplay)
        assert lrn.device_replay.eager  # CPU: the oracle path
        assert lrn.device_replay.seed == 1234
        step = lrn.updater.step
        lrn.updater.step = lambda b: seen.append(step(b)) or seen[-1]
        lrn.run(max_updates=3)
        assert lrn.updater.update_count == 3 and len(seen) == 3
        for stats in seen:
            assert all(math.isfinite(float(v)) for v in stats.values())
        rep, n = lrn.device_replay, lrn.device_rollout.N
        assert rep.size >= p.batch_size
        assert rep._draws == 3  # one push_sample launch per update
        warm = max(0, math.ceil(p.batch_size / n) - 1)  # push-only rollouts
        assert rep._head == (warm + 3) * n
    finally:
        lrn.close()


def test_learner_default_keeps_device_replay(params):
    from pdrl_amd.agents import Learner
    from pdrl_amd.utils import load_params

    assert load_params().replay_kernel == "eager"
    p = _device_params(params, "SAC")
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        assert type(lrn.device_replay) is DeviceReplay
    finally:
        lrn.close()


def test_learner_rejects_bad_replay_kernel(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params, "SAC")
    p.replay_kernel = "triton"
    with pytest.raises(ValueError, match="replay_kernel"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")
