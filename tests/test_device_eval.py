"""Greedy device evaluation, CPU side: the vectorised eager reference (which
is also the GPU kernels' oracle) against a plain single-env loop, its
invariants, reproducibility and isolation from the training rollout, the
validation errors, the learner integration and the ``evaluate`` CLI role."""
import json
import math

import pytest
import torch

from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.networks.models import (MlpLSTMCriticContinuous,
                                      MlpLSTMSeperateContinuous,
                                      MlpLSTMSingleContinuous)
from pdrl_amd.ops.evaluate import DeviceEvaluator
from pdrl_amd.ops.rollout import (CartPoleDyn, DeviceRollout,
                                  MountainCarContDyn, uniform)

CART, CAR = "CartPole-v1", "MountainCarContinuous-v0"
S, MAX_STEPS = 5, 40


def _switching_cartpole(hidden=64, scale=30.0):
    """An untrained core never changes its arg-max action; scaling the body
    weights and zeroing the head biases makes one that does."""
    torch.manual_seed(0)
    model = MlpLSTMSingle(4, 2, S, hidden)
    with torch.no_grad():
        model.actor.core.body_w *= scale
        model.actor.core.heads_b.zero_()
    return model


def _car_model(cls, hidden=64):
    torch.manual_seed(0)
    return cls(2, 1, S, hidden)


# --------------------------------------------------------------------------- #
# independent oracle: one env at a time, plain Python control flow
# --------------------------------------------------------------------------- #
def _single_env_loop(core, dyn, continuous, seed, n, episodes, max_steps):
    env = torch.tensor([n])
    draws = getattr(dyn, "reset_draws", dyn.obs_dim)
    returns, lengths, forces = [], [], []
    with torch.no_grad():
        for e in range(episodes):
            u = torch.stack([uniform(seed, env, e, k) for k in range(1, draws + 1)], 1)
            state = dyn.reset(u)
            h = torch.zeros(1, core.hidden)
            c = torch.zeros(1, core.hidden)
            ret, length, f2, terminated = torch.zeros(()), 0, 0.0, False
            while not terminated and length < max_steps:
                outs, h, c = core._forward_eager(state.unsqueeze(1), h, c)
                if continuous:
                    act = torch.tanh(outs["mu"][:, 0, 0])
                    f2 += float(act.clamp(-1.0, 1.0)[0]) ** 2
                else:
                    lg = outs["logits"][0, 0]
                    best = 0
                    for a in range(1, lg.shape[0]):
                        if float(lg[a]) > float(lg[best]):
                            best = a
                    act = torch.tensor([best])
                state, rew, term = dyn.step(state, act)
                ret = ret + rew[0]
                length += 1
                terminated = bool(term[0])
            returns.append(float(ret))
            lengths.append(length)
            forces.append((f2, terminated))
    return returns, lengths, forces


@pytest.mark.parametrize("kind", ["cartpole", "car-ppo", "car-sac"])
def test_eager_reference_matches_single_env_loop(kind):
    """3 envs x 2 episodes. Lengths must be equal; returns are fp32 sums of
    the same rewards in the same order, up to batch-1 vs batch-3 GEMM
    rounding (a few ulp of the logits), so 1e-5 absolute."""
    if kind == "cartpole":
        model, env, dyn, cont = _switching_cartpole(), CART, CartPoleDyn, False
    else:
        cls = MlpLSTMSingleContinuous if kind == "car-ppo" else MlpLSTMSeperateContinuous
        model, env, dyn, cont = _car_model(cls), CAR, MountainCarContDyn, True
    core = model.actor.core
    ev = DeviceEvaluator(core, env, 3, 2, "cpu", seed=1, max_episode_steps=MAX_STEPS)
    assert ev.eager
    res = ev.evaluate()
    for n in range(3):
        returns, lengths, _ = _single_env_loop(core, dyn, cont, 1, n, 2, MAX_STEPS)
        assert res["lengths"][n].tolist() == lengths
        assert res["returns"][n].tolist() == pytest.approx(returns, abs=1e-5)
    if kind == "cartpole":  # the policy under test does change its action
        assert int(ev.switches.sum()) > 0
        assert int((res["lengths"] < MAX_STEPS).sum()) > 0


# --------------------------------------------------------------------------- #
# invariants
# --------------------------------------------------------------------------- #
def test_cartpole_invariants():
    ev = DeviceEvaluator(_switching_cartpole().actor.core, CART, 16, 3, "cpu",
                         seed=1, max_episode_steps=MAX_STEPS)
    res = ev.evaluate()
    assert res["returns"].shape == (16, 3) and res["returns"].dtype == torch.float32
    assert res["lengths"].shape == (16, 3) and res["lengths"].dtype == torch.int32
    assert int(res["lengths"].min()) >= 1 and int(res["lengths"].max()) <= MAX_STEPS
    assert torch.equal(res["returns"], res["lengths"].to(torch.float32))
    # both ways of ending an episode occur
    assert int((res["lengths"] < MAX_STEPS).sum()) > 0
    assert int((res["lengths"] == MAX_STEPS).sum()) > 0
    assert bool(torch.isfinite(ev.margin).all())
    s = ev.summary()
    assert s["min_return"] <= s["mean_return"] <= s["max_return"]
    assert s["mean_length"] == pytest.approx(float(res["lengths"].float().mean()))


@pytest.mark.parametrize("cls", [MlpLSTMSingleContinuous, MlpLSTMSeperateContinuous])
def test_mountain_car_invariants(cls):
    """return = -0.1 * sum(force^2) (+ 100 if the episode terminated), with
    the forces of the single-env loop; the first two envs start next to the
    goal and reach it, the third does not."""
    core = _car_model(cls).actor.core
    ev = DeviceEvaluator(core, CAR, 3, 1, "cpu", seed=1, max_episode_steps=MAX_STEPS)
    start = torch.tensor([[0.40, 0.04], [0.44, 0.04], [-0.5, 0.0]])
    res = ev.evaluate(start)
    assert int(res["lengths"].min()) >= 1 and int(res["lengths"].max()) <= MAX_STEPS
    assert res["lengths"][:, 0].tolist()[2] == MAX_STEPS
    assert all(int(v) < MAX_STEPS for v in res["lengths"][:2, 0])
    with torch.no_grad():
        for n in range(3):
            state = start[n:n + 1]
            h = c = torch.zeros(1, core.hidden)
            f2, terminated = 0.0, False
            for _ in range(int(res["lengths"][n, 0])):
                outs, h, c = core._forward_eager(state.unsqueeze(1), h, c)
                act = torch.tanh(outs["mu"][:, 0, 0])
                f2 += float(act.clamp(-1.0, 1.0)[0]) ** 2
                state, _, term = MountainCarContDyn.step(state, act)
                terminated = bool(term[0])
            assert terminated == (n < 2)
            want = -0.1 * f2 + (100.0 if terminated else 0.0)
            assert float(res["returns"][n, 0]) == pytest.approx(want, abs=1e-4)


# --------------------------------------------------------------------------- #
# reproducibility and isolation
# --------------------------------------------------------------------------- #
def test_same_seed_reproduces_and_other_seed_differs():
    core = _switching_cartpole().actor.core
    a = DeviceEvaluator(core, CART, 8, 2, "cpu", seed=1, max_episode_steps=MAX_STEPS)
    b = DeviceEvaluator(core, CART, 8, 2, "cpu", seed=1, max_episode_steps=MAX_STEPS)
    ra = {k: v.clone() for k, v in a.evaluate().items()}
    rb = b.evaluate()
    assert torch.equal(ra["returns"], rb["returns"])
    assert torch.equal(ra["lengths"], rb["lengths"])
    other = DeviceEvaluator(core, CART, 8, 2, "cpu", seed=2, max_episode_steps=MAX_STEPS)
    assert torch.equal(a.start_states(0), b.start_states(0))
    assert not torch.equal(a.start_states(0), other.start_states(0))
    assert not torch.equal(a.start_states(1), other.start_states(1))
    # the stream of episode e is tick e, lanes 1..4, of the evaluator's seed
    want = CartPoleDyn.reset(torch.stack(
        [uniform(1, torch.arange(8), 1, k) for k in range(1, 5)], 1))
    assert torch.equal(a.start_states(1), want)


def test_result_tensors_are_stable_and_repeatable():
    ev = DeviceEvaluator(_switching_cartpole().actor.core, CART, 4, 2, "cpu",
                         seed=3, max_episode_steps=MAX_STEPS)
    first = ev.evaluate()
    snap = {k: v.clone() for k, v in first.items()}
    again = ev.evaluate()
    assert again["returns"] is first["returns"] and again["lengths"] is first["lengths"]
    assert torch.equal(again["returns"], snap["returns"])
    assert torch.equal(again["lengths"], snap["lengths"])


def test_training_rollout_and_evaluation_do_not_disturb_each_other():
    model = _switching_cartpole()
    core = model.actor.core

    def rollout():
        return DeviceRollout(core, CART, 4, S, "cpu", seed=7, time_horizon=500)

    alone = rollout()
    for _ in range(3):
        alone.rollout()

    ev = DeviceEvaluator(core, CART, 4, 2, "cpu", seed=1, max_episode_steps=MAX_STEPS)
    ro = rollout()
    ro.rollout()
    before = {k: v.clone() for k, v in ev.evaluate().items()}
    ro.rollout()
    ro.rollout()
    after = ev.evaluate()
    assert torch.equal(before["returns"], after["returns"])
    assert torch.equal(before["lengths"], after["lengths"])
    # ... and the rollout went on as if no evaluation had happened
    assert torch.equal(ro.tick, alone.tick) and int(ro.tick[0]) == 3 * S
    assert torch.equal(ro.env_state, alone.env_state)
    assert torch.equal(ro.h, alone.h) and torch.equal(ro.c, alone.c)


# --------------------------------------------------------------------------- #
# validation
# --------------------------------------------------------------------------- #
def test_rejects_unsupported_configurations():
    disc = MlpLSTMSingle(4, 2, S, 64).actor.core
    cont = MlpLSTMSingleContinuous(2, 1, S, 64).actor.core
    with pytest.raises(ValueError, match="Gaussian policy core"):
        DeviceEvaluator(MlpLSTMSingle(2, 1, S, 64).actor.core, CAR, 4, 1, "cpu", 0)
    with pytest.raises(ValueError, match="first head"):
        DeviceEvaluator(MlpLSTMSingleContinuous(4, 2, S, 64).actor.core, CART,
                        4, 1, "cpu", 0)
    with pytest.raises(ValueError, match="episodes must be positive"):
        DeviceEvaluator(disc, CART, 4, 0, "cpu", 0)
    with pytest.raises(ValueError, match="step loop bound"):
        DeviceEvaluator(disc, CART, 4, 8390, "cpu", 0)  # 8390 * 500 > 2^22
    with pytest.raises(ValueError, match="step loop bound"):
        DeviceEvaluator(cont, CAR, 4, 2, "cpu", 0, max_episode_steps=(1 << 21) + 1)
    with pytest.raises(ValueError, match="dual-body"):
        DeviceEvaluator(MlpLSTMCriticContinuous(4, 2, S, 64).core, CART, 4, 1,
                        "cpu", 0)
    with pytest.raises(ValueError, match="no device dynamics"):
        DeviceEvaluator(disc, "MountainCar-v0", 4, 1, "cpu", 0)
    with pytest.raises(ValueError, match="hidden size"):
        DeviceEvaluator(MlpLSTMSingle(4, 2, S, 48).actor.core, CART, 4, 1, "cpu", 0)
    ev = DeviceEvaluator(disc, CART, 4, 1, "cpu", 0)  # 8388 * 500 fits
    assert DeviceEvaluator(disc, CART, 1, 8388, "cpu", 0).E == 8388
    with pytest.raises(ValueError, match="start_state"):
        ev.evaluate(torch.zeros(3, 4))


# --------------------------------------------------------------------------- #
# learner
# --------------------------------------------------------------------------- #
def _device_params(params, algo="IMPALA"):
    params.algo, params.env = algo, CART
    params.obs_dim, params.n_actions, params.continuous = 4, 2, False
    params.actor_mode = "device"
    params.model_save_interval = 10_000
    params.eval_envs, params.eval_episodes, params.eval_seed = 4, 1, 4321
    return params


def test_learner_evaluates_every_interval(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params)
    p.eval_interval = 2
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        assert lrn.evaluator is not None and lrn.last_eval is None
        assert (lrn.evaluator.N, lrn.evaluator.E) == (4, 1)
        lrn.run(max_updates=1)
        assert lrn.last_eval is None
        lrn.run(max_updates=2)
        assert lrn.last_eval is not None and lrn.last_eval["update"] == 2
        for k in ("mean_return", "min_return", "max_return", "mean_length"):
            assert math.isfinite(lrn.last_eval[k]), k
        assert 1.0 <= lrn.last_eval["mean_return"] <= 500.0
        # evaluation consumed no training ticks
        assert int(lrn.device_rollout.tick[0]) == 2 * p.seq_len
        lrn.writer.flush()
    finally:
        lrn.close()
    tags = [json.loads(line)["tag"] for line in
            open(f"{p.result_dir}/scalars.jsonl").read().splitlines()]
    for tag in ("eval-mean-return", "eval-min-return", "eval-mean-length"):
        assert tags.count(tag) == 1, tag


def test_learner_without_interval_builds_no_evaluator(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params)
    assert p.eval_interval == 0  # the default of parameters.json
    lrn = Learner(None, "127.0.0.1", 0, p, device="cpu")
    try:
        assert lrn.evaluator is None
        lrn.run(max_updates=2)
        assert lrn.last_eval is None
    finally:
        lrn.close()


def test_learner_evaluates_in_workers_mode(params):
    """The evaluator needs only the env's device dynamics and the actor core,
    not the device actor: a workers-mode learner fed from elsewhere (here a
    synthetic batch in place of the ring) evaluates too."""
    import socket

    from pdrl_amd.agents import Learner
    from pdrl_amd.buffers import SharedRolloutRing, rollout_fields
    from tests.conftest import make_batch

    p = _device_params(params, "PPO")
    p.actor_mode = "workers"
    p.eval_interval = 1
    fields = rollout_fields(p.obs_dim, p.n_actions, p.hidden_size, False)
    ring = SharedRolloutRing(fields, p.seq_len, p.batch_size, True)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    lrn = Learner(ring, "127.0.0.1", port - 1, p, device="cpu")  # PUB on port
    try:
        assert lrn.device_rollout is None and lrn.evaluator is not None
        lrn.next_batch = lambda timeout=30.0: make_batch(p)
        lrn.run(max_updates=1)
        assert lrn.last_eval["update"] == 1
        assert 1.0 <= lrn.last_eval["mean_return"] <= 500.0
    finally:
        lrn.close()


def test_learner_rejects_evaluation_it_cannot_do(params):
    from pdrl_amd.agents import Learner

    p = _device_params(params, "PPO")
    p.eval_interval = 5
    p.env, p.obs_dim, p.n_actions = "MountainCar-v0", 2, 3
    p.actor_mode = "workers"
    with pytest.raises(ValueError, match="eval_interval.*no device dynamics"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")
    p = _device_params(params, "PPO")
    p.eval_interval = 5
    p.env, p.obs_dim, p.n_actions = CAR, 2, 1
    p.actor_mode = "workers"
    with pytest.raises(ValueError, match="eval_interval.*continuous policies only"):
        Learner(None, "127.0.0.1", 0, p, device="cpu")


# --------------------------------------------------------------------------- #
# CLI
# --------------------------------------------------------------------------- #
def test_main_evaluate_role_prints_json(params, monkeypatch, capsys, tmp_path):
    import main as main_mod
    from pdrl_amd.agents.learner_module import switch_module

    p = params
    p.algo, p.env = "IMPALA", CART
    p.obs_dim, p.n_actions, p.continuous = 4, 2, False
    p.eval_envs, p.eval_episodes, p.eval_seed = 3, 2, 4321
    upd_cls, model_cls = switch_module("IMPALA")
    torch.manual_seed(0)
    upd = upd_cls(model_cls(4, 2, p.seq_len, p.hidden_size), p, "cpu")
    (tmp_path / "models").mkdir()
    p.model_dir = str(tmp_path / "models")
    ckpt = tmp_path / "models" / "IMPALA_7.pt"
    upd.save(ckpt)

    monkeypatch.setattr(main_mod, "Params", p)
    assert "evaluate" in main_mod.fn_dict
    for args in ((str(ckpt),), ()):  # explicit path; newest in model_dir
        main_mod.fn_dict["evaluate"](*args)
        line = capsys.readouterr().out.strip().splitlines()[-1]
        rec = json.loads(line)
        assert rec["algo"] == "IMPALA" and rec["env"] == CART
        assert rec["checkpoint"] == str(ckpt)
        assert rec["envs"] == 3 and rec["episodes"] == 2
        assert rec["min_return"] <= rec["mean_return"] <= rec["max_return"]
        assert 1.0 <= rec["mean_length"] <= 500.0
        assert rec["mean_return"] == rec["mean_length"]  # CartPole: 1 per step

    # the line is the evaluator's own result for the checkpoint's weights
    ev = DeviceEvaluator(upd.model.actor.core, CART, 3, 2, "cpu", seed=4321)
    ev.evaluate()
    assert rec["mean_return"] == pytest.approx(ev.summary()["mean_return"])
