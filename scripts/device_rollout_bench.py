"""Device actor mode throughput (env-steps/s), host clock closed by a
synchronize, 50 warm-up calls, timed windows of at least ``--window`` s.

    python scripts/device_rollout_bench.py [--repeats 3] [--window 1.0]

(a) ``rollout()`` alone at N=128 and N=1024 (S=5, H=64);
(b) rollout + IMPALA update in device mode at B=128 — the end-to-end figure
    to hold against ``bench.py --mode staged`` (the path this mode replaces)
    and ``--mode resident`` (the ceiling: no data path at all);
(c) the Gaussian ``rollout()`` alone on MountainCarContinuous-v0, both
    sampling schemes (mode 0 = PPO-C, 1 = SAC-C), at N=128 and N=1024;
(d) rollout + PPO-Continuous update in device mode at B=128;
(e) one greedy ``evaluate()`` call (whole episodes, untrained policy) on
    CartPole-v1 (8 episodes per env) and MountainCarContinuous-v0 (1
    episode of 999 steps) at N=64 and N=1024: ``ms_per_call`` and, since
    the envs run side by side, ``us_per_step`` of the longest env;
(f) the device replay alone, CartPole SAC fields, N = B = 128, capacity
    10240: ``append_batch`` + ``sample`` of ``DeviceReplay``
    (``replay_kernel`` eager) against ``push_sample`` of
    ``FusedDeviceReplay`` (fused); also ``us_per_call``;
(g) rollout + replay + SAC / SAC-Continuous update in device mode at B=128
    (``Learner.next_batch`` + ``updater.step``), once per ``replay_kernel``.
    In (f) and (g) the two paths alternate inside one run.
(h) the envs whose observation is not their state: ``rollout()`` alone at
    N=128 and N=1024 on Acrobot-v1 and on Pendulum-v1 (both Gaussian
    schemes), and one ``evaluate()`` call each (1 episode, N=64).

``--only-replay`` runs (f) and (g) alone.

Prints one JSON line per measurement; ``values`` holds every repeat.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

WARMUP = 50


def timed(fn, window_s: float, steps_per_call: int, chunk: int) -> float:
    """env-steps/s over one window of >= window_s (whole chunks of calls)."""
    torch.cuda.synchronize()
    calls = 0
    t0 = time.perf_counter()
    while True:
        for _ in range(chunk):
            fn()
        calls += chunk
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if el >= window_s:
            return calls * steps_per_call / el


def report(name: str, values: list[float], **cfg):
    print(json.dumps({
        "metric": name, "unit": "env-steps/s",
        "median": sorted(values)[len(values) // 2],
        "min": min(values), "max": max(values), "values": values, **cfg,
    }), flush=True)


def replay_sections(args, dev: str, S: int, H: int):
    """(f) and (g): the off-policy replay, eager ops against the fused
    launch. Both paths are built first and timed alternately, repeat by
    repeat, so drift of the machine hits them alike."""
    import shutil
    import tempfile

    from pdrl_amd.agents import Learner
    from pdrl_amd.buffers import rollout_fields
    from pdrl_amd.buffers.device_replay import DeviceReplay, FusedDeviceReplay
    from pdrl_amd.utils import load_params

    def alternate(fns: dict, steps_per_call: int, chunk: int) -> dict:
        for fn in fns.values():
            for _ in range(WARMUP):
                fn()
        vals = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                vals[k].append(timed(fn, args.window, steps_per_call, chunk))
        return vals

    def us_per_call(values: list[float], steps_per_call: int) -> float:
        return steps_per_call / sorted(values)[len(values) // 2] * 1e6

    # (f) replay alone
    N = B = 128
    fields = rollout_fields(4, 2, H, False)
    torch.manual_seed(0)
    batch = {k: torch.randn(N, S, d, device=dev) for k, d in fields.items()}
    eager = DeviceReplay(fields, S, 10240, dev, seed=1234)
    fused = FusedDeviceReplay(fields, S, 10240, dev, seed=1234)

    def eager_call():
        eager.append_batch(batch)
        eager.sample(B)

    vals = alternate({"eager": eager_call,
                      "fused": lambda: fused.push_sample(batch, B)}, N * S, 200)
    for kernel, v in vals.items():
        report("replay_only", v, replay_kernel=kernel, num_push=N, batch_size=B,
               seq_len=S, hidden=H, capacity=10240,
               us_per_call=us_per_call(v, N * S))

    # (g) rollout + replay + update, device mode, B=128
    for algo, env, dims, cont, name in (
            ("SAC", "CartPole-v1", (4, 2), False, "device_mode_sac"),
            ("SAC-Continuous", "MountainCarContinuous-v0", (2, 1), True,
             "device_mode_sacc")):
        learners = {}
        for kernel in ("eager", "fused"):
            p = load_params()
            p.algo, p.env, p.continuous = algo, env, cont
            p.obs_dim, p.n_actions = dims
            p.batch_size, p.seq_len, p.hidden_size = 128, S, H
            p.actor_mode, p.replay_kernel = "device", kernel
            p.result_dir = tempfile.mkdtemp(prefix="pdrl_bench_")
            torch.manual_seed(1234)
            learners[kernel] = Learner(None, "127.0.0.1", 0, p, device=dev)

        def stepper(lrn):
            return lambda: lrn.updater.step(lrn.next_batch())

        vals = alternate({k: stepper(l) for k, l in learners.items()},
                         128 * S, 100)
        for kernel, v in vals.items():
            report(name, v, replay_kernel=kernel, batch_size=128, seq_len=S,
                   hidden=H, us_per_call=us_per_call(v, 128 * S),
                   replay_size=learners[kernel].device_replay.size)
        for lrn in learners.values():
            lrn.close()
            shutil.rmtree(lrn.params.result_dir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--seq-len", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--only-replay", action="store_true",
                    help="run the replay entries (f) and (g) alone")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "needs a GPU"
    if args.only_replay:
        replay_sections(args, "cuda:0", args.seq_len, args.hidden)
        return
    from pdrl_amd.agents.learner_module import ImpalaUpdater, PPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.networks.models import (MlpLSTMSeperateContinuous,
                                          MlpLSTMSingleContinuous)
    from pdrl_amd.ops.rollout import DeviceRollout
    from pdrl_amd.utils import load_params

    dev, S, H = "cuda:0", args.seq_len, args.hidden

    # (a) rollout alone
    for n_envs in (128, 1024):
        torch.manual_seed(0)
        model = MlpLSTMSingle(4, 2, S, H).to(dev)
        ro = DeviceRollout(model.actor.core, "CartPole-v1", n_envs, S, dev,
                           seed=1, time_horizon=500)
        for _ in range(WARMUP):
            ro.rollout()
        vals = [timed(ro.rollout, args.window, n_envs * S, 200)
                for _ in range(args.repeats)]
        report("rollout_only", vals, num_envs=n_envs, seq_len=S, hidden=H)

    # (b) rollout + IMPALA update, device mode, B=128
    p = load_params()
    p.algo, p.batch_size, p.seq_len, p.hidden_size = "IMPALA", 128, S, H
    p.obs_dim, p.n_actions = 4, 2
    torch.manual_seed(1234)
    model = MlpLSTMSingle(4, 2, S, H)
    upd = ImpalaUpdater(model, p, dev)
    ro = DeviceRollout(upd.model.actor.core, "CartPole-v1", p.batch_size, S,
                       dev, seed=1234, time_horizon=p.time_horizon)

    def step():
        upd.step(ro.rollout())

    for _ in range(WARMUP):
        step()
    vals = [timed(step, args.window, p.batch_size * S, 200)
            for _ in range(args.repeats)]
    games, mean50 = ro.episode_stats()
    report("device_mode_impala", vals, batch_size=p.batch_size, seq_len=S,
           hidden=H, episodes=games, mean50=mean50)

    # (c) Gaussian rollout alone, MountainCarContinuous-v0, both schemes
    cenv = "MountainCarContinuous-v0"
    for mode, cls in ((0, MlpLSTMSingleContinuous), (1, MlpLSTMSeperateContinuous)):
        for n_envs in (128, 1024):
            torch.manual_seed(0)
            model = cls(2, 1, S, H).to(dev)
            ro = DeviceRollout(model.actor.core, cenv, n_envs, S, dev, seed=1,
                               time_horizon=500)
            for _ in range(WARMUP):
                ro.rollout()
            vals = [timed(ro.rollout, args.window, n_envs * S, 200)
                    for _ in range(args.repeats)]
            report("rollout_only", vals, env=cenv, mode=mode, num_envs=n_envs,
                   seq_len=S, hidden=H)

    # (d) rollout + PPO-Continuous update, device mode, B=128
    p = load_params()
    p.algo, p.batch_size, p.seq_len, p.hidden_size = "PPO-Continuous", 128, S, H
    p.env, p.obs_dim, p.n_actions, p.continuous = cenv, 2, 1, True
    torch.manual_seed(1234)
    model = MlpLSTMSingleContinuous(2, 1, S, H)
    upd = PPOUpdater(model, p, dev)
    ro = DeviceRollout(upd.model.actor.core, cenv, p.batch_size, S, dev,
                       seed=1234, time_horizon=p.time_horizon)

    def step_c():
        upd.step(ro.rollout())

    for _ in range(WARMUP):
        step_c()
    vals = [timed(step_c, args.window, p.batch_size * S, 200)
            for _ in range(args.repeats)]
    games, mean50 = ro.episode_stats()
    report("device_mode_ppoc", vals, batch_size=p.batch_size, seq_len=S,
           hidden=H, episodes=games, mean50=mean50)

    # (e) one greedy evaluate() call: whole episodes in one launch. The envs
    # run side by side, so the call lasts as long as its longest env:
    # us_per_step = call time / the largest per-env step count
    from pdrl_amd.ops.evaluate import DeviceEvaluator

    for env, cls, dims, episodes in ((
            "CartPole-v1", MlpLSTMSingle, (4, 2), 8), (
            cenv, MlpLSTMSeperateContinuous, (2, 1), 1)):
        for n_envs in (64, 1024):
            torch.manual_seed(0)
            model = cls(*dims, S, H).to(dev)
            ev = DeviceEvaluator(model.actor.core, env, n_envs, episodes, dev,
                                 seed=4321)
            for _ in range(5):
                ev.evaluate()
            per_env = ev.lengths.sum(1)
            steps, longest = int(per_env.sum()), int(per_env.max())
            vals = [timed(ev.evaluate, args.window, steps, 20)
                    for _ in range(args.repeats)]
            ms = sorted(steps / v * 1e3 for v in vals)[len(vals) // 2]
            report("evaluate_call", vals, env=env, num_envs=n_envs,
                   episodes=episodes, hidden=H, env_steps=steps,
                   longest_env_steps=longest, ms_per_call=ms,
                   us_per_step=ms * 1e3 / longest, **ev.summary())

    # (h) Acrobot-v1 and Pendulum-v1: rollout alone, one evaluate() call
    acro, pen = "Acrobot-v1", "Pendulum-v1"
    for env, mode, cls, dims in ((acro, None, MlpLSTMSingle, (6, 3)),
                                 (pen, 0, MlpLSTMSingleContinuous, (3, 1)),
                                 (pen, 1, MlpLSTMSeperateContinuous, (3, 1))):
        for n_envs in (128, 1024):
            torch.manual_seed(0)
            model = cls(*dims, S, H).to(dev)
            ro = DeviceRollout(model.actor.core, env, n_envs, S, dev, seed=1,
                               time_horizon=500)
            for _ in range(WARMUP):
                ro.rollout()
            vals = [timed(ro.rollout, args.window, n_envs * S, 200)
                    for _ in range(args.repeats)]
            report("rollout_only", vals, env=env, mode=mode, num_envs=n_envs,
                   seq_len=S, hidden=H)
    for env, cls, dims in ((acro, MlpLSTMSingle, (6, 3)),
                           (pen, MlpLSTMSeperateContinuous, (3, 1))):
        torch.manual_seed(0)
        model = cls(*dims, S, H).to(dev)
        ev = DeviceEvaluator(model.actor.core, env, 64, 1, dev, seed=4321)
        for _ in range(5):
            ev.evaluate()
        per_env = ev.lengths.sum(1)
        steps, longest = int(per_env.sum()), int(per_env.max())
        vals = [timed(ev.evaluate, args.window, steps, 20)
                for _ in range(args.repeats)]
        ms = sorted(steps / v * 1e3 for v in vals)[len(vals) // 2]
        report("evaluate_call", vals, env=env, num_envs=64, episodes=1,
               hidden=H, env_steps=steps, longest_env_steps=longest,
               ms_per_call=ms, us_per_step=ms * 1e3 / longest, **ev.summary())

    # (f), (g) the off-policy replay: eager ops against the fused launch
    replay_sections(args, dev, S, H)


if __name__ == "__main__":
    main()
