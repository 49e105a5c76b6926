"""Greedy device evaluation: whole episodes of the deterministic policy.

``DeviceEvaluator.evaluate()`` runs ``episodes`` episodes in each of
``num_envs`` native environments under the greedy action and returns one
return and one length per (env, episode). On a GPU this is ONE launch of
``rollout_eval_discrete`` / ``rollout_eval_gaussian`` (csrc/rollout.hip)
reading the core's live weights by pointer; on a CPU device, or with
``PDRL_ROLLOUT_EAGER=1``, the same class runs the pure-torch fp32 reference
below, which is both the CPU path and the kernels' oracle.

It is the training rollout (ops/rollout.py) minus everything a batch needs:

    action     discrete: arg-max logit, lowest index on ties
               Gaussian: tanh(mu) — the mean of PPO-C's Normal(tanh(mu), ·)
               and the zero-noise action of SAC-C's squashed Gaussian
    episodes   episode e of env n starts from ``Dyn.reset`` of
               u(seed, n, tick = e, lanes 1..draws) with h = c = 0, and ends
               on ``terminated`` or at ``max_episode_steps``
               (``time_horizon`` plays no part)
    state      none: the start states are a pure function of (seed, n, e),
               so every call measures the same episodes, and nothing of a
               training ``DeviceRollout`` (envs, ticks, replay) is touched

``evaluate(start_state)`` may replace the start of episode 0 by a given
``(N, state_dim)`` state (the env's state vector, which
``Dyn.observe`` turns into the policy's observation; for CartPole and
MountainCar the two are the same).
"""
from __future__ import annotations

import os

import torch

from pdrl_amd.ops.rollout import (DEVICE_ENVS, _M32, DeviceRollout,
                                  is_continuous_env, uniform)

# bound of the kernels' step loop (csrc/rollout.hip::kEvalMaxIters)
MAX_ITERS = 1 << 22


class DeviceEvaluator:
    """See module docstring. ``core`` is the actor's ``SeqLSTMCore``; its
    parameters are read live on every call (no copies)."""

    def __init__(self, core, env_name: str, num_envs: int, episodes: int,
                 device, seed: int, max_episode_steps: int | None = None):
        if env_name not in DEVICE_ENVS:
            raise ValueError(
                f"env {env_name!r} has no device dynamics "
                f"(available: {sorted(DEVICE_ENVS)})")
        self.dyn = dyn = DEVICE_ENVS[env_name]
        self.continuous = is_continuous_env(env_name)
        if getattr(core, "input2_dim", None) is not None:
            raise ValueError("DeviceEvaluator does not support dual-body cores")
        # the policy kind, shapes and H are held to DeviceRollout's own rules
        if self.continuous:
            DeviceRollout._check_gaussian_core(self, core, env_name)
        else:
            DeviceRollout._check_discrete_core(self, core, env_name)
        if num_envs < 1:
            raise ValueError("num_envs must be positive")
        if episodes < 1:
            raise ValueError("episodes must be positive")
        self.max_episode_steps = int(max_episode_steps or dyn.max_episode_steps)
        if self.max_episode_steps < 1:
            raise ValueError("max_episode_steps must be positive")
        if int(episodes) * self.max_episode_steps > MAX_ITERS:
            raise ValueError(
                f"episodes * max_episode_steps = {int(episodes)} * "
                f"{self.max_episode_steps} exceeds the step loop bound "
                f"{MAX_ITERS}")
        self.core = core
        self.device = torch.device(device)
        if core.body_w.device != self.device:
            raise ValueError(
                f"core lives on {core.body_w.device}, evaluator on {self.device}")
        self.N, self.E, self.H = int(num_envs), int(episodes), core.hidden
        self.seed = int(seed) & _M32
        self.eager = (self.device.type != "cuda"
                      or os.environ.get("PDRL_ROLLOUT_EAGER") == "1")
        if not self.eager:
            from pdrl_amd import ops

            self._ext = ops.ext()  # a missing kernel is an error, not a fallback

        dev = self.device
        self._env_ids = torch.arange(self.N, device=dev, dtype=torch.int64)
        # the result: same tensor objects on every call
        self.returns = torch.zeros(self.N, self.E, dtype=torch.float32, device=dev)
        self.lengths = torch.zeros(self.N, self.E, dtype=torch.int32, device=dev)
        self.result = {"returns": self.returns, "lengths": self.lengths}
        # reference only: smallest decision margin seen per env over the live
        # steps of the last call (see the GPU parity test)
        self.margin = torch.full((self.N,), float("inf"), dtype=torch.float32,
                                 device=dev)
        # reference only, discrete policies: steps per env whose action
        # differs from the previous step's of the same episode
        self.switches = torch.zeros(self.N, dtype=torch.int64, device=dev)

    # ------------------------------------------------------------------ #
    def _reset_uniforms(self, tick) -> torch.Tensor:
        """(N, draws) uniforms of the start state of episode ``tick``."""
        draws = getattr(self.dyn, "reset_draws", self.dyn.state_dim)
        return torch.stack([uniform(self.seed, self._env_ids, tick, k)
                            for k in range(1, draws + 1)], 1)

    def start_states(self, episode: int = 0) -> torch.Tensor:
        """(N, state_dim) start states of ``episode`` (no policy involved)."""
        return self.dyn.reset(self._reset_uniforms(int(episode)))

    @torch.no_grad()
    def evaluate(self, start_state: torch.Tensor | None = None
                 ) -> dict[str, torch.Tensor]:
        if start_state is not None and tuple(start_state.shape) != (
                self.N, self.dyn.state_dim):
            raise ValueError(
                f"start_state must be ({self.N}, {self.dyn.state_dim}), got "
                f"{tuple(start_state.shape)}")
        if self.eager:
            self._evaluate_eager(start_state)
        else:
            c = self.core
            fn = (self._ext.rollout_eval_gaussian if self.continuous
                  else self._ext.rollout_eval_discrete)
            fn(*(w.detach() for w in (c.body_w, c.body_b, c.w_ih, c.w_hh,
                                      c.b_g, c.heads_w, c.heads_b)),
               self.returns, self.lengths, start_state, self.dyn.env_id,
               self.seed, self.max_episode_steps)
        return self.result

    def _greedy(self, state, h, c):
        """One policy step: (action, next h, next c, action margin)."""
        outs, h, c = self.core._forward_eager(
            self.dyn.observe(state).unsqueeze(1), h, c)
        if self.continuous:
            act = torch.tanh(outs["mu"][:, 0, 0])
            return act, h, c, torch.full_like(act, float("inf"))
        lg = outs["logits"][:, 0]
        # strict > scan from action 0: ties go to the lowest index
        best = lg[:, 0]
        act = torch.zeros_like(self._env_ids)
        for a in range(1, lg.shape[1]):
            better = lg[:, a] > best
            act = torch.where(better, torch.full_like(act, a), act)
            best = torch.where(better, lg[:, a], best)
        top2 = lg.topk(2, dim=1).values
        return act, h, c, top2[:, 0] - top2[:, 1]

    def _evaluate_eager(self, start_state):
        """fp32 torch reference of the evaluation kernels: the same hash, op
        order of ``SeqLSTMCore._forward_eager``, the ``*Dyn`` dynamics.
        ``margin`` keeps, per env, the smallest top-1 minus top-2 logit and
        threshold distance over the env's live steps: below it one float
        rounding can change the trajectory."""
        dyn, N, E = self.dyn, self.N, self.E
        dev = self.device
        state = (start_state.to(dev, torch.float32) if start_state is not None
                 else self.start_states(0))
        h = torch.zeros(N, self.H, dtype=torch.float32, device=dev)
        c = torch.zeros_like(h)
        episode = torch.zeros(N, dtype=torch.int64, device=dev)
        steps = torch.zeros(N, dtype=torch.int32, device=dev)
        run = torch.zeros(N, dtype=torch.float32, device=dev)
        self.returns.zero_()
        self.lengths.zero_()
        self.margin.fill_(float("inf"))
        self.switches.zero_()
        prev = torch.full_like(episode, -1)  # previous action of the episode
        for _ in range(E * self.max_episode_steps):
            alive = episode < E
            if not bool(alive.any()):
                break
            act, h, c, m = self._greedy(state, h, c)
            if self.continuous:
                m = torch.minimum(m, dyn.threshold_margin(state, act))
                nxt, rew, terminated = dyn.step(state, act)
            else:
                nxt, rew, terminated = dyn.step(state, act)
                m = torch.minimum(m, dyn.threshold_margin(nxt))
                self.switches += (alive & (prev >= 0) & (act != prev)).to(torch.int64)
                prev = act
            self.margin = torch.where(alive, torch.minimum(self.margin, m),
                                      self.margin)
            steps = steps + 1
            run = run + rew
            done = alive & (terminated | (steps >= self.max_episode_steps))
            idx = done.nonzero()[:, 0]
            self.returns[idx, episode[idx]] = run[idx]
            self.lengths[idx, episode[idx]] = steps[idx]
            episode = episode + done.to(torch.int64)
            fresh = dyn.reset(self._reset_uniforms(episode))
            keep = (~done).to(torch.float32)
            state = torch.where(done[:, None], fresh, nxt)
            h = h * keep[:, None]
            c = c * keep[:, None]
            steps = steps * (~done).to(torch.int32)
            run = run * keep
            prev = torch.where(done, torch.full_like(prev, -1), prev)

    # ------------------------------------------------------------------ #
    def summary(self) -> dict[str, float]:
        """Mean / min / max return and mean length of the last call, over
        all (env, episode) pairs. One D2H."""
        packed = torch.stack([self.returns.mean(), self.returns.min(),
                              self.returns.max(),
                              self.lengths.to(torch.float32).mean()]).cpu()
        mean, lo, hi, length = packed.tolist()
        return {"mean_return": mean, "min_return": lo, "max_return": hi,
                "mean_length": length}
