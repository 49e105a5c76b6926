"""Device actor: N native environments stepped by the policy on the GPU.

``DeviceRollout.rollout()`` advances ``num_envs`` environments by
``seq_len`` steps — policy forward, categorical sample, log-prob, env
dynamics, termination, auto-reset — and returns the ``(N, S, dim)`` batch in
the learner's own field layout (``buffers.rollout_fields``). On a GPU this is
ONE launch of the HIP kernel ``rollout_discrete`` (csrc/rollout.hip) reading
the core's live weights by pointer; on a CPU device, or with
``PDRL_ROLLOUT_EAGER=1``, the same class runs the pure-torch fp32 reference
below, which is both the CPU fallback and the kernel's oracle.

Random stream (shared with csrc/rollout_rng.h, all uint32):

    wang(s): s=(s^61)^(s>>16); s*=9; s^=s>>4; s*=0x27d4eb2d; s^=s>>15
    h0 = wang(seed ^ (env * 0x9E3779B1))
    h  = wang(h0 ^ wang(tick*8 + k + 0x85ebca6b))
    u(seed, env, tick, k) = float(h >> 8) * 2^-24        # in [0, 1)

Lane k=0 is the action uniform of step ``tick`` (first step ever: tick 1);
lanes 1..4 are the reset state of a reset caused by the step at ``tick``;
the initial state at construction uses tick 0.

Env state is NOT checkpointed: a resumed run starts fresh episodes.
"""
from __future__ import annotations

import os
from collections import deque

import torch

from pdrl_amd.buffers import rollout_fields

_M32 = 0xFFFFFFFF
# "no episode ended at this step" marker in ep_ret (csrc/rollout.hip)
NO_EPISODE = -1.0e30


def _wang(s: torch.Tensor) -> torch.Tensor:
    """uint32 Wang hash on int64 tensors holding values in [0, 2^32)."""
    s = (s ^ 61) ^ (s >> 16)
    s = (s * 9) & _M32
    s = s ^ (s >> 4)
    s = (s * 0x27D4EB2D) & _M32
    s = s ^ (s >> 15)
    return s


def uniform(seed: int, env: torch.Tensor, tick, k: int) -> torch.Tensor:
    """u(seed, env, tick, k) as fp32; ``env`` int64 tensor, ``tick`` an int
    or an int64 tensor broadcastable against it."""
    env = env.to(torch.int64)
    if not torch.is_tensor(tick):
        tick = torch.full_like(env, int(tick))
    h0 = _wang((int(seed) & _M32) ^ ((env * 0x9E3779B1) & _M32))
    ctr = (tick.to(torch.int64) * 8 + int(k) + 0x85EBCA6B) & _M32
    h = _wang(h0 ^ _wang(ctr))
    return (h >> 8).to(torch.float32) * (1.0 / 16777216.0)


# --------------------------------------------------------------------------- #
# Reference env dynamics (fp32 torch; mirrored by the traits structs of
# csrc/rollout.hip). A second native env is one more class here, one more
# struct + case there.
# --------------------------------------------------------------------------- #
class CartPoleDyn:
    """CartPole-v1: constants and Euler update of envs/cartpole.py, fp32."""

    env_id = 0
    obs_dim = 4
    n_actions = 2
    max_episode_steps = 500
    GRAVITY, MASS_POLE, TOTAL_MASS = 9.8, 0.1, 1.1
    LENGTH, POLE_MASS_LENGTH, FORCE_MAG, TAU = 0.5, 0.05, 10.0, 0.02
    THETA_THRESHOLD, X_THRESHOLD = 0.20943951023931953, 2.4

    @staticmethod
    def reset(u: torch.Tensor) -> torch.Tensor:
        """u: (N, 4) uniforms → initial state in [-0.05, 0.05)."""
        return -0.05 + 0.1 * u

    @classmethod
    def step(cls, state: torch.Tensor, action: torch.Tensor):
        """state (N,4) fp32, action (N,) int → (state', reward, terminated)."""
        x, x_dot, theta, theta_dot = state.unbind(1)
        force = torch.where(action == 1, cls.FORCE_MAG, -cls.FORCE_MAG).to(state.dtype)
        cos_t, sin_t = torch.cos(theta), torch.sin(theta)
        temp = (force + cls.POLE_MASS_LENGTH * theta_dot * theta_dot * sin_t) / cls.TOTAL_MASS
        theta_acc = (cls.GRAVITY * sin_t - cos_t * temp) / (
            cls.LENGTH * (4.0 / 3.0 - cls.MASS_POLE * cos_t * cos_t / cls.TOTAL_MASS))
        x_acc = temp - cls.POLE_MASS_LENGTH * theta_acc * cos_t / cls.TOTAL_MASS
        x = x + cls.TAU * x_dot
        x_dot = x_dot + cls.TAU * x_acc
        theta = theta + cls.TAU * theta_dot
        theta_dot = theta_dot + cls.TAU * theta_acc
        terminated = ((x < -cls.X_THRESHOLD) | (x > cls.X_THRESHOLD)
                      | (theta < -cls.THETA_THRESHOLD) | (theta > cls.THETA_THRESHOLD))
        return (torch.stack([x, x_dot, theta, theta_dot], 1),
                torch.ones_like(x), terminated)

    @classmethod
    def threshold_margin(cls, state: torch.Tensor) -> torch.Tensor:
        """Distance of |x| / |θ| from its termination threshold."""
        return torch.minimum((state[:, 0].abs() - cls.X_THRESHOLD).abs(),
                             (state[:, 2].abs() - cls.THETA_THRESHOLD).abs())


DEVICE_ENVS = {"CartPole-v1": CartPoleDyn}


def has_device_env(env_name: str) -> bool:
    return env_name in DEVICE_ENVS


class DeviceRollout:
    """See module docstring. ``core`` is the actor's ``SeqLSTMCore``; its
    parameters are read live on every call (no copies)."""

    STATS_SLOTS = 64  # rollout() calls of ep_ret kept between host reductions

    def __init__(self, core, env_name: str, num_envs: int, seq_len: int,
                 device, seed: int, time_horizon: int,
                 max_episode_steps: int | None = None):
        if env_name not in DEVICE_ENVS:
            raise ValueError(
                f"env {env_name!r} has no device dynamics "
                f"(available: {sorted(DEVICE_ENVS)})")
        self.dyn = dyn = DEVICE_ENVS[env_name]
        if getattr(core, "input2_dim", None) is not None:
            raise ValueError("DeviceRollout does not support dual-body cores")
        if not core.head_names or core.head_names[0] != "logits":
            raise ValueError(
                "DeviceRollout needs a discrete policy core whose first head "
                f"is 'logits' (got heads {core.head_names})")
        if core.hidden not in (32, 64, 128):
            raise ValueError(
                f"hidden size {core.hidden} unsupported (32/64/128)")
        if core.input_dim != dyn.obs_dim or core.head_dims["logits"] != dyn.n_actions:
            raise ValueError(
                f"core shape (obs {core.input_dim}, actions "
                f"{core.head_dims['logits']}) does not match {env_name} "
                f"(obs {dyn.obs_dim}, actions {dyn.n_actions})")
        if num_envs < 1 or seq_len < 1:
            raise ValueError("num_envs and seq_len must be positive")
        self.core = core
        self.device = torch.device(device)
        if core.body_w.device != self.device:
            raise ValueError(
                f"core lives on {core.body_w.device}, rollout on {self.device}")
        self.N, self.S, self.H = int(num_envs), int(seq_len), core.hidden
        self.seed = int(seed) & _M32
        self.time_horizon = int(time_horizon)
        self.max_episode_steps = int(max_episode_steps or dyn.max_episode_steps)
        self.eager = (self.device.type != "cuda"
                      or os.environ.get("PDRL_ROLLOUT_EAGER") == "1")
        if not self.eager:
            from pdrl_amd import ops

            self._ext = ops.ext()  # a missing kernel is an error, not a fallback

        N, S, H, dev = self.N, self.S, self.H, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.fields = rollout_fields(dyn.obs_dim, dyn.n_actions, H, False)
        # the batch: same tensor objects on every call (graph-capturable)
        self.batch = {k: torch.zeros(N, S, d, **f32) for k, d in self.fields.items()}
        # persistent per-env state
        self._env_ids = torch.arange(N, device=dev, dtype=torch.int64)
        u0 = torch.stack([uniform(self.seed, self._env_ids, 0, k)
                          for k in range(1, dyn.obs_dim + 1)], 1)
        self.env_state = dyn.reset(u0).contiguous()
        self.h = torch.zeros(N, H, **f32)
        self.c = torch.zeros(N, H, **f32)
        self.is_fir = torch.ones(N, **f32)
        self.ep_steps = torch.zeros(N, dtype=torch.int32, device=dev)
        self.ep_run = torch.zeros(N, **f32)
        self.tick = torch.zeros(N, dtype=torch.int32, device=dev)
        # reference only: smallest decision margin seen per env (see the
        # parity test) — |u - cdf boundary| and threshold distance
        self.margin = torch.full((N,), float("inf"), **f32)
        # episode returns, one (N, S) slot per call, reduced lazily
        self._ep_ring = torch.full((self.STATS_SLOTS, N, S), NO_EPISODE, **f32)
        self._slot = 0
        self.episodes = 0
        self._last50: deque[float] = deque(maxlen=50)

    # ------------------------------------------------------------------ #
    def _weights(self):
        c = self.core
        return (c.body_w, c.body_b, c.w_ih, c.w_hh, c.b_g, c.heads_w, c.heads_b)

    @torch.no_grad()
    def rollout(self) -> dict[str, torch.Tensor]:
        if self._slot == self.STATS_SLOTS:
            self._drain()
        ep_ret = self._ep_ring[self._slot]
        self._slot += 1
        if self.eager:
            self._rollout_eager(ep_ret)
        else:
            b = self.batch
            self._ext.rollout_discrete(
                *(w.detach() for w in self._weights()),
                self.env_state, self.h, self.c, self.is_fir, self.ep_steps,
                self.ep_run, self.tick, b["obs"], b["act"], b["rew"],
                b["logits"], b["log_prob"], b["is_fir"], b["hx"], b["cx"],
                ep_ret, self.dyn.env_id, self.seed, self.time_horizon,
                self.max_episode_steps)
        return self.batch

    def _rollout_eager(self, ep_ret: torch.Tensor):
        """fp32 torch reference: same hash, op order of
        ``SeqLSTMCore._forward_eager``, same sampling rule and dynamics."""
        dyn, b, A = self.dyn, self.batch, self.dyn.n_actions
        for t in range(self.S):
            self.tick += 1
            b["obs"][:, t] = self.env_state
            b["hx"][:, t] = self.h
            b["cx"][:, t] = self.c
            b["is_fir"][:, t, 0] = self.is_fir
            outs, h, c = self.core._forward_eager(
                self.env_state.unsqueeze(1), self.h, self.c)
            lg = outs["logits"][:, 0]
            # softmax → inverse CDF against one uniform (cpu_actor.cpp rule)
            mx = lg.max(dim=1).values
            prob = torch.exp(lg - mx[:, None])
            Z = prob[:, 0].clone()
            for a in range(1, A):
                Z = Z + prob[:, a]
            u = uniform(self.seed, self._env_ids, self.tick, 0)
            cdf = torch.zeros_like(u)
            act = torch.zeros_like(u, dtype=torch.int64)
            for a in range(A - 1):  # the last action takes the remainder
                cdf = cdf + prob[:, a] / Z
                act += (u >= cdf).to(torch.int64)
                self.margin = torch.minimum(self.margin, (u - cdf).abs())
            log_prob = lg.gather(1, act[:, None])[:, 0] - mx - torch.log(Z)
            state, rew, terminated = dyn.step(self.env_state, act)
            self.margin = torch.minimum(self.margin, dyn.threshold_margin(state))
            self.ep_steps += 1
            self.ep_run += rew
            done = terminated | (self.ep_steps >= self.max_episode_steps)
            reset = done | (self.ep_steps >= self.time_horizon)
            b["act"][:, t, 0] = act.to(torch.float32)
            b["rew"][:, t, 0] = rew
            b["logits"][:, t] = lg
            b["log_prob"][:, t, 0] = log_prob
            ep_ret[:, t] = torch.where(reset, self.ep_run,
                                       torch.full_like(rew, NO_EPISODE))
            fresh = dyn.reset(torch.stack(
                [uniform(self.seed, self._env_ids, self.tick, k)
                 for k in range(1, dyn.obs_dim + 1)], 1))
            keep = (~reset).to(torch.float32)
            self.env_state = torch.where(reset[:, None], fresh, state)
            self.h = h * keep[:, None]
            self.c = c * keep[:, None]
            self.is_fir = reset.to(torch.float32)
            self.ep_steps *= (~reset).to(torch.int32)
            self.ep_run *= keep

    # ------------------------------------------------------------------ #
    def _drain(self):
        """Reduce the ep_ret slots written since the last drain (one D2H
        sync), in time order: call, then step, then env."""
        if self._slot == 0:
            return
        ret = self._ep_ring[: self._slot].transpose(1, 2).reshape(-1).cpu()
        self._slot = 0
        ended = ret[ret > 0.5 * NO_EPISODE].tolist()
        self.episodes += len(ended)
        self._last50.extend(ended)

    def episode_stats(self) -> tuple[int, float]:
        """(episodes finished so far, mean return of the last 50) — the
        manager's 50-episode mean. One host sync; call at a logging cadence."""
        self._drain()
        mean = sum(self._last50) / len(self._last50) if self._last50 else 0.0
        return self.episodes, float(mean)
