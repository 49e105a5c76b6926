"""Device actor: N native environments stepped by the policy on the GPU.

``DeviceRollout.rollout()`` advances ``num_envs`` environments by
``seq_len`` steps — policy forward, sample, log-prob, env dynamics,
termination, auto-reset — and returns the ``(N, S, dim)`` batch in the
learner's own field layout (``buffers.rollout_fields``). On a GPU this is ONE
launch of a HIP kernel of csrc/rollout.hip reading the core's live weights by
pointer — ``rollout_discrete`` (categorical policy) or ``rollout_gaussian``
(continuous control), chosen by the env's dynamics class; on a CPU device, or
with ``PDRL_ROLLOUT_EAGER=1``, the same class runs the pure-torch fp32
reference below, which is both the CPU fallback and the kernels' oracle.

Random stream (shared with csrc/rollout_rng.h, all uint32):

    wang(s): s=(s^61)^(s>>16); s*=9; s^=s>>4; s*=0x27d4eb2d; s^=s>>15
    h0 = wang(seed ^ (env * 0x9E3779B1))
    h  = wang(h0 ^ wang(tick*8 + k + 0x85ebca6b))
    u(seed, env, tick, k) = float(h >> 8) * 2^-24        # in [0, 1)

Eight lanes per (env, tick). Lane k=0 is the categorical action uniform of
step ``tick`` (first step ever: tick 1; unused by Gaussian policies); lanes
1..4 are the reset state of a reset caused by the step at ``tick``; lanes 5
and 6 are the radius and the angle of a Gaussian policy's one standard normal

    n(seed, env, tick) = sqrt(-2 * log(1 - u5)) * cos(6.2831855 * u6)

(``1 - u5`` is exact in fp32 and never 0); lane 7 is free here (the fused
device replay draws its slots from it under a salted seed:
buffers/device_replay.py). The initial state
at construction uses tick 0. One normal per tick means one action dimension:
more need a wider counter.

Gaussian policies (heads ``mu`` then ``std`` | ``log_std``; the schemes of
cpu_actor.cpp::act_batch_gaussian; ``logits`` is ``[mu_raw | second_raw]``):

    mode 0 (PPO-C, std):   mean = tanh(mu); sd = softplus(s) + 1e-4
                           act = mean + sd*n            (stored unclipped)
                           lp  = -0.5*n*n - log(sd) - 0.9189385
    mode 1 (SAC-C, log_std): ls = clamp(s, -20, 2); sd = exp(ls)
                           z = mu + sd*n; act = tanh(z)
                           lp  = -0.5*n*n - ls - 0.9189385 - log(1 - act² + 1e-7)
    OU exploration (mode 1; env i at a step with i < ou_envs or
    tick <= warmup_steps; ``ou_state`` is zeroed on every reset):
                           ou = ou - theta*ou + sigma*n; z = ou; act = tanh(z)
                           lp  = -0.5*((z-mu)/sd)² - ls - 0.9189385
                                 - log(1 - act² + 1e-7)

Env state is NOT checkpointed: a resumed run starts fresh episodes.

Greedy evaluation of the same cores on the same dynamics — whole episodes,
deterministic action, no batch — is the sibling ops/evaluate.py.
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


def hash_bits(seed: int, env: torch.Tensor, tick, k: int) -> torch.Tensor:
    """The raw 32 bits h(seed, env, tick, k) (csrc/rollout_rng.h::bits) as
    int64 values in [0, 2^32); ``env`` int64 tensor, ``tick`` an int or an
    int64 tensor broadcastable against it. The counter ``tick*8 + k`` is
    uint32, so it wraps after 2^29 ticks."""
    env = env.to(torch.int64)
    if not torch.is_tensor(tick):
        tick = torch.full_like(env, int(tick))
    h0 = _wang((int(seed) & _M32) ^ ((env * 0x9E3779B1) & _M32))
    ctr = (tick.to(torch.int64) * 8 + int(k) + 0x85EBCA6B) & _M32
    return _wang(h0 ^ _wang(ctr))


def uniform(seed: int, env: torch.Tensor, tick, k: int) -> torch.Tensor:
    """u(seed, env, tick, k) as fp32; arguments as ``hash_bits``."""
    h = hash_bits(seed, env, tick, k)
    return (h >> 8).to(torch.float32) * (1.0 / 16777216.0)


# --------------------------------------------------------------------------- #
# Reference env dynamics (fp32 torch; mirrored by the traits structs of
# csrc/rollout.hip). A further native env is one more class here, one more
# struct + case there. Every class has ``state_dim`` and ``observe(state)``:
# ``env_state`` is (N, state_dim), the batch's ``obs`` and the core's input
# are ``observe(env_state)`` (obs_dim wide). For CartPole and MountainCar the
# two are the same and ``observe`` is the identity.
# --------------------------------------------------------------------------- #
class CartPoleDyn:
    """CartPole-v1: constants and Euler update of envs/cartpole.py, fp32."""

    env_id = 0
    obs_dim = state_dim = 4
    n_actions = 2
    max_episode_steps = 500
    GRAVITY, MASS_POLE, TOTAL_MASS = 9.8, 0.1, 1.1
    LENGTH, POLE_MASS_LENGTH, FORCE_MAG, TAU = 0.5, 0.05, 10.0, 0.02
    THETA_THRESHOLD, X_THRESHOLD = 0.20943951023931953, 2.4

    @staticmethod
    def observe(state: torch.Tensor) -> torch.Tensor:
        return state

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


class MountainCarContDyn:
    """MountainCarContinuous-v0: constants and update of
    envs/mountain_car.py, fp32. A continuous-action env: ``act_dim`` instead
    of ``n_actions``, ``step`` takes a float action, and the reset draws
    hash lane 1 only."""

    env_id = 1
    obs_dim = state_dim = 2
    act_dim = 1
    reset_draws = 1
    max_episode_steps = 999
    MIN_POSITION, MAX_POSITION, MAX_SPEED = -1.2, 0.6, 0.07
    GOAL_POSITION, GOAL_VELOCITY, POWER = 0.45, 0.0, 0.0015

    @staticmethod
    def observe(state: torch.Tensor) -> torch.Tensor:
        return state

    @staticmethod
    def reset(u: torch.Tensor) -> torch.Tensor:
        """u: (N, 1) uniforms → (pos in [-0.6, -0.4), vel 0)."""
        pos = -0.6 + 0.2 * u[:, 0]
        return torch.stack([pos, torch.zeros_like(pos)], 1)

    @classmethod
    def _advance(cls, state: torch.Tensor, action: torch.Tensor):
        pos, vel = state.unbind(1)
        force = action.clamp(-1.0, 1.0)
        vel = (vel + (force * cls.POWER - 0.0025 * torch.cos(3 * pos))).clamp(
            -cls.MAX_SPEED, cls.MAX_SPEED)
        raw = pos + vel
        pos = raw.clamp(cls.MIN_POSITION, cls.MAX_POSITION)
        vel = torch.where((pos <= cls.MIN_POSITION) & (vel < 0),
                          torch.zeros_like(vel), vel)
        return force, raw, pos, vel

    @classmethod
    def step(cls, state: torch.Tensor, action: torch.Tensor):
        """state (N,2) fp32, action (N,) fp32 → (state', reward, terminated)."""
        force, _, pos, vel = cls._advance(state, action)
        terminated = (pos >= cls.GOAL_POSITION) & (vel >= cls.GOAL_VELOCITY)
        reward = -0.1 * force * force + torch.where(terminated, 100.0, 0.0).to(state.dtype)
        return torch.stack([pos, vel], 1), reward, terminated

    @classmethod
    def threshold_margin(cls, state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        """Smallest distance, over the step from PRE-step ``state`` under
        ``action``, to a place where one float rounding changes the
        trajectory discontinuously: the unclamped position from the left
        wall (velocity zeroing), the position from the goal, and the
        velocity from 0 once past the goal. The clamps are continuous."""
        _, raw, pos, vel = cls._advance(state, action)
        margin = torch.minimum((raw - cls.MIN_POSITION).abs(),
                               (pos - cls.GOAL_POSITION).abs())
        past_goal = pos >= cls.GOAL_POSITION
        return torch.where(past_goal, torch.minimum(margin, vel.abs()), margin)


PI, TWO_PI = 3.1415927, 6.2831855  # as fp32 rounds them


def wrap_angle(x: torch.Tensor) -> torch.Tensor:
    """x modulo 2π into [-π, π): ``x - 2π·floor((x + π) / 2π)`` on both
    sides, so neither calls a library remainder."""
    return x - TWO_PI * torch.floor((x + PI) / TWO_PI)


class AcrobotDyn:
    """Acrobot-v1: constants, "book" equations of motion and RK4 step of
    envs/acrobot.py, fp32, with the unit masses and lengths folded in. The
    first env whose observation is not its state: ``state_dim`` values
    (θ1, θ2, θ̇1, θ̇2) are carried, ``observe`` turns them into the
    ``obs_dim`` values the policy and the batch see."""

    env_id = 2
    obs_dim = 6
    state_dim = 4
    n_actions = 3
    reset_draws = 4
    max_episode_steps = 500
    DT = 0.2
    MAX_VEL_1, MAX_VEL_2 = 4 * 3.141592653589793, 9 * 3.141592653589793

    @staticmethod
    def observe(state: torch.Tensor) -> torch.Tensor:
        t1, t2, d1, d2 = state.unbind(1)
        return torch.stack([torch.cos(t1), torch.sin(t1), torch.cos(t2),
                            torch.sin(t2), d1, d2], 1)

    @staticmethod
    def reset(u: torch.Tensor) -> torch.Tensor:
        """u: (N, 4) uniforms → all four in [-0.1, 0.1)."""
        return -0.1 + 0.2 * u

    @staticmethod
    def _derivs(t1, t2, v1, v2, torque):
        """(θ̈1, θ̈2); m1 = m2 = l1 = 1, lc = 0.5, I = 1, g = 9.8 folded in:
        d1 = 3.5 + cos θ2, d2 = 1.25 + 0.5 cos θ2, cos(x - π/2) = sin x."""
        c2, s2 = torch.cos(t2), torch.sin(t2)
        d1 = 3.5 + c2
        d2 = 1.25 + 0.5 * c2
        phi2 = 4.9 * torch.sin(t1 + t2)
        phi1 = -0.5 * v2 * v2 * s2 - v2 * v1 * s2 + 14.7 * torch.sin(t1) + phi2
        a2 = ((torque + d2 / d1 * phi1 - 0.5 * v1 * v1 * s2 - phi2)
              / (1.25 - d2 * d2 / d1))
        a1 = -(d2 * a2 + phi1) / d1
        return a1, a2

    @staticmethod
    def height(state: torch.Tensor) -> torch.Tensor:
        """Tip height above the bar; the episode terminates above 1."""
        return -torch.cos(state[:, 0]) - torch.cos(state[:, 0] + state[:, 1])

    @classmethod
    def step(cls, state: torch.Tensor, action: torch.Tensor):
        """state (N,4) fp32, action (N,) int → (state', reward, terminated)."""
        t1, t2, v1, v2 = state.unbind(1)
        torque = action.to(state.dtype) - 1.0
        dt, half = cls.DT, 0.5 * cls.DT
        k1a, k1b = cls._derivs(t1, t2, v1, v2, torque)
        x1, x2 = v1 + half * k1a, v2 + half * k1b
        k2a, k2b = cls._derivs(t1 + half * v1, t2 + half * v2, x1, x2, torque)
        y1, y2 = v1 + half * k2a, v2 + half * k2b
        k3a, k3b = cls._derivs(t1 + half * x1, t2 + half * x2, y1, y2, torque)
        z1, z2 = v1 + dt * k3a, v2 + dt * k3b
        k4a, k4b = cls._derivs(t1 + dt * y1, t2 + dt * y2, z1, z2, torque)
        sixth = dt / 6.0
        t1 = wrap_angle(t1 + sixth * (v1 + 2.0 * x1 + 2.0 * y1 + z1))
        t2 = wrap_angle(t2 + sixth * (v2 + 2.0 * x2 + 2.0 * y2 + z2))
        v1 = (v1 + sixth * (k1a + 2.0 * k2a + 2.0 * k3a + k4a)).clamp(
            -cls.MAX_VEL_1, cls.MAX_VEL_1)
        v2 = (v2 + sixth * (k1b + 2.0 * k2b + 2.0 * k3b + k4b)).clamp(
            -cls.MAX_VEL_2, cls.MAX_VEL_2)
        state = torch.stack([t1, t2, v1, v2], 1)
        terminated = cls.height(state) > 1.0
        reward = torch.where(terminated, 0.0, -1.0).to(state.dtype)
        return state, reward, terminated

    @classmethod
    def threshold_margin(cls, state: torch.Tensor) -> torch.Tensor:
        """Distance of the tip height from its termination threshold. The
        wrap needs no term: a flip moves θ by 2π, which neither the
        observation nor the dynamics (sin / cos of θ only) can see — hence
        ``obs``, never ``env_state``, is what two implementations share."""
        return (cls.height(state) - 1.0).abs()


class PendulumDyn:
    """Pendulum-v1 with the normalised action of envs/pendulum.py (torque
    u = 2·clip(a, -1, 1)), fp32. State (θ, θ̇) with θ never wrapped, obs
    (cos θ, sin θ, θ̇). g = 10, m = l = 1, dt = 0.05 folded in: the
    action-independent part of the speed update is 15·sin θ·dt."""

    env_id = 3
    obs_dim = 3
    state_dim = 2
    act_dim = 1
    reset_draws = 2
    max_episode_steps = 200
    MAX_SPEED = 8.0

    @staticmethod
    def observe(state: torch.Tensor) -> torch.Tensor:
        th, thd = state.unbind(1)
        return torch.stack([torch.cos(th), torch.sin(th), thd], 1)

    @staticmethod
    def reset(u: torch.Tensor) -> torch.Tensor:
        """u: (N, 2) uniforms → θ in [-π, π), θ̇ in [-1, 1)."""
        return torch.stack([-PI + TWO_PI * u[:, 0], -1.0 + 2.0 * u[:, 1]], 1)

    @classmethod
    def step(cls, state: torch.Tensor, action: torch.Tensor):
        """state (N,2) fp32, action (N,) fp32 → (state', reward, False)."""
        th, thd = state.unbind(1)
        u = 2.0 * action.clamp(-1.0, 1.0)
        w = wrap_angle(th)
        cost = w * w + 0.1 * thd * thd + 0.001 * u * u
        drift = 0.75 * torch.sin(th)
        thd = (thd + (drift + 0.15 * u)).clamp(-cls.MAX_SPEED, cls.MAX_SPEED)
        th = th + 0.05 * thd
        return (torch.stack([th, thd], 1), -cost,
                torch.zeros_like(th, dtype=torch.bool))

    @staticmethod
    def threshold_margin(state: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
        """No discontinuity anywhere: the clips are continuous and wrap(θ)²
        is continuous at ±π, so no env is ever excluded."""
        return torch.full_like(state[:, 0], float("inf"))


DEVICE_ENVS = {"CartPole-v1": CartPoleDyn,
               "MountainCarContinuous-v0": MountainCarContDyn,
               "Acrobot-v1": AcrobotDyn,
               "Pendulum-v1": PendulumDyn}
# head names[:2] → sampling scheme of a Gaussian policy (as the worker chooses)
GAUSSIAN_MODES = {("mu", "std"): 0, ("mu", "log_std"): 1}
HALF_LOG_2PI = 0.9189385


def is_continuous_env(env_name: str) -> bool:
    """True when the env has device dynamics with a continuous action."""
    return hasattr(DEVICE_ENVS.get(env_name), "act_dim")


def normal(seed: int, env: torch.Tensor, tick) -> torch.Tensor:
    """The standard normal of (env, tick): Box-Muller on hash lanes 5 / 6."""
    u5 = uniform(seed, env, tick, 5)
    u6 = uniform(seed, env, tick, 6)
    return torch.sqrt(-2.0 * torch.log(1.0 - u5)) * torch.cos(6.2831855 * u6)


def has_device_env(env_name: str) -> bool:
    return env_name in DEVICE_ENVS


class DeviceRollout:
    """See module docstring. ``core`` is the actor's ``SeqLSTMCore``; its
    parameters are read live on every call (no copies)."""

    STATS_SLOTS = 64  # rollout() calls of ep_ret kept between host reductions

    def __init__(self, core, env_name: str, num_envs: int, seq_len: int,
                 device, seed: int, time_horizon: int,
                 max_episode_steps: int | None = None, *, ou_envs: int = 0,
                 warmup_steps: int = 0, ou_theta: float = 0.15,
                 ou_sigma: float = 0.6):
        if env_name not in DEVICE_ENVS:
            raise ValueError(
                f"env {env_name!r} has no device dynamics "
                f"(available: {sorted(DEVICE_ENVS)})")
        self.dyn = dyn = DEVICE_ENVS[env_name]
        self.continuous = is_continuous_env(env_name)
        if getattr(core, "input2_dim", None) is not None:
            raise ValueError("DeviceRollout does not support dual-body cores")
        if self.continuous:
            self._check_gaussian_core(core, env_name)
            self.mode = GAUSSIAN_MODES[tuple(core.head_names[:2])]
        else:
            self._check_discrete_core(core, env_name)
            self.mode = None
        self.ou_envs, self.warmup_steps = int(ou_envs), int(warmup_steps)
        self.ou_theta, self.ou_sigma = float(ou_theta), float(ou_sigma)
        if self.ou_envs < 0 or self.warmup_steps < 0:
            raise ValueError("ou_envs and warmup_steps must not be negative")
        if (self.ou_envs or self.warmup_steps) and self.mode != 1:
            # importance ratios of on-policy algorithms assume the actions
            # came from the recorded policy, which OU actions do not
            raise ValueError(
                "OU exploration needs an off-policy Gaussian core with heads "
                f"['mu', 'log_std'] (got heads {core.head_names})")
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
        if self.continuous:  # logits = [mu | std or log_std], act of width 1
            self.fields = rollout_fields(dyn.obs_dim, dyn.act_dim, H, True)
        else:
            self.fields = rollout_fields(dyn.obs_dim, dyn.n_actions, H, False)
        # the batch: same tensor objects on every call (graph-capturable)
        self.batch = {k: torch.zeros(N, S, d, **f32) for k, d in self.fields.items()}
        # persistent per-env state; env_state is (N, state_dim), and the
        # batch's obs / the core's input are dyn.observe(env_state)
        self._env_ids = torch.arange(N, device=dev, dtype=torch.int64)
        self.env_state = dyn.reset(self._reset_uniforms(0)).contiguous()
        self.ou_state = torch.zeros(N, **f32)  # OU exploration (Gaussian mode 1)
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
    def _check_discrete_core(self, core, env_name: str):
        dyn = self.dyn
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

    def _check_gaussian_core(self, core, env_name: str):
        dyn = self.dyn
        if tuple((core.head_names or [])[:2]) not in GAUSSIAN_MODES:
            raise ValueError(
                f"DeviceRollout on {env_name} needs a Gaussian policy core "
                "whose first heads are ['mu', 'std'] or ['mu', 'log_std'] "
                f"(got heads {core.head_names})")
        if core.hidden not in (32, 64, 128):
            raise ValueError(
                f"hidden size {core.hidden} unsupported (32/64/128)")
        second = core.head_names[1]
        # the counter hash has eight lanes per tick, which is one normal:
        # more action dimensions need a wider counter (csrc/rollout_rng.h)
        if (core.input_dim != dyn.obs_dim or core.head_dims["mu"] != dyn.act_dim
                or core.head_dims[second] != dyn.act_dim):
            raise ValueError(
                f"core shape (obs {core.input_dim}, action dims "
                f"{core.head_dims['mu']}/{core.head_dims[second]}) does not "
                f"match {env_name} (obs {dyn.obs_dim}, action dim "
                f"{dyn.act_dim})")

    def _reset_uniforms(self, tick) -> torch.Tensor:
        """(N, draws) uniforms of a reset caused by ``tick``: lanes 1.."""
        draws = getattr(self.dyn, "reset_draws", self.dyn.state_dim)
        return torch.stack([uniform(self.seed, self._env_ids, tick, k)
                            for k in range(1, draws + 1)], 1)

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
            if self.continuous:
                self._rollout_eager_gaussian(ep_ret)
            else:
                self._rollout_eager(ep_ret)
        elif self.continuous:
            b = self.batch
            self._ext.rollout_gaussian(
                *(w.detach() for w in self._weights()),
                self.env_state, self.h, self.c, self.is_fir, self.ep_steps,
                self.ep_run, self.tick, self.ou_state, b["obs"], b["act"],
                b["rew"], b["logits"], b["log_prob"], b["is_fir"], b["hx"],
                b["cx"], ep_ret, self.dyn.env_id, self.mode, self.seed,
                self.time_horizon, self.max_episode_steps, self.ou_envs,
                min(self.warmup_steps, _M32), self.ou_theta, self.ou_sigma)
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

    def _rollout_eager_gaussian(self, ep_ret: torch.Tensor):
        """fp32 torch reference of ``rollout_gaussian``: the formulas of the
        module docstring on ``SeqLSTMCore._forward_eager``. Sampling a
        Gaussian has no decision boundary, so ``margin`` records the env's
        threshold distances only."""
        dyn, b = self.dyn, self.batch
        second = self.core.head_names[1]
        for t in range(self.S):
            self.tick += 1
            obs = dyn.observe(self.env_state)
            b["obs"][:, t] = obs
            b["hx"][:, t] = self.h
            b["cx"][:, t] = self.c
            b["is_fir"][:, t, 0] = self.is_fir
            outs, h, c = self.core._forward_eager(
                obs.unsqueeze(1), self.h, self.c)
            mu, s = outs["mu"][:, 0, 0], outs[second][:, 0, 0]
            n = normal(self.seed, self._env_ids, self.tick)
            if self.mode == 0:
                mean = torch.tanh(mu)
                sd = torch.nn.functional.softplus(s) + 1e-4
                act = mean + sd * n
                log_prob = -0.5 * n * n - torch.log(sd) - HALF_LOG_2PI
            else:
                ls = s.clamp(-20.0, 2.0)
                sd = torch.exp(ls)
                tick = self.tick.to(torch.int64) & _M32
                explore = (self._env_ids < self.ou_envs) | (tick <= self.warmup_steps)
                ou = self.ou_state - self.ou_theta * self.ou_state + self.ou_sigma * n
                self.ou_state = torch.where(explore, ou, self.ou_state)
                z = torch.where(explore, ou, mu + sd * n)
                q = (z - mu) / sd
                quad = torch.where(explore, -0.5 * (q * q), -0.5 * n * n)
                act = torch.tanh(z)
                log_prob = (quad - ls - HALF_LOG_2PI
                            - torch.log(1.0 - act * act + 1e-7))
            self.margin = torch.minimum(
                self.margin, dyn.threshold_margin(self.env_state, act))
            state, rew, terminated = dyn.step(self.env_state, act)
            self.ep_steps += 1
            self.ep_run += rew
            done = terminated | (self.ep_steps >= self.max_episode_steps)
            reset = done | (self.ep_steps >= self.time_horizon)
            b["act"][:, t, 0] = act
            b["rew"][:, t, 0] = rew
            b["logits"][:, t, 0] = mu
            b["logits"][:, t, 1] = s
            b["log_prob"][:, t, 0] = log_prob
            ep_ret[:, t] = torch.where(reset, self.ep_run,
                                       torch.full_like(rew, NO_EPISODE))
            fresh = dyn.reset(self._reset_uniforms(self.tick))
            keep = (~reset).to(torch.float32)
            self.env_state = torch.where(reset[:, None], fresh, state)
            self.h = h * keep[:, None]
            self.c = c * keep[:, None]
            self.ou_state = torch.where(reset, torch.zeros_like(keep), self.ou_state)
            self.is_fir = reset.to(torch.float32)
            self.ep_steps *= (~reset).to(torch.int32)
            self.ep_run *= keep

    def _rollout_eager(self, ep_ret: torch.Tensor):
        """fp32 torch reference: same hash, op order of
        ``SeqLSTMCore._forward_eager``, same sampling rule and dynamics."""
        dyn, b, A = self.dyn, self.batch, self.dyn.n_actions
        for t in range(self.S):
            self.tick += 1
            obs = dyn.observe(self.env_state)
            b["obs"][:, t] = obs
            b["hx"][:, t] = self.h
            b["cx"][:, t] = self.c
            b["is_fir"][:, t, 0] = self.is_fir
            outs, h, c = self.core._forward_eager(
                obs.unsqueeze(1), self.h, self.c)
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
            fresh = dyn.reset(self._reset_uniforms(self.tick))
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
