"""Pendulum-v1: native implementation (standard published dynamics per the
Gymnasium Pendulum docs), with one deviation: the action is NORMALISED. The
policy's action ``a`` lies in [-1, 1] and the torque is ``u = 2 * clip(a, -1,
1)``, where Gymnasium takes the torque in [-2, 2] directly (docs/MIGRATING.md).
Nothing in the workers scales actions, and MountainCarContinuous-v0 takes
[-1, 1] as well. A good policy scores about -150 over the 200 steps.
"""
from __future__ import annotations

import math

import numpy as np

from .base import Box, register


def wrap_angle(x: float) -> float:
    """x modulo 2π into [-π, π)."""
    return x - 2.0 * math.pi * math.floor((x + math.pi) / (2.0 * math.pi))


@register("Pendulum-v1")
class PendulumEnv:
    GRAVITY = 10.0
    MASS = 1.0
    LENGTH = 1.0
    DT = 0.05
    MAX_SPEED = 8.0
    MAX_TORQUE = 2.0
    MAX_EPISODE_STEPS = 200

    def __init__(self, seed: int | None = None):
        high = np.array([1.0, 1.0, self.MAX_SPEED], dtype=np.float32)
        self.observation_space = Box(-high, high)
        self.action_space = Box(np.array([-1.0]), np.array([1.0]))
        self._rng = np.random.default_rng(seed)
        self._state = None  # (θ, θ̇); θ = 0 is upright and is never wrapped
        self._steps = 0

    def seed(self, seed: int):
        self._rng = np.random.default_rng(seed)

    def _obs(self):
        theta, theta_dot = self._state
        return np.array([math.cos(theta), math.sin(theta), theta_dot],
                        dtype=np.float32)

    def reset(self, seed: int | None = None):
        if seed is not None:
            self.seed(seed)
        theta = self._rng.uniform(-math.pi, math.pi)
        theta_dot = self._rng.uniform(-1.0, 1.0)
        self._state = np.array([theta, theta_dot], dtype=np.float64)
        self._steps = 0
        return self._obs(), {}

    def step(self, action):
        action = np.asarray(action, dtype=np.float64).reshape(-1)
        u = self.MAX_TORQUE * float(np.clip(action[0], -1.0, 1.0))
        theta, theta_dot = self._state
        g, m, l, dt = self.GRAVITY, self.MASS, self.LENGTH, self.DT

        cost = wrap_angle(theta) ** 2 + 0.1 * theta_dot**2 + 0.001 * u**2
        theta_dot += (3.0 * g / (2.0 * l) * math.sin(theta)
                      + 3.0 / (m * l**2) * u) * dt
        theta_dot = float(np.clip(theta_dot, -self.MAX_SPEED, self.MAX_SPEED))
        theta += theta_dot * dt
        self._state = np.array([theta, theta_dot], dtype=np.float64)
        self._steps += 1

        truncated = self._steps >= self.MAX_EPISODE_STEPS
        return self._obs(), -cost, False, truncated, {}
