"""Acrobot-v1: native implementation (standard published dynamics per the
Gymnasium Acrobot docs: the "book" equations of motion, one RK4 step of 0.2 s
per env step). Three actions, torque ``action - 1`` on the second joint;
reward -1 per step until the tip swings above the bar. Solved ≈ -100 reward.
"""
from __future__ import annotations

import math

import numpy as np

from .base import Box, Discrete, register
from .pendulum import wrap_angle


@register("Acrobot-v1")
class AcrobotEnv:
    DT = 0.2
    LINK_LENGTH_1 = 1.0
    LINK_MASS_1 = 1.0
    LINK_MASS_2 = 1.0
    LINK_COM_POS_1 = 0.5
    LINK_COM_POS_2 = 0.5
    LINK_MOI = 1.0
    GRAVITY = 9.8
    MAX_VEL_1 = 4 * math.pi
    MAX_VEL_2 = 9 * math.pi
    MAX_EPISODE_STEPS = 500

    def __init__(self, seed: int | None = None):
        high = np.array([1.0, 1.0, 1.0, 1.0, self.MAX_VEL_1, self.MAX_VEL_2],
                        dtype=np.float32)
        self.observation_space = Box(-high, high)
        self.action_space = Discrete(3)
        self._rng = np.random.default_rng(seed)
        self._state = None  # (θ1, θ2, θ̇1, θ̇2); θ1 = 0 hangs straight down
        self._steps = 0

    def seed(self, seed: int):
        self._rng = np.random.default_rng(seed)

    def _obs(self):
        t1, t2, d1, d2 = self._state
        return np.array([math.cos(t1), math.sin(t1), math.cos(t2),
                         math.sin(t2), d1, d2], dtype=np.float32)

    def reset(self, seed: int | None = None):
        if seed is not None:
            self.seed(seed)
        self._state = self._rng.uniform(-0.1, 0.1, size=4).astype(np.float64)
        self._steps = 0
        return self._obs(), {}

    @classmethod
    def derivs(cls, s: np.ndarray, torque: float) -> np.ndarray:
        """d/dt of (θ1, θ2, θ̇1, θ̇2) under a constant torque."""
        m1, m2, l1 = cls.LINK_MASS_1, cls.LINK_MASS_2, cls.LINK_LENGTH_1
        lc1, lc2 = cls.LINK_COM_POS_1, cls.LINK_COM_POS_2
        i1 = i2 = cls.LINK_MOI
        g = cls.GRAVITY
        t1, t2, dt1, dt2 = s
        d1 = (m1 * lc1**2
              + m2 * (l1**2 + lc2**2 + 2 * l1 * lc2 * math.cos(t2)) + i1 + i2)
        d2 = m2 * (lc2**2 + l1 * lc2 * math.cos(t2)) + i2
        # the published cos(x - π/2) written as sin x, which is exactly 0 at
        # x = 0: hanging at rest is a fixed point to the last bit
        phi2 = m2 * lc2 * g * math.sin(t1 + t2)
        phi1 = (-m2 * l1 * lc2 * dt2**2 * math.sin(t2)
                - 2 * m2 * l1 * lc2 * dt2 * dt1 * math.sin(t2)
                + (m1 * lc1 + m2 * l1) * g * math.sin(t1)
                + phi2)
        ddt2 = ((torque + d2 / d1 * phi1
                 - m2 * l1 * lc2 * dt1**2 * math.sin(t2) - phi2)
                / (m2 * lc2**2 + i2 - d2**2 / d1))
        ddt1 = -(d2 * ddt2 + phi1) / d1
        return np.array([dt1, dt2, ddt1, ddt2], dtype=np.float64)

    @classmethod
    def rk4(cls, s: np.ndarray, torque: float, dt: float) -> np.ndarray:
        """One classical Runge-Kutta step; angles and speeds left unbounded."""
        k1 = cls.derivs(s, torque)
        k2 = cls.derivs(s + 0.5 * dt * k1, torque)
        k3 = cls.derivs(s + 0.5 * dt * k2, torque)
        k4 = cls.derivs(s + dt * k3, torque)
        return s + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)

    @classmethod
    def energy(cls, s: np.ndarray) -> float:
        """Kinetic plus potential energy (conserved under zero torque)."""
        m1, m2, l1 = cls.LINK_MASS_1, cls.LINK_MASS_2, cls.LINK_LENGTH_1
        lc1, lc2 = cls.LINK_COM_POS_1, cls.LINK_COM_POS_2
        i1 = i2 = cls.LINK_MOI
        g = cls.GRAVITY
        t1, t2, dt1, dt2 = s
        d11 = (m1 * lc1**2
               + m2 * (l1**2 + lc2**2 + 2 * l1 * lc2 * math.cos(t2)) + i1 + i2)
        d12 = m2 * (lc2**2 + l1 * lc2 * math.cos(t2)) + i2
        d22 = m2 * lc2**2 + i2
        kinetic = 0.5 * d11 * dt1**2 + d12 * dt1 * dt2 + 0.5 * d22 * dt2**2
        potential = (-(m1 * lc1 + m2 * l1) * g * math.cos(t1)
                     - m2 * lc2 * g * math.cos(t1 + t2))
        return kinetic + potential

    def step(self, action):
        action = int(action)
        assert action in (0, 1, 2), f"invalid action {action}"
        torque = float(action - 1)
        s = self.rk4(self._state, torque, self.DT)
        s[0] = wrap_angle(s[0])
        s[1] = wrap_angle(s[1])
        s[2] = float(np.clip(s[2], -self.MAX_VEL_1, self.MAX_VEL_1))
        s[3] = float(np.clip(s[3], -self.MAX_VEL_2, self.MAX_VEL_2))
        self._state = s
        self._steps += 1

        terminated = bool(-math.cos(s[0]) - math.cos(s[1] + s[0]) > 1.0)
        truncated = self._steps >= self.MAX_EPISODE_STEPS
        reward = 0.0 if terminated else -1.0
        return self._obs(), reward, terminated, truncated, {}
