"""Plain restatement of stable-baselines3 2.3.2 `VecNormalize` (the spec of fleet_norm.hip) for the tests.

Arithmetic is generic: float64 NumPy arrays for the comparisons with the device, or object arrays of `fractions.Fraction` for
the known answers (everything but the square root is exact then).  Deviations from SB3 that the device makes on purpose, and
this model with it: (a) batch moments in float64 (SB3: float32 accumulation of the float32 observations); (b) the reward
enters as the env's float64 reward rounded to float32.
"""
from __future__ import annotations

import numpy as np


def batch_moments(X):
    """mean and population variance over axis 0 (two passes, as np.var)."""
    n = X.shape[0]
    m = X.sum(axis=0) / n
    d = X - m
    return m, (d * d).sum(axis=0) / n, n


class RMS:
    """SB3 RunningMeanStd: update_from_moments, operation for operation."""

    def __init__(self, shape=(), zero=0.0, one=1.0, count=1e-4):
        self.mean = np.full(shape, zero, dtype=object if not isinstance(zero, float) else np.float64)
        self.var = np.full(shape, one, dtype=self.mean.dtype)
        self.count = count

    def update(self, X):
        bm, bv, n = batch_moments(X)
        delta = bm - self.mean
        tot = self.count + n
        new_mean = self.mean + delta * n / tot
        m_a = self.var * self.count
        m_b = bv * n
        m_2 = m_a + m_b + delta * delta * self.count * n / tot
        self.mean, self.var, self.count = new_mean, m_2 / tot, tot


def clip(x, c):
    return np.minimum(np.maximum(x, -c), c)


class VecNormModel:
    """reset(obs) -> obs'; step(obs, reward, done, terminal) -> (obs', reward', terminal') with float64 inputs / outputs
    (obs' and terminal' are rounded to float32 as the device does)."""

    def __init__(self, num_envs, obs_dim, training=True, norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0,
                 gamma=0.99, epsilon=1e-8, exact=False):
        from fractions import Fraction

        zero, one, cnt = (Fraction(0), Fraction(1), Fraction(1, 10000)) if exact else (0.0, 1.0, 1e-4)
        self.exact = exact
        self.obs_rms = RMS((obs_dim,), zero, one, cnt)
        self.ret_rms = RMS((), zero, one, cnt)
        self.returns = np.full(num_envs, zero, dtype=self.obs_rms.mean.dtype)
        self.training, self.norm_obs, self.norm_reward = training, norm_obs, norm_reward
        self.clip_obs, self.clip_reward, self.gamma, self.epsilon = clip_obs, clip_reward, gamma, epsilon

    def _as(self, x):
        if self.exact:
            from fractions import Fraction

            return np.vectorize(Fraction, otypes=[object])(np.asarray(x))
        return np.asarray(x, dtype=np.float64)

    def normalize_obs(self, obs):
        x = self._as(obs)
        if not self.norm_obs:
            return x if self.exact else x.astype(np.float32)
        sd = np.sqrt(np.asarray(self.obs_rms.var, dtype=np.float64) + self.epsilon)
        y = clip((np.asarray(x, dtype=np.float64) - np.asarray(self.obs_rms.mean, dtype=np.float64)) / sd, self.clip_obs)
        return y.astype(np.float32)

    def normalize_reward(self, r):
        r = np.asarray(r, dtype=np.float64)
        if not self.norm_reward:
            return r
        return clip(r / np.sqrt(float(self.ret_rms.var) + self.epsilon), self.clip_reward)

    def reset(self, obs):
        self.returns = self.returns * 0
        if self.training and self.norm_obs:
            self.obs_rms.update(self._as(obs))
        return self.normalize_obs(obs)

    def step(self, obs, reward, done, terminal=None, outputs=True):
        """reward: the env's float64 rewards (rounded to float32 here, deviation (b)).  outputs=False: advance the state only."""
        done = np.asarray(done).astype(bool)
        if self.training and self.norm_obs:
            self.obs_rms.update(self._as(obs))
        o = self.normalize_obs(obs) if outputs else None
        r = np.asarray(reward, dtype=np.float64).astype(np.float32).astype(np.float64)
        if self.training:
            self.returns = self.returns * self.gamma + self._as(r)
            self.ret_rms.update(self.returns)
        rn = self.normalize_reward(r) if outputs else None
        t = None
        if terminal is not None:
            t = np.array(terminal, dtype=np.float32, copy=True)
            if done.any():
                t[done] = self.normalize_obs(np.asarray(terminal)[done])
        self.returns[done] = 0
        return o, rn, t
