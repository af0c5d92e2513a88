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


def _wave_order_sum(P, waves=4):
    """P [k, ...] -> [...]: `waves` accumulators, accumulator w adds entries w, w + waves, ... one after the other from 0.0,
    then the accumulators are added in the order 0, 1, ...  (the zero padding of the tail adds exact zeros)."""
    k = P.shape[0]
    rounds = -(-k // waves)
    Q = np.zeros((rounds * waves,) + P.shape[1:])
    Q[:k] = P
    Q = Q.reshape((rounds, waves) + P.shape[1:])
    acc = np.zeros_like(Q[0])
    for i in range(rounds):
        acc = acc + Q[i]
    out = acc[0]
    for w in range(1, waves):
        out = out + acc[w]
    return out


def _lane_tree_sum(P, lanes=64):
    """P [k, ...] -> [...]: lane l adds entries l, l + lanes, ... one after the other from 0.0, then the shuffle tree
    lane[i] += lane[i + off] for off = lanes / 2 ... 1 leaves the total in lane 0."""
    k = P.shape[0]
    rounds = -(-k // lanes)
    Q = np.zeros((rounds * lanes,) + P.shape[1:])
    Q[:k] = P
    Q = Q.reshape((rounds, lanes) + P.shape[1:])
    acc = np.zeros_like(Q[0])
    for i in range(rounds):
        acc = acc + Q[i]
    off = lanes // 2
    while off:
        acc = acc[:off] + acc[off:2 * off]
        off //= 2
    return acc[0]


def _shifted_moments(S1, S2, K, n):
    """fleet_norm.hip batch_moments: mean and population variance from the sums shifted by K."""
    m2 = S2 - S1 * S1 / n
    with np.errstate(invalid="ignore", divide="ignore"):
        return K + S1 / n, np.where(m2 > 0.0, m2 / n, 0.0), n


def device_order_moments(X, rows=64, waves=4):
    """The observations' batch moments in the kernels' summation scheme (the comments at the top of fleet_norm.hip), float64
    NumPy, X [E, D]: the shift K is row 0; a slab holds `rows` rows; inside a slab wave w takes rows w, w + 4, ... and the four
    waves are added in the order 0..3 (norm_moments); the slabs are added the same way, wave w taking slabs w, w + 4, ...
    (norm_finalize); then mean = K + S1 / n and var = m2 > 0 ? m2 / n : 0 with m2 = S2 - S1^2 / n.
    It restates the ORDER of the sums, not the device's bits (its square root is not in here): the tests compare it with the
    two-pass `batch_moments` to show which tolerance the scheme can hold on its own."""
    X = np.asarray(X, dtype=np.float64)
    E = X.shape[0]
    K = X[0]
    V = X - K
    slabs = -(-E // rows)
    P = np.zeros((slabs * rows,) + X.shape[1:])
    P[:E] = V
    P = np.moveaxis(P.reshape((slabs, rows) + X.shape[1:]), 0, 1)  # [row in slab, slab, ...]
    S1 = _wave_order_sum(_wave_order_sum(P, waves), waves)
    S2 = _wave_order_sum(_wave_order_sum(P * P, waves), waves)
    return _shifted_moments(S1, S2, K, E)


def device_order_return_moments(x, rows=64):
    """The same for the returns block, x [E] (the new returns): one row per lane and the 64-lane shuffle tree per slab
    (norm_moments), then lane l takes slabs l, l + 64, ... and the tree again (norm_finalize)."""
    x = np.asarray(x, dtype=np.float64)
    E = x.shape[0]
    K = x[0]
    slabs = -(-E // rows)
    P = np.zeros(slabs * rows)
    P[:E] = x - K
    P = P.reshape(slabs, rows).T  # [lane, slab]
    S1 = _lane_tree_sum(_lane_tree_sum(P, rows), rows)
    S2 = _lane_tree_sum(_lane_tree_sum(P * P, rows), rows)
    return _shifted_moments(S1, S2, K, E)


class RMS:
    """SB3 RunningMeanStd: update_from_moments, operation for operation.  `moments`: the batch moments (default: two passes)."""

    def __init__(self, shape=(), zero=0.0, one=1.0, count=1e-4, moments=batch_moments):
        self.mean = np.full(shape, zero, dtype=object if not isinstance(zero, float) else np.float64)
        self.var = np.full(shape, one, dtype=self.mean.dtype)
        self.count = count
        self.moments = moments

    def update(self, X):
        bm, bv, n = self.moments(X)
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
                 gamma=0.99, epsilon=1e-8, exact=False, device_order=False):
        """device_order: take the batch moments in the kernels' summation scheme (`device_order_moments`) instead of two passes."""
        from fractions import Fraction

        zero, one, cnt = (Fraction(0), Fraction(1), Fraction(1, 10000)) if exact else (0.0, 1.0, 1e-4)
        self.exact = exact
        self.obs_rms = RMS((obs_dim,), zero, one, cnt, device_order_moments if device_order else batch_moments)
        self.ret_rms = RMS((), zero, one, cnt, device_order_return_moments if device_order else batch_moments)
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
        self.returns = self.returns * 0 + 0  # (+ 0: SB3 sets np.zeros, and -0.0 + 0 is +0.0)
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


    def get_state(self):
        """The state in the shape of DeviceNormalizer.get_state() (for `check_stats` between two models)."""
        from fleetrl_amd.vec_normalize import NormState, RunningStats

        o, r = self.obs_rms, self.ret_rms
        return NormState(RunningStats(np.array(o.mean, dtype=np.float64), np.array(o.var, dtype=np.float64), o.count),
                         RunningStats(np.float64(r.mean), np.float64(r.var), r.count), np.array(self.returns, dtype=np.float64))


def stats_ratios(st, model):
    """Worst error of a state's running statistics over `check_stats`'s tolerance for it: (mean, var, ret mean, ret var).
    A ratio <= 1 passes `check_stats`."""
    m, v = model.obs_rms.mean, model.obs_rms.var
    dm, dv = np.abs(st.obs_rms.mean - m), np.abs(st.obs_rms.var - v)
    with np.errstate(invalid="ignore", divide="ignore"):
        r_mean = np.where(dm == 0, 0.0, dm / (1e-12 * (np.abs(m) + np.sqrt(v))))
        r_var = np.where(dv == 0, 0.0, np.minimum(dv / (1e-10 * v), dv / (1e-14 * (1 + m * m))))
    rm, rv = float(model.ret_rms.mean), float(model.ret_rms.var)
    drm, drv = abs(float(st.ret_rms.mean) - rm), abs(float(st.ret_rms.var) - rv)
    r_rmean = 0.0 if drm == 0 else drm / (1e-12 * (abs(rm) + np.sqrt(rv)))
    r_rvar = 0.0 if drv == 0 else drv / max(1e-10 * rv, 1e-14 * (1 + rm * rm))
    return float(np.max(r_mean)), float(np.max(r_var)), float(r_rmean), float(r_rvar)


def check_stats(norm, model, tag, fraction=1.0):
    """The running statistics of `norm` (anything with get_state()) against the model's: means to 1e-12 of |mean| + sd,
    variances to 1e-10 relative or 1e-14 of 1 + mean^2; counts and returns bit for bit.  `fraction` < 1 asks for that part of
    each tolerance."""
    st = norm.get_state()
    m, v = model.obs_rms.mean, model.obs_rms.var
    assert np.all(np.abs(st.obs_rms.mean - m) <= fraction * 1e-12 * (np.abs(m) + np.sqrt(v))), tag
    ok = (np.abs(st.obs_rms.var - v) <= fraction * 1e-10 * v) | (np.abs(st.obs_rms.var - v) <= fraction * 1e-14 * (1 + m * m))
    assert ok.all(), (tag, np.max(np.abs(st.obs_rms.var - v) / np.maximum(v, 1e-300)))
    rm, rv = float(model.ret_rms.mean), float(model.ret_rms.var)
    assert abs(float(st.ret_rms.mean) - rm) <= fraction * 1e-12 * (abs(rm) + np.sqrt(rv)), tag
    assert abs(float(st.ret_rms.var) - rv) <= fraction * max(1e-10 * rv, 1e-14 * (1 + rm * rm)), tag
    assert st.obs_rms.count == model.obs_rms.count and st.ret_rms.count == model.ret_rms.count, tag
    assert np.array_equal(st.returns.view(np.uint64), model.returns.view(np.uint64)), tag


def close_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ulps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return bool(np.all((ulps <= 2) | (np.abs(a - b) <= 1e-6)))


def close_reward(r, mr):
    """The normalised rewards against the model's: 1e-6 or two float32 spacings of the value."""
    r, mr = np.asarray(r, np.float64), np.asarray(mr, np.float64)
    return bool(np.all((np.abs(r - mr) <= 1e-6) | (np.abs(r - mr) <= 2 * np.spacing(np.abs(mr).astype(np.float32)))))
