"""float64 NumPy model of the exploration epilogue (include/fleet_hip.h "exploration actions on the device"): the Philox counter
scheme, the uniforms, Box-Muller, the three modes and the log-probability.  The generator itself is
`replay_model.philox4x32_10`; `words` is the same function over arrays of counters (held to the scalar one by
tests/test_explore_cpu.py).  Nothing here needs a GPU or the library."""
import numpy as np

import replay_model as rp

M32 = rp.M32
LOG_SQRT_2PI = 0.9189385332046727  # the device adds float32(0.9189385332)
EPS_MAX = float(np.sqrt(48 * np.log(2)))  # |eps| <= sqrt(-2 ln 2^-24) = 5.768...
SEED = 0x5EED0000C0FFEE11  # the seed of the statistical checks, on the host model and on the device (high half set)
STAT_SHAPE = (4096, 50)


def counter(env, block, step):
    """(env id, column block, step lo, step hi)."""
    return int(env) & M32, int(block) & M32, int(step) & M32, (int(step) >> 32) & M32


def key(seed):
    return int(seed) & M32, (int(seed) >> 32) & M32


def block_words(seed, env, block, step):
    """The four words of one (env, column block, step), with the scalar generator."""
    return rp.philox4x32_10(counter(env, block, step), key(seed))


def words(seed, env_ids, A, step) -> np.ndarray:
    """uint64 [E, ceil(A / 4), 4]: the blocks of every (env, column block) at `step` (uint64 arithmetic on 32-bit values)."""
    u = np.uint64
    env_ids = np.asarray(env_ids, dtype=np.int64) & M32
    nb = -(-A // 4)
    c0 = np.repeat(env_ids.astype(u)[:, None], nb, axis=1)
    c1 = np.repeat(np.arange(nb, dtype=u)[None, :], len(env_ids), axis=0)
    _, _, s_lo, s_hi = counter(0, 0, step)
    c2, c3 = np.full_like(c0, s_lo), np.full_like(c0, s_hi)
    k0, k1 = key(seed)
    m, s = u(M32), u(32)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ u(k0), p1 & m, (p0 >> s) ^ c3 ^ u(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def u_open_low(x):
    """((x >> 8) + 1) * 2^-24, in (0, 1]: exact in float32."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def u_open_high(x):
    """(x >> 8) * 2^-24, in [0, 1): exact in float32."""
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def normals(seed, env_ids, A, step) -> np.ndarray:
    """eps float64 [E, A]: Box-Muller on the pairs (x0, x1) and (x2, x3) of every block; the even column takes the cosine."""
    w = words(seed, env_ids, A, step)
    r = np.sqrt(-2.0 * np.log(u_open_low(w[..., 0::2])))  # [E, nb, 2]
    t = 2.0 * np.pi * u_open_high(w[..., 1::2])
    z = np.stack([r * np.cos(t), r * np.sin(t)], axis=-1)  # [E, nb, pair, (cos, sin)]
    return z.reshape(len(w), -1)[:, :A]


def uniforms(seed, env_ids, A, step) -> np.ndarray:
    """u float64 [E, A] in [0, 1): every column's own word."""
    return u_open_high(words(seed, env_ids, A, step)).reshape(len(env_ids), -1)[:, :A]


# ---- the modes -------------------------------------------------------------------------------------------------------------------
def log_prob64(actions, mean, log_std) -> np.ndarray:
    """Normal(mean, exp(log_std)).log_prob(actions).sum(-1) in float64 on the given (float32) numbers."""
    a, m, ls = (np.asarray(v, dtype=np.float64) for v in (actions, mean, log_std))
    return (-((a - m) ** 2) / (2.0 * np.exp(ls) ** 2) - ls - LOG_SQRT_2PI).sum(-1)


def log_prob_torch32(actions, mean, log_std) -> np.ndarray:
    """The same with torch-CPU float32, as SB3 evaluates it."""
    import torch

    a, m, ls = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for v in (actions, mean, log_std))
    return torch.distributions.Normal(m, ls.exp().expand_as(m)).log_prob(a).sum(-1).numpy()


def gaussian(mean, log_std, eps, low=-1.0, high=1.0):
    """(actions, env_actions, log_prob) of the GAUSSIAN mode with a clipping head, float64."""
    mean, eps = np.asarray(mean, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    a = mean + np.exp(np.asarray(log_std, dtype=np.float64)) * eps
    return a, np.clip(a, low, high), log_prob64(a, mean, log_std)


def action_noise(d, sigma, shift, eps, low=-1.0, high=1.0):
    """SB3's `_sample_action` with NormalActionNoise(shift, sigma) on the unit action space."""
    d, eps = np.asarray(d, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    return np.clip(d + (np.asarray(shift, dtype=np.float64) + np.asarray(sigma, dtype=np.float64) * eps), low, high)


def uniform(low, high, u):
    return low + (high - low) * np.asarray(u, dtype=np.float64)


# ---- statistics ------------------------------------------------------------------------------------------------------------------
def lag1(a, b) -> float:
    """Sample correlation of two equally shaped arrays of (nominally) standard normals."""
    a, b = np.ravel(a), np.ravel(b)
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


def moments(eps, eps_next_step) -> dict:
    """What the statistical checks look at: mean, variance, max |eps| and the three lag-1 correlations, with their bounds for
    n = eps.size draws (5 standard errors: mean 1/sqrt(n), variance sqrt(2/n), correlation 1/sqrt(n))."""
    n = eps.size
    return {"n": n, "mean": float(eps.mean()), "var": float(eps.var()), "max_abs": float(np.abs(eps).max()),
            "corr_columns": lag1(eps[:, :-1], eps[:, 1:]), "corr_envs": lag1(eps[:-1], eps[1:]), "corr_steps": lag1(eps, eps_next_step),
            "bound_mean": 5 / np.sqrt(n), "bound_var": 5 * np.sqrt(2 / n), "bound_corr": 5 / np.sqrt(n)}


def check_moments(m: dict) -> list:
    """The failed checks of `moments`, by name."""
    bad = []
    if not abs(m["mean"]) <= m["bound_mean"]:
        bad.append("mean")
    if not abs(m["var"] - 1) <= m["bound_var"]:
        bad.append("var")
    if not m["max_abs"] <= 5.77:
        bad.append("max_abs")
    for k in ("corr_columns", "corr_envs", "corr_steps"):
        if not abs(m[k]) <= m["bound_corr"]:
            bad.append(k)
    return bad
