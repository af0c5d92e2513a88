"""The forward side of SAC (include/fleet_hip.h "SAC on the device") restated for the tests: stable-baselines3 2.3.2's expressions in
float64, the header's float32 chain from stored values, the lane-order sum, and the bounds the GPU tests hold the device to.  Nothing
here needs a GPU or the library.

What SB3 computes (names as in SB3 2.3.2):
  `Actor.get_action_dist_params`   latent = latent_pi(obs); mean = mu(latent); log_std = clamp(log_std(latent), LOG_STD_MIN = -20,
                                   LOG_STD_MAX = 2)
  `SquashedDiagGaussianDistribution`   gaussian_actions = mean + exp(log_std) * eps; actions = tanh(gaussian_actions);
                                   log_prob = Normal(mean, std).log_prob(gaussian_actions).sum(1) - log(1 - actions^2 + 1e-6).sum(1)
  `SAC.train`                      next_q = min_c critic_target_c(next_obs, next_actions) - ent_coef * next_log_prob;
                                   target_q = rewards + (1 - dones) * gamma * next_q
`sb3_log_prob64` and `sb3_target64` are those lines in float64; `log_prob_terms64` is the header's form, with the Gaussian term written
in eps: -(u - m)^2 / (2 sd^2) = -eps^2 / 2 because u - m = sd * eps.  tests/test_sac_cpu.py holds the two to float64 rounding.

The bounds of tests/test_sac_gpu.py.  The device's expf, logf and tanhf are taken to be within 2 ulp of the true function of their
float32 argument, as tests/test_explore_gpu.py takes them; ulp(x) <= 2^-23 |x|.  Every stage is compared with the model fed the
device's OWN stored outputs of the stage before, so only that stage's error is seen:
  u     u = fmaf(sd, eps, m) with sd = expf(ls) up to 2 ulp off: sd * eps moves by <= 2 ulp of it, one more rounding of the sum (half an
        ulp of u), and half an ulp for the model's own float64 -> float32 comparison: within 4 * 2^-23 * max(|u|, |sd * eps|), the bound
        tests/test_explore_gpu.py uses for the same expression (`U_ULPS`).
  a     a = tanhf(u_dev): within 2 ulp of tanh(u_dev), |a| <= 1: 2.5 * 2^-23 * max(|a|, 2^-126) with half an ulp for the binade edge
        (`A_ULPS`).
  lp    t[j] is exactly rounded arithmetic on stored values: the model's bits (`fma32` is a correctly rounded fmaf), and S(t) with it.
        c[j] = logf(arg) on an argument that is exactly rounded arithmetic on the stored a: the device's c is within 2 ulp of log(arg),
        the model's float32 c within half an ulp: |dc[j]| <= 2.5 * 2^-23 |c[j]|.  S is a float32 sum tree of depth
        n = ceil(A / 64) + 6 (the lane's chain, then 6 butterfly levels): S(c_dev) and S(c_model) differ by at most sum_j |dc[j]|
        plus twice the tree's rounding, 2 * n * 2^-24 * sum_j |c[j]|.  The final subtraction is one rounding of two values that differ by
        that much: one more ulp of lp.  So
          |lp_dev - lp_model| <= (2.5 * 2^-23 + 2 n * 2^-24) * sum_j |c[j]| + 2^-23 * |lp|        (`log_prob_bound`)
        This is a worst-case bound and is used as it is, with no further margin: the typical error is several times smaller because
        the terms' errors do not all point one way.  It holds in the saturated case too: there a = +-1 exactly, arg = 1e-6f,
        c = logf(1e-6f) = -13.8155..., an ordinary argument of logf.
  y     four float32 operations on stored values: the model's bits.
"""
import math

import numpy as np

import policy_bits as pb
import policy_model as pm

ROOT = pm.ROOT
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
LOG_SQRT_2PI = 0.9189385332046727
EPSILON = 1e-6
F32 = np.float32
ULP = 2.0 ** -23
U_ULPS, A_ULPS, C_ULPS = 4.0, 2.5, 2.5


# ---- SB3's expressions, float64 ------------------------------------------------------------------------------------------------------
def clamp_log_std64(log_std):
    return np.clip(np.asarray(log_std, np.float64), LOG_STD_MIN, LOG_STD_MAX)


def sb3_log_prob64(mean, log_std, gaussian_actions) -> np.ndarray:
    """`SquashedDiagGaussianDistribution.log_prob(actions, gaussian_actions)`: Normal(mean, std).log_prob(u).sum(1) -
    log(1 - tanh(u)^2 + 1e-6).sum(1), float64, log_std already clamped."""
    m, ls, u = (np.asarray(v, np.float64) for v in (mean, log_std, gaussian_actions))
    sd = np.exp(ls)
    normal = -((u - m) ** 2) / (2.0 * sd ** 2) - ls - LOG_SQRT_2PI
    return normal.sum(1) - np.log(1.0 - np.tanh(u) ** 2 + EPSILON).sum(1)


def log_prob_terms64(log_std, eps, actions):
    """The header's two terms in float64: t = -eps^2 / 2 - ls - log sqrt(2 pi), c = log(1 - a^2 + 1e-6)."""
    ls, e, a = (np.asarray(v, np.float64) for v in (log_std, eps, actions))
    return -0.5 * e * e - ls - LOG_SQRT_2PI, np.log(1.0 - a * a + EPSILON)


def act64(mean, raw_log_std, eps) -> dict:
    """`Actor.get_action_dist_params` behind the heads, then the squashed sample, float64."""
    m, e = np.asarray(mean, np.float64), np.asarray(eps, np.float64)
    ls = clamp_log_std64(raw_log_std)
    u = m + np.exp(ls) * e
    a = np.tanh(u)
    t, c = log_prob_terms64(ls, e, a)
    return {"log_std": ls, "gaussian_actions": u, "actions": a, "log_prob": t.sum(1) - c.sum(1)}


def sb3_target64(rewards, dones, gamma, q, ent_coef, next_log_prob) -> np.ndarray:
    """`SAC.train`: target_q = rewards + (1 - dones) * gamma * (min_c q_c - ent_coef * next_log_prob), float64; q [B, n_critics]."""
    r, d, lp = (np.asarray(v, np.float64).reshape(-1) for v in (rewards, dones, next_log_prob))
    next_q = np.asarray(q, np.float64).min(1) - float(ent_coef) * lp
    return r + (1.0 - d) * float(gamma) * next_q


# ---- the header's float32 chain ------------------------------------------------------------------------------------------------------
def clamp_log_std32(raw) -> np.ndarray:
    """ls = l < -20 ? -20 : (l > 2 ? 2 : l): exact."""
    l = np.asarray(raw, F32)
    with np.errstate(invalid="ignore"):
        return np.where(l < F32(-20.0), F32(-20.0), np.where(l > F32(2.0), F32(2.0), l)).astype(F32)


def lane_sum32(x) -> np.ndarray:
    """S: float32 [E, A] -> float32 [E].  Lane i of 64 adds its columns i, i + 64, ... in ascending order to 0; then the xor butterfly
    s += shuffle_xor(s, 1), 2, 4, 8, 16, 32; lane 0's value (every lane holds the same bits: the butterfly is symmetric)."""
    x = np.asarray(x, F32)
    E, A = x.shape
    lanes = np.zeros((E, 64), F32)
    for j0 in range(0, A, 64):
        w = min(64, A - j0)
        lanes[:, :w] = lanes[:, :w] + x[:, j0:j0 + w]
    idx = np.arange(64)
    for d in (1, 2, 4, 8, 16, 32):
        lanes = (lanes + lanes[:, idx ^ d]).astype(F32)
    return lanes[:, 0]


def sum_depth(A: int) -> int:
    return math.ceil(A / 64) + 6


def terms32(log_std, eps, actions):
    """(t, c) float32 from the device's stored ls, eps and a: the exactly rounded operations in float32 in the header's order, logf in
    float64 rounded to float32."""
    ls, e, a = (np.asarray(v, F32) for v in (log_std, eps, actions))
    t = (pb.fma32(F32(-0.5) * e, e, -ls) - F32(0.9189385332)).astype(F32)
    arg = ((F32(1.0) - a * a).astype(F32) + F32(1e-6)).astype(F32)
    c = np.log(arg.astype(np.float64)).astype(F32)
    return t, c


def log_prob32(log_std, eps, actions) -> np.ndarray:
    t, c = terms32(log_std, eps, actions)
    return (lane_sum32(t) - lane_sum32(c)).astype(F32)


def log_prob_bound(log_std, eps, actions) -> np.ndarray:
    """Per row: what |lp_dev - log_prob32(...)| may reach (the module's docstring)."""
    _, c = terms32(log_std, eps, actions)
    A = c.shape[1]
    sc = np.abs(c.astype(np.float64)).sum(1)
    lp = np.abs(log_prob32(log_std, eps, actions).astype(np.float64))
    return (C_ULPS * ULP + 2 * sum_depth(A) * 2.0 ** -24) * sc + ULP * lp


def u_reference(mean, log_std, eps):
    """(u float64, bound): fmaf(exp(ls), eps, m) on the stored m, ls, eps."""
    m, ls, e = (np.asarray(v, F32).astype(np.float64) for v in (mean, log_std, eps))
    se = np.exp(ls) * e
    u = se + m
    return u, U_ULPS * ULP * np.maximum(np.abs(u), np.abs(se))


def a_reference(gaussian_actions):
    a = np.tanh(np.asarray(gaussian_actions, F32).astype(np.float64))
    return a, A_ULPS * ULP * np.maximum(np.abs(a), 2.0 ** -126)


def target32(rewards, dones, gamma, q, ent_coef, next_log_prob) -> np.ndarray:
    """The header's four float32 operations: p = alpha * lp; v = qmin - p; t = (1 - d) * gamma; y = r + t * v, each rounded on its
    own; q float32 [B, n_critics] (qmin = q_1 < q_0 ? q_1 : q_0)."""
    r, d, lp = (np.asarray(v, F32).reshape(-1) for v in (rewards, dones, next_log_prob))
    q = np.asarray(q, F32)
    qmin = q[:, 0] if q.shape[1] == 1 else np.where(q[:, 1] < q[:, 0], q[:, 1], q[:, 0])
    p = (F32(ent_coef) * lp).astype(F32)
    v = (qmin - p).astype(F32)
    t = ((F32(1.0) - d).astype(F32) * F32(gamma)).astype(F32)
    return (r + (t * v).astype(F32)).astype(F32)


# ---- networks and inputs of the tests ------------------------------------------------------------------------------------------------
TRUNKS = {"one": (), "tanh": (64, 64), "relu": (130, 70)}
ES = (1, 15, 16, 17, 37)  # around the 16-row tile
ACTS = (1, 3, 4, 5, 50, 64, 65, 130, 256)  # the 4-column Philox block; 2A crossing 64 / 128 / 512; a sum that crosses wavefronts
D_SMALL, D_CHUNKED = 7, 131  # below and above the forward's 128-column chunk
SEED, TARGET_SEED = 0x5AC0000012345678, 0x7A26E70000000001


def networks(kind: str, D: int, A: int, n_critics: int = 2, salt: int = 0, log_std_bias=None):
    """(actor layers with the [2A, H] last layer, critics' layers, activation): torch's default initialisation; log_std_bias replaces
    the bias of the log_std rows (to reach the clamp)."""
    rng = np.random.default_rng(100003 * salt + 1009 * D + 17 * A + len(kind))
    hidden = TRUNKS[kind]
    actor = pm.random_layers(rng, (D,) + hidden + (2 * A,))
    if log_std_bias is not None:
        w, b = actor[-1]
        b = b.copy()
        b[A:] = np.asarray(log_std_bias, np.float32)
        actor[-1] = (w, b)
    critics = [pm.random_layers(rng, (D + A,) + hidden + (1,)) for _ in range(n_critics)]
    return actor, critics, "relu" if kind == "relu" else "tanh"


def observations(E: int, D: int, salt: int = 0) -> np.ndarray:
    return np.clip(np.random.default_rng(77 + salt + 13 * E + D).standard_normal((E, D)) * 3, -10, 10).astype(np.float32)


def sac_state_dict(actor, critics, target_critics=None) -> dict:
    """An SB3 SAC policy's state dict from an actor whose last layer is [2A, H]: split into actor.mu / actor.log_std."""
    sd = {}
    for i, (w, b) in enumerate(actor[:-1]):
        sd[f"actor.latent_pi.{2 * i}.weight"], sd[f"actor.latent_pi.{2 * i}.bias"] = w, b
    w, b = actor[-1]
    A = w.shape[0] // 2
    sd["actor.mu.weight"], sd["actor.mu.bias"] = w[:A], b[:A]
    sd["actor.log_std.weight"], sd["actor.log_std.bias"] = w[A:], b[A:]
    for prefix, nets in (("critic", critics), ("critic_target", target_critics if target_critics is not None else critics)):
        for k, qf in enumerate(nets):
            for i, (w, b) in enumerate(qf):
                sd[f"{prefix}.qf{k}.{2 * i}.weight"], sd[f"{prefix}.qf{k}.{2 * i}.bias"] = w, b
    return sd
