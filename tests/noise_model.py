"""float64 NumPy model of the correlated noise processes (include/fleet_hip.h "correlated action noise on the device"): the Philox
counter scheme, the gain and twiddle tables, one pink sequence as the direct sum and -- separately -- through np.fft.irfft of the
colorednoise recipe, the (t, q) state machine with done flags and exhaustion, and the Ornstein-Uhlenbeck recursion.  The generator
is `replay_model.philox4x32_10` (`philox` is the same function over arrays, held to it by tests/test_noise_cpu.py), the uniforms and
Box-Muller are explore_model's.  Nothing here needs a GPU or the library."""
import numpy as np

import explore_model as em
import replay_model as rp

M32 = rp.M32
PINK_TAG, OU_TAG = 0x80000000, 0x40000000
SEED = em.SEED
NS = (2, 3, 7, 64, 65, 192, 193)
# the lengths past one block of samples (64 x 4 per lane trip: n > 256) and past one chunk of staged frequencies (K = n / 2 + 1 > 256)
NS_WIDE = (256, 257, 320, 386, 510, 511, 512, 513, 1030, 4096)
BETAS = (0.0, 1.0, 2.0)
NOISE_BOUND = 1e-5  # |eps_dev - eps_model| of one Box-Muller normal, as test_explore_gpu.test_drawn_noise_equals_the_model holds it
CHUNK = 256  # frequencies the device stages at a time (fleet_noise.hip kChunk)


# ---- draws -----------------------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, seed) -> np.ndarray:
    """philox4x32_10 over broadcastable arrays of counter words under key (seed lo, seed hi): uint64 [..., 4]."""
    u = np.uint64
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.int64) & M32 for c in (c0, c1, c2, c3)))
    c0, c1, c2, c3 = (c.astype(u) for c in (c0, c1, c2, c3))
    k0, k1 = em.key(seed)
    m, s = u(M32), u(32)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ u(k0), p1 & m, (p0 >> s) ^ c3 ^ u(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def normals4(w) -> np.ndarray:
    """[..., 4] words -> [..., 4] standard normals: Box-Muller on (x0, x1) and (x2, x3), cosine first."""
    r = np.sqrt(-2.0 * np.log(em.u_open_low(w[..., 0::2])))
    t = 2.0 * np.pi * em.u_open_high(w[..., 1::2])
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=-1).reshape(w.shape)


def pink_counter(env, column, q, k):
    return int(env) & M32, PINK_TAG | (int(column) // 2), int(q) & M32, int(k) & M32


def ou_counter(env, column, calls):
    return int(env) & M32, OU_TAG | (int(column) // 4), int(calls) & M32, (int(calls) >> 32) & M32


def pink_coefficients(seed, env_ids, A, q, n):
    """(a, b) float64 [E, A, K]: the spectral coefficients of every (env, column) for sequence number q[e] (unit variance, b as drawn:
    the zeros at k = 0 and 2k = n are the sum's business)."""
    env_ids, q = np.asarray(env_ids, dtype=np.int64), np.broadcast_to(np.asarray(q, dtype=np.int64), (len(env_ids),))
    K, P = n // 2 + 1, (A + 1) // 2
    w = philox(env_ids[:, None, None], (PINK_TAG | np.arange(P))[None, :, None], q[:, None, None], np.arange(K)[None, None, :], seed)
    z = normals4(w)  # [E, P, K, 4]
    a = np.stack([z[..., 0], z[..., 2]], axis=2).reshape(len(env_ids), 2 * P, K)[:, :A]
    b = np.stack([z[..., 1], z[..., 3]], axis=2).reshape(len(env_ids), 2 * P, K)[:, :A]
    return a, b


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def spectrum_scale(n, beta):
    """(s [K], sigma) of colorednoise.powerlaw_psd_gaussian(beta, n)."""
    K = n // 2 + 1
    f = np.arange(K, dtype=np.float64) / n
    f[0] = f[1]
    s = f ** (-beta / 2.0)
    w = s[1:].copy()
    w[-1] *= (1 + (n % 2)) / 2.0
    return s, 2.0 * np.sqrt(np.sum(w ** 2)) / n


def tables(n, beta):
    """(gain [K], twiddle [n, 2]) in float64."""
    s, sigma = spectrum_scale(n, beta)
    K = len(s)
    weight = np.full(K, 2.0)
    weight[0] = np.sqrt(2.0)
    if n % 2 == 0:
        weight[-1] = np.sqrt(2.0)
    ang = 2.0 * np.pi * np.arange(n) / n
    return weight * s / (n * sigma), np.stack([np.cos(ang), np.sin(ang)], axis=1)


def tables32(n, beta):
    g, tw = tables(n, beta)
    return g.astype(np.float32), tw.astype(np.float32)


def real_only(n):
    """[K] bool: the frequencies whose imaginary coefficient is zero."""
    k = np.arange(n // 2 + 1)
    return (k == 0) | (2 * k == n)


# ---- one sequence ----------------------------------------------------------------------------------------------------------------
def direct_sum(a, b, n, beta, gain=None, twiddle=None):
    """y [..., n] = sum_k gain[k] (a_k cos[m] - b_k sin[m]), m = (k t) mod n, from coefficients [..., K]; with the float32 tables
    given, the sum the device evaluates, in float64."""
    g, tw = tables(n, beta)
    g = g if gain is None else np.asarray(gain, dtype=np.float64)
    tw = tw if twiddle is None else np.asarray(twiddle, dtype=np.float64)
    K = n // 2 + 1
    m = (np.arange(K)[:, None] * np.arange(n)[None, :]) % n  # [K, n]
    bz = np.where(real_only(n), 0.0, b)
    return (a * g) @ tw[m, 0] - (bz * g) @ tw[m, 1]


def irfft_form(a, b, n, beta):
    """The colorednoise recipe as written: scale by s, sqrt(2) on the real-only terms, irfft, divide by sigma."""
    s, sigma = spectrum_scale(n, beta)
    sr, si = a * s, b * s
    si = np.where(real_only(n), 0.0, si)
    sr = np.where(real_only(n), np.sqrt(2.0) * sr, sr)
    return np.fft.irfft(sr + 1j * si, n=n, axis=-1) / sigma


def variance(n, beta):
    """Var(y[t]) exactly, the same for every t: sum of gain^2."""
    return float(np.sum(tables(n, beta)[0] ** 2))


def correlation(n, beta, lag):
    g2 = tables(n, beta)[0] ** 2
    return float(np.sum(g2 * np.cos(2.0 * np.pi * np.arange(len(g2)) * lag / n)) / np.sum(g2))


def periodogram_expectation(n, beta):
    """(E |Y_k|^2, its standard deviation) [K] for Y = rfft(y): n^2 gain^2 / 2 x chi^2_2 inside, n^2 gain^2 x chi^2_1 at k = 0 and 2k = n."""
    g2 = n * n * tables(n, beta)[0] ** 2
    edge = real_only(n)
    return np.where(edge, g2, g2 / 2.0), np.where(edge, np.sqrt(2.0) * g2, g2 / 2.0)


# ---- the float32 chain and the tolerance it gives -----------------------------------------------------------------------------------
FAULTS = ("drop_last", "drop_chunk_first", "phase_reset")


def chain32(a, b, n, beta, displace=None, fault=None):
    """y [C, n]: the chain fleet_noise.h states, restated in float32 from the model's coefficients a, b [C, K]: coefficients rounded
    to float32, the staged products gain x a and gain x b rounded once, +0 for the imaginary part at k = 0 and 2k = n, k ascending,
    two accumulate steps per k each rounded to float32 once (product and sum formed in float64, then rounded: the device's fmaf
    rounds the exact sum, this the float64 one), the phase m advanced by t modulo n in integers.
    displace: a seed; every normal is moved by a uniform draw within +-NOISE_BOUND before it is rounded, which is what the device's
    Box-Muller may do to it.  fault: one of FAULTS, what the wide lengths exist to catch -- the last frequency dropped, the first
    frequency of the second chunk (k = CHUNK) dropped, the phase walk restarted at k = CHUNK."""
    f32, f64 = np.float32, np.float64
    a, b = np.array(a, dtype=f64), np.array(b, dtype=f64)
    K = n // 2 + 1
    assert a.shape == b.shape and a.ndim == 2 and a.shape[1] == K and fault in (None,) + FAULTS
    if displace is not None:
        rng = np.random.default_rng(displace)
        a += rng.uniform(-NOISE_BOUND, NOISE_BOUND, a.shape)
        b += rng.uniform(-NOISE_BOUND, NOISE_BOUND, b.shape)
    gain, tw = tables32(n, beta)
    ga = (gain[None, :] * a.astype(f32)).astype(f64)  # (float32 x float32 rounded to float32, held in float64)
    gb = (gain[None, :] * b.astype(f32)).astype(f64)
    gb[:, real_only(n)] = 0.0
    cos, sin = tw[:, 0].astype(f64), tw[:, 1].astype(f64)
    t = np.arange(n)
    m, acc = np.zeros(n, np.int64), np.zeros((len(a), n))
    for k in range(K):
        if fault == "phase_reset" and k == CHUNK:
            m[:] = 0
        skip = (fault == "drop_last" and k == K - 1) or (fault == "drop_chunk_first" and k == CHUNK)
        if not skip:
            acc = (acc + ga[:, k, None] * cos[m]).astype(f32).astype(f64)
            acc = (acc - gb[:, k, None] * sin[m]).astype(f32).astype(f64)
        m += t
        m[m >= n] -= n
    return acc


TOL_COLUMNS = (3, 16)  # E x A = 48 columns under SEED, sequence number 0


def chain_errors(n, betas=BETAS, displace=True, fault=None):
    """{beta: max |chain32 - direct_sum over the float32 tables|} over the 48 columns of TOL_COLUMNS; displaced under the seed n.
    With displace and without a fault this is R(n, beta): the reference alone decides it."""
    E, A = TOL_COLUMNS
    a, b = (c.reshape(E * A, -1) for c in pink_coefficients(SEED, np.arange(E), A, 0, n))
    out = {}
    for beta in betas:
        want = direct_sum(a, b, n, beta, *tables32(n, beta))
        out[beta] = float(np.abs(chain32(a, b, n, beta, n if displace else None, fault) - want).max())
    return out


def round_up2(x):
    """x rounded up to two significant digits."""
    e = int(np.floor(np.log10(x))) - 1
    return float(f"{int(np.ceil(x / 10.0 ** e - 1e-9))}e{e}")


# pink_tol(n, beta) = 2 R(n, beta) rounded up to two digits, R = chain_errors(n)[beta].  The factor 2: R is the maximum under ONE
# displacement pattern, not the worst one, and the restatement rounds twice where the device's fmaf rounds once.
# tests/test_noise_cpu.py recomputes every entry, holds it below half the smallest gain, and shows that it sees each of FAULTS.
PINK_TOL_WIDE = {
    (256, 0.0): 4.8e-05, (256, 1.0): 4.5e-05, (256, 2.0): 4.1e-05,
    (257, 0.0): 4.7e-05, (257, 1.0): 4.9e-05, (257, 2.0): 4.8e-05,
    (320, 0.0): 4.6e-05, (320, 1.0): 4.5e-05, (320, 2.0): 4.2e-05,
    (386, 0.0): 5.0e-05, (386, 1.0): 4.9e-05, (386, 2.0): 4.4e-05,
    (510, 0.0): 4.9e-05, (510, 1.0): 5.0e-05, (510, 2.0): 4.4e-05,
    (511, 0.0): 5.0e-05, (511, 1.0): 4.9e-05, (511, 2.0): 4.4e-05,
    (512, 0.0): 4.8e-05, (512, 1.0): 5.1e-05, (512, 2.0): 4.9e-05,
    (513, 0.0): 5.4e-05, (513, 1.0): 5.0e-05, (513, 2.0): 5.3e-05,
    (1030, 0.0): 5.1e-05, (1030, 1.0): 5.5e-05, (1030, 2.0): 4.8e-05,
    (4096, 0.0): 5.7e-05, (4096, 1.0): 5.8e-05, (4096, 2.0): 5.9e-05,
}


def pink_tol(n, beta):
    """|y_dev - y_model| a sample of a wide length is held to."""
    return PINK_TOL_WIDE[(n, float(beta))]


# ---- the processes ---------------------------------------------------------------------------------------------------------------
class PinkModel:
    """The (t, q) state machine over sequences computed on demand; `float32_tables`: the sum over the rounded tables."""

    def __init__(self, E, A, n, beta=1.0, seed=SEED, env_id_offset=0, float32_tables=True):
        self.E, self.A, self.n, self.beta, self.seed = E, A, n, beta, seed
        self.ids = np.arange(E) + env_id_offset
        self.t, self.q = np.zeros(E, np.int32), np.zeros(E, np.uint32)
        self._tables = tables32(n, beta) if float32_tables else tables(n, beta)
        self.cache = np.zeros((E, n, A))
        self._fill(np.ones(E, bool))

    def _fill(self, which):
        idx = np.flatnonzero(which)
        if idx.size:
            a, b = pink_coefficients(self.seed, self.ids[idx], self.A, self.q[idx], self.n)
            self.cache[idx] = np.swapaxes(direct_sum(a, b, self.n, self.beta, *self._tables), 1, 2)

    def _restart(self, which):
        self.q[which] += np.uint32(1)
        self.t[which] = 0
        self._fill(which)

    def reset(self, mask=None):
        self._restart(np.ones(self.E, bool) if mask is None else np.asarray(mask).astype(bool))

    def next(self, done=None):
        again = self.t >= self.n
        if done is not None:
            again = again | np.asarray(done).astype(bool)
        self._restart(again)
        out = self.cache[np.arange(self.E), self.t]
        self.t += 1
        return out


class OUModel:
    def __init__(self, E, A, mu, sigma, theta=0.15, dt=1e-2, seed=SEED, env_id_offset=0):
        self.E, self.A, self.seed, self.ids = E, A, seed, np.arange(E) + env_id_offset
        self.mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (A,)).astype(np.float32).astype(np.float64)
        self.ss = (np.broadcast_to(np.asarray(sigma, dtype=np.float64), (A,)) * np.sqrt(dt)).astype(np.float32).astype(np.float64)
        self.th = float(np.float32(theta * dt))
        self.x, self.calls = np.zeros((E, A)), 0

    def eps(self):
        nb = (self.A + 3) // 4
        _, _, lo, hi = ou_counter(0, 0, self.calls)
        w = philox(self.ids[:, None], (OU_TAG | np.arange(nb))[None, :], lo, hi, self.seed)
        return normals4(w).reshape(self.E, -1)[:, :self.A]

    def reset(self, mask=None):
        self.x[np.ones(self.E, bool) if mask is None else np.asarray(mask).astype(bool)] = 0.0

    def next(self, done=None):
        if done is not None:
            self.reset(done)
        self.x = self.x + self.th * (self.mu - self.x) + self.ss * self.eps()
        self.calls += 1
        return self.x.copy()
