"""NumPy restatement of stable-baselines3 2.3.2 `ReplayBuffer` (common/buffers.py, optimize_memory_usage=False), written from its
published semantics: the model fleet_replay.hip is held to, bit for bit.

  add            the ring: row pos <- (obs, next_obs with the terminal rows of done envs, action, float32(reward), done, timeout)
  get_samples    `_get_samples`: rows picked by (row, env) pairs, observations and rewards normalised at sample time with the
                 statistics handed in (`_normalize_obs` / `_normalize_reward`, the float64 arithmetic of fleet_norm.hip), dones
                 as done * (1 - timeout)
  philox4x32_10  the counter-based generator of Salmon et al. (SC'11), with Python integers
  draw           the device's index draw: one block per sample, two 64-bit multiply-highs
"""
import numpy as np

import vecnorm_model as vm

ALIGN = 256
ARRAYS = ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")
M32 = 0xFFFFFFFF


def rows_of(buffer_size, E):
    return max(buffer_size // E, 1)


def layout(buffer_size, E, D, A):
    """Bytes and offsets of the device allocation (include/fleet_hip.h FleetReplayLayout): the six arrays in the order of ARRAYS,
    each at the next multiple of 256 bytes, then the error word in an aligned block of its own."""
    R = rows_of(buffer_size, E)
    row = {"observations": E * D * 4, "next_observations": E * D * 4, "actions": E * A * 4, "rewards": E * 4, "dones": E, "timeouts": E}
    out, off = {"rows": R}, 0
    for n in ARRAYS:
        out[n] = {"offset": off, "bytes": row[n] * R, "row_bytes": row[n]}
        off = -(-(off + row[n] * R) // ALIGN) * ALIGN
    out["error_offset"] = off
    out["total_bytes"] = off + ALIGN
    return out


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """The block (x0, x1, x2, x3) of a 4 x 32-bit counter under a 2 x 32-bit key."""
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def mulhi64(x, n):
    """floor(x * n / 2^64) for 0 <= x < 2^64: in [0, n), never n."""
    return (int(x) * int(n)) >> 64


def draw_one(seed, call, b, upper, E):
    x = philox4x32_10((b, 0, call & M32, (call >> 32) & M32), (seed & M32, (seed >> 32) & M32))
    return mulhi64(x[0] | (x[1] << 32), upper), mulhi64(x[2] | (x[3] << 32), E)


def _philox_vec(c0, c2, c3, seed):
    """philox4x32_10 over arrays of counters (c0, 0, c2, c3), uint64 arithmetic on 32-bit values."""
    u = np.uint64
    c0 = np.asarray(c0, dtype=u)
    c1 = np.zeros_like(c0)
    c2, c3 = np.full_like(c0, c2), np.full_like(c0, c3)
    k0, k1 = int(seed) & M32, (int(seed) >> 32) & M32
    m, s = u(M32), u(32)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2  # 32 x 32 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ u(k0), p1 & m, (p0 >> s) ^ c3 ^ u(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def _mulhi64_vec(lo, hi, n):
    """floor((lo | hi << 32) * n / 2^64) for n < 2^32, from 32-bit limbs."""
    u = np.uint64
    n = u(n)
    t = (lo * n) >> u(32)
    return (hi * n + t) >> u(32)


def draw(seed, call, B, upper, E):
    """(rows, envs) int32 [B] of minibatch number `call`."""
    x0, x1, x2, x3 = _philox_vec(np.arange(B), call & M32, (call >> 32) & M32, seed)
    return _mulhi64_vec(x0, x1, upper).astype(np.int32), _mulhi64_vec(x2, x3, E).astype(np.int32)


# ---- the buffer ----------------------------------------------------------------------------------------------------------------
def normalize_obs(x, mean, var, clip_obs, epsilon):
    y = (np.asarray(x, np.float32).astype(np.float64) - mean) / np.sqrt(var + epsilon)
    return vm.clip(y, clip_obs).astype(np.float32)


def normalize_reward(r, ret_var, clip_reward, epsilon):
    y = np.asarray(r, np.float32).astype(np.float64) / np.sqrt(np.float64(ret_var) + epsilon)
    return vm.clip(y, clip_reward).astype(np.float32)


class ReplayModel:
    def __init__(self, buffer_size, E, D, A, seed=0):
        self.E, self.D, self.A, self.seed = E, D, A, seed
        self.R = R = rows_of(buffer_size, E)
        f = np.float32
        self.observations, self.next_observations = np.zeros((R, E, D), f), np.zeros((R, E, D), f)
        self.actions, self.rewards = np.zeros((R, E, A), f), np.zeros((R, E), f)
        self.dones, self.timeouts = np.zeros((R, E), np.uint8), np.zeros((R, E), np.uint8)
        self.pos, self.full, self.calls = 0, False, 0

    def add(self, obs, next_obs, action, reward, done, terminal=None, timeout=None):
        p = self.pos
        d = np.asarray(done) != 0
        self.observations[p] = obs
        nxt = np.array(next_obs, np.float32, copy=True)
        if terminal is not None and d.any():
            nxt[d] = np.asarray(terminal)[d]  # the other terminal rows are never read
        self.next_observations[p] = nxt
        self.actions[p] = action
        self.rewards[p] = np.asarray(reward).astype(np.float32)  # rounded once
        self.dones[p] = d
        self.timeouts[p] = 0 if timeout is None else timeout
        self.pos += 1
        if self.pos == self.R:
            self.pos, self.full = 0, True

    def upper(self):
        return self.R if self.full else self.pos

    def arrays(self):
        return {n: getattr(self, n) for n in ARRAYS}

    def get_samples(self, rows, envs, stats=None):
        """(observations, actions, next_observations, dones [B,1], rewards [B,1]).  stats: None, or a dict with obs_mean, obs_var,
        ret_var (float64), norm_obs, norm_reward, clip_obs, clip_reward, epsilon."""
        rows, envs = np.asarray(rows), np.asarray(envs)
        o, n = self.observations[rows, envs], self.next_observations[rows, envs]
        r = self.rewards[rows, envs]
        if stats is not None and stats["norm_obs"]:
            o = normalize_obs(o, stats["obs_mean"], stats["obs_var"], stats["clip_obs"], stats["epsilon"])
            n = normalize_obs(n, stats["obs_mean"], stats["obs_var"], stats["clip_obs"], stats["epsilon"])
        if stats is not None and stats["norm_reward"]:
            r = normalize_reward(r, stats["ret_var"], stats["clip_reward"], stats["epsilon"])
        d = self.dones[rows, envs].astype(np.float32) * (np.float32(1) - self.timeouts[rows, envs].astype(np.float32))
        return o, self.actions[rows, envs], n, d.reshape(-1, 1), r.reshape(-1, 1)

    def sample(self, B, stats=None):
        rows, envs = draw(self.seed, self.calls, B, self.upper(), self.E)
        self.calls += 1
        return self.get_samples(rows, envs, stats), rows, envs
