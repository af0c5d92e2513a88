"""NumPy restatement of stable-baselines3 2.3.2 `RolloutBuffer` (common/buffers.py), written from its published semantics: the model
fleet_rollout.hip is held to, bit for bit.  Everything is float32, as SB3's arrays are; scalars enter the arithmetic as float32
(NumPy treats SB3's Python floats as weak scalars next to float32 arrays), the product gamma * gae_lambda is formed in float64 first,
as Python forms it, and rounded once.
"""
import numpy as np

ALIGN = 256
ARRAYS = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


def layout(E, K, D, A):
    """Bytes and offsets of the device allocation (include/fleet_hip.h FleetRolloutLayout): the eight arrays in the order of ARRAYS,
    each at the next multiple of 256 bytes, then the error word in an aligned block of its own."""
    row = {"obs": E * D * 4, "actions": E * A * 4, "episode_starts": E}
    out, off = {}, 0
    for n in ARRAYS:
        rb = row.get(n, E * 4)
        out[n] = {"offset": off, "bytes": rb * K, "row_bytes": rb}
        off = -(-(off + rb * K) // ALIGN) * ALIGN
    out["error_offset"] = off
    out["total_bytes"] = off + ALIGN
    return out


def gae(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda):
    """compute_returns_and_advantage: (advantages, returns), float32 [K, E]."""
    f = np.float32
    rewards, values = np.asarray(rewards, f), np.asarray(values, f)
    K = rewards.shape[0]
    g, gl = f(gamma), f(float(gamma) * float(gae_lambda))
    adv = np.zeros_like(rewards)
    last = np.zeros(rewards.shape[1], f)
    for t in reversed(range(K)):
        if t == K - 1:
            nnt = f(1) - (np.asarray(dones) != 0).astype(f)
            nv = np.asarray(last_values, f).reshape(-1)
        else:
            nnt = f(1) - (np.asarray(episode_starts[t + 1]) != 0).astype(f)
            nv = values[t + 1]
        delta = (rewards[t] + (g * nv) * nnt) - values[t]
        last = delta + (gl * nnt) * last
        adv[t] = last
    assert adv.dtype == f and last.dtype == f
    return adv, adv + values


def swap_and_flatten(a):
    """SB3's view for sampling: [K, E, ...] -> [E * K, ...], flat index i = e * K + t."""
    a = np.asarray(a)
    return a.swapaxes(0, 1).reshape(a.shape[0] * a.shape[1], *a.shape[2:])


class RolloutModel:
    def __init__(self, E, K, D, A, gamma=0.99, gae_lambda=0.95):
        self.E, self.K, self.D, self.A, self.gamma, self.gae_lambda = E, K, D, A, gamma, gae_lambda
        f = np.float32
        self.obs, self.actions = np.zeros((K, E, D), f), np.zeros((K, E, A), f)
        self.rewards, self.values, self.log_probs = np.zeros((K, E), f), np.zeros((K, E), f), np.zeros((K, E), f)
        self.advantages, self.returns = np.zeros((K, E), f), np.zeros((K, E), f)
        self.episode_starts = np.zeros((K, E), np.uint8)
        self.pos = 0

    def add(self, obs, actions, reward, episode_start, value, log_prob, terminal_value=None, done=None):
        t, f = self.pos, np.float32
        self.obs[t], self.actions[t] = obs, actions
        r = np.asarray(reward).astype(f)  # rounded once
        if terminal_value is not None:
            d = np.asarray(done) != 0
            r = np.where(d, r + f(self.gamma) * np.asarray(terminal_value, f), r).astype(f)
        self.rewards[t], self.episode_starts[t] = r, episode_start
        self.values[t], self.log_probs[t] = np.asarray(value, f).reshape(-1), log_prob
        self.pos += 1

    def compute_returns_and_advantage(self, last_values, dones):
        self.advantages, self.returns = gae(self.rewards, self.values, self.episode_starts, last_values, dones, self.gamma,
                                            self.gae_lambda)

    def sample(self, indices):
        """get()'s rows for flat indices: (obs, actions, values, log_probs, advantages, returns)."""
        return tuple(swap_and_flatten(a)[indices] for a in (self.obs, self.actions, self.values, self.log_probs, self.advantages,
                                                            self.returns))
