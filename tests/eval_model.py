"""Restatement of include/fleet_hip.h "evaluation of the agent on the device" (fleet_eval_*, fleetrl_amd/csrc/fleet_eval.hip) for the
tests: the bookkeeping launch -- stable-baselines3 2.3.2 evaluate_policy's inner loop over one step of a vectorised env --, the closing
launch's statistics block with its ordered sum S, and the gate of EvalCallback's "new best"."""
import os

import numpy as np

import train_model as tm

ROOT = tm.ROOT
F64 = np.float64
LANES = tm.LANES                     # fleet_eval.h: kEvalThreads
SCAN_THREADS = 1024                  # kEvalScanThreads: one chunk of envs
MAX_EPISODES, STATS_LEN = 65536, 16  # FLEET_EVAL_MAX_EPISODES, FLEET_EVAL_STATS
STATS = ("mean_reward", "std_reward", "mean_ep_length", "std_ep_length", "episodes", "best_mean_reward", "new_best", "num_timesteps",
         "evaluations")


def targets(n_eval_episodes: int, E: int) -> np.ndarray:
    """SB3: episode_count_targets = [(n_eval_episodes + i) // n_envs for i in range(n_envs)]."""
    return np.array([(n_eval_episodes + i) // E for i in range(E)], dtype=np.int64)


class Evaluation:
    """The handle's bookkeeping: sums f64[E], lengths i32[E], counts i32[E], the lists of max_episodes slots and their count; the best
    mean so far, the gate and the number of evaluations."""

    def __init__(self, E: int, max_episodes: int):
        self.E, self.M = int(E), int(max_episodes)
        self.sums, self.lengths, self.counts = np.zeros(E, F64), np.zeros(E, np.int32), np.zeros(E, np.int32)
        self.ep_reward, self.ep_length, self.listed = np.zeros(self.M, F64), np.zeros(self.M, np.int32), 0
        self.best, self.gate, self.evaluations = F64(-np.inf), 0, 0

    def clear(self):
        self.sums[:], self.lengths[:], self.counts[:], self.listed = 0.0, 0, 0, 0

    def step(self, done, reward, n_eval_episodes: int, source: int = 0, ep_return=None, ep_len=None):
        """One step of E' = len(done) <= E envs, the header's lines: every env's sum and length move on; an env below its target that
        finished takes slot listed + k (k: its rank among them, ascending env id) and starts afresh."""
        E = len(done)
        want = targets(n_eval_episodes, E)
        k = 0
        for i in range(E):
            s = self.sums[i] + F64(reward[i])
            n = self.lengths[i] + np.int32(1)
            if self.counts[i] < want[i] and done[i]:
                slot = self.listed + k
                if slot < self.M:
                    self.ep_reward[slot] = F64(ep_return[i]) if source else s
                    self.ep_length[slot] = np.int32(ep_len[i]) if source else n
                k += 1
                self.counts[i] += 1
                s, n = F64(0.0), np.int32(0)
            self.sums[i], self.lengths[i] = s, n
        self.listed += k

    def lists(self):
        n = min(self.listed, self.M)
        return self.ep_reward[:n].copy(), self.ep_length[:n].copy()

    def finish(self, num_timesteps: int = 0) -> np.ndarray:
        """The statistics block f64[16], the gate and the best."""
        out = np.zeros(STATS_LEN, F64)
        r, n_len = self.lists()
        out[0:4] = mean_std(r) + mean_std(n_len.astype(F64))
        out[4] = F64(r.size)
        self.gate = int(new_best(out[0], self.best))
        if self.gate:
            self.best = out[0]
        self.evaluations += 1
        out[5], out[6], out[7], out[8] = self.best, F64(self.gate), F64(num_timesteps), F64(self.evaluations)
        return out


def mean_std(x) -> tuple:
    """(S(x) / n, sqrt(S((x - mean)^2) / n)) with S the ordered float64 sum (train_model.tree_sum); NaN, NaN for n == 0."""
    x = np.asarray(x, dtype=F64)
    n = x.size
    if n == 0:
        return F64(np.nan), F64(np.nan)
    mean = tm.tree_sum(x) / F64(n)
    d = x - mean
    return mean, np.sqrt(tm.tree_sum(d * d) / F64(n))


def new_best(mean, best) -> bool:
    """EvalCallback: `if mean_reward > self.best_mean_reward` -- false for an equal mean and for NaN."""
    return bool(mean > best)


def sb3_evaluate(steps, n_eval_episodes: int):
    """stable_baselines3/common/evaluation.py (2.3.2) written out per env for an env without Monitor: `steps` yields (rewards [E], dones
    [E]) per env step; returns (episode_rewards, episode_lengths) once every quota is met or the steps run out."""
    episode_rewards, episode_lengths = [], []
    current_rewards = current_lengths = episode_counts = episode_count_targets = None
    for rewards, dones in steps:
        n_envs = len(dones)
        if current_rewards is None:
            episode_counts = np.zeros(n_envs, dtype="int")
            episode_count_targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")
            current_rewards, current_lengths = np.zeros(n_envs), np.zeros(n_envs, dtype="int")
        if not (episode_counts < episode_count_targets).any():
            break
        current_rewards += rewards
        current_lengths += 1
        for i in range(n_envs):
            if episode_counts[i] < episode_count_targets[i]:
                if dones[i]:
                    episode_rewards.append(current_rewards[i])
                    episode_lengths.append(current_lengths[i])
                    episode_counts[i] += 1
                    current_rewards[i] = 0
                    current_lengths[i] = 0
    return episode_rewards, episode_lengths


def launches(n_steps: int, with_norm: bool, with_sync: bool = False) -> int:
    """4 n + 5 with a normaliser, 3 n + 4 without, one more with a sync: forward, step, [normalise], bookkeeping per step; reset,
    [normaliser's reset], clear, the closing launch, the snapshot."""
    return (4 if with_norm else 3) * n_steps + (5 if with_norm else 4) + (1 if with_sync else 0)


assert os.path.isdir(ROOT)
