"""Restatement of include/fleet_hip.h "collect_rollouts on the device" (fleet_collect_*, fleetrl_amd/csrc/fleet_collect.hip) for the
tests: the episode ring -- SB3's ep_info_buffer, a deque(maxlen = W) extended over the step's finished envs in env order, and the slot
rule the kernel places them by -- and the closing launch's statistics block with its ordered sum S."""
import os
from collections import deque

import numpy as np

import train_model as tm

ROOT = tm.ROOT
F64 = np.float64
LANES = tm.LANES                  # fleet_collect.h: kCollectThreads
SCAN_THREADS = 1024               # kCollectScanThreads: one chunk of envs
MAX_WINDOW, STATS_LEN = 4096, 16  # FLEET_COLLECT_MAX_WINDOW, FLEET_COLLECT_STATS
STATS = ("ep_rew_mean", "ep_len_mean", "episodes", "total_episodes", "num_steps")


def slot_rule(count: int, c: int, k: int, W: int):
    """(kept, slot) of the k-th of a step's c finished envs, the ring having taken `count` episodes before: the header's line."""
    return c - k <= W, (count + k) % W


class Ring:
    """The device's ring by the slot rule: ring_return f64[W], ring_length i32[W], count, and the episodes since the last finish."""

    def __init__(self, W: int):
        self.W, self.count, self.since = int(W), 0, 0
        self.ret, self.len = np.zeros(W, F64), np.zeros(W, np.int32)

    def step(self, done, ep_return, ep_len):
        idx = np.flatnonzero(np.asarray(done))  # ascending env id
        c = idx.size
        for k, e in enumerate(idx):
            kept, slot = slot_rule(self.count, c, k, self.W)
            if kept:
                self.ret[slot], self.len[slot] = ep_return[e], ep_len[e]
        self.count += c
        self.since += c

    def window(self):
        """(returns, lengths) of the last min(count, W) episodes, oldest first."""
        n = min(self.count, self.W)
        order = [(self.count - n + i) % self.W for i in range(n)]
        return self.ret[order], self.len[order]

    def finish(self, first_step: int = 0, steps: int = 0) -> np.ndarray:
        """The statistics block f64[16]: S over the slots 0 .. n-1 (by slot, not by age), the means, the counts."""
        out = np.zeros(STATS_LEN, F64)
        n = min(self.count, self.W)
        if n:
            out[0] = tm.tree_sum(self.ret[:n]) / F64(n)
            out[1] = tm.tree_sum(self.len[:n].astype(F64)) / F64(n)
        else:
            out[0] = out[1] = np.nan
        out[2], out[3], out[4] = F64(self.since), F64(self.count), F64(first_step + steps)
        self.since = 0
        return out


class Sb3Buffer:
    """What SB3 keeps: `_update_info_buffer` extends ep_info_buffer = deque(maxlen = stats_window_size) with info["episode"] of every
    env whose info carries one, walking `infos` in env order."""

    def __init__(self, W: int):
        self.buf = deque(maxlen=int(W))

    def step(self, done, ep_return, ep_len):
        self.buf.extend((float(ep_return[e]), int(ep_len[e])) for e in range(len(done)) if done[e])

    def window(self):
        return np.array([r for r, _ in self.buf], F64), np.array([n for _, n in self.buf], np.int32)


def launches_ppo(K: int, with_norm: bool) -> int:
    """5 K + 3 with a normaliser, 4 K + 3 without: explore, step, [normalise], add, episodes per step; forward, GAE, the closing launch."""
    return (5 if with_norm else 4) * K + 3


def launches_offpolicy(n_steps: int, with_norm: bool, first_step: int = 0, learning_starts: int = 0, with_noise: bool = False) -> int:
    """4 per step and the closing launch; one more per step with a normaliser, one more per step that asks the noise handle."""
    asks = sum(1 for t in range(n_steps) if with_noise and first_step + t >= learning_starts)
    return (5 if with_norm else 4) * n_steps + asks + 1


assert os.path.isdir(ROOT)
