"""`DeviceRolloutBuffer`: stable-baselines3 2.3.2 `RolloutBuffer` in device memory.

PPO's rollout storage, its advantages / returns (GAE) and its minibatch sampling, on the GPU (fleetrl_amd/csrc/fleet_rollout.hip,
include/fleet_hip.h `fleet_rollout_*`): `FleetVecEnv.step_torch` and `FleetVecNormalize.step_torch` write a step's observations and
dones straight into the buffer's rows (`slot(t)`), `add` stores the rest in one launch, `compute_returns_and_advantage` is one
launch, and `get` yields minibatches gathered by one launch each.  Nothing crosses to the host.  Semantics are SB3's: float32
arrays, time-major [n_steps, num_envs, ...], flat sample indices in `swap_and_flatten` order (i = env * n_steps + t).  The
policy network, the optimiser and PPO itself are the caller's (examples/ppo_device_loop.py).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from . import _capi
from ._capi import FleetHipError
from ._handle import _DeviceHandle

__all__ = ["DeviceRolloutBuffer", "RolloutBatch", "RolloutSlot"]

# SB3's RolloutBufferSamples
RolloutBatch = namedtuple("RolloutBatch", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])
RolloutSlot = namedtuple("RolloutSlot", ["obs", "actions", "reward", "episode_start", "value", "log_prob"])


class DeviceRolloutBuffer(_DeviceHandle):
    """One `fleet_rollout_*` handle.  The `*_dev` methods take raw device addresses; every other method takes torch tensors on
    the buffer's device and launches on torch's current stream."""
    _prefix = "rollout"

    def __init__(self, num_envs: int, n_steps: int, obs_dim: int, act_dim: int, gamma: float = 0.99, gae_lambda: float = 0.95,
                 device: int = 0):
        self.num_envs, self.n_steps, self.obs_dim, self.act_dim = int(num_envs), int(n_steps), int(obs_dim), int(act_dim)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        p = _capi.FleetRolloutParams(C.sizeof(_capi.FleetRolloutParams), self.num_envs, self.n_steps, self.obs_dim, self.act_dim, 0,
                                     self.gamma, self.gae_lambda)
        self._open(device, p)
        self.pos, self.full = 0, False

    # ---- device pointers ------------------------------------------------------------------------------------------------
    def arrays_dev(self) -> dict:
        """name -> base address of the eight arrays."""
        a = _capi.FleetRolloutArrays()
        self._check(self.lib.fleet_rollout_arrays(self.h, C.byref(a)))
        return {n: getattr(a, n) for n in _capi.ROLLOUT_ARRAY_NAMES}

    def slot_dev(self, t: int) -> _capi.FleetRolloutSlot:
        s = _capi.FleetRolloutSlot()
        self._check(self.lib.fleet_rollout_slot(self.h, int(t), C.byref(s)))
        return s

    def add_dev(self, t: int, obs_ptr: int, actions_ptr: int, reward_ptr: int, reward_dtype: int, episode_start_ptr: int,
                value_ptr: int, log_prob_ptr: int, terminal_value_ptr: int | None = None, done_ptr: int | None = None):
        self._check(self.lib.fleet_rollout_add_dev(self.h, int(t), obs_ptr, actions_ptr, reward_ptr, int(reward_dtype),
                                                   episode_start_ptr, value_ptr, log_prob_ptr, terminal_value_ptr, done_ptr))

    def finish_dev(self, last_values_ptr: int, dones_ptr: int):
        self._check(self.lib.fleet_rollout_finish_dev(self.h, last_values_ptr, dones_ptr))

    def gather_dev(self, indices_ptr: int, batch: int, obs_ptr=None, actions_ptr=None, values_ptr=None, log_probs_ptr=None,
                   advantages_ptr=None, returns_ptr=None):
        self._check(self.lib.fleet_rollout_gather_dev(self.h, indices_ptr, int(batch), obs_ptr, actions_ptr, values_ptr,
                                                      log_probs_ptr, advantages_ptr, returns_ptr))

    def check_errors(self):
        """Waits for the buffer's stream; raises FleetHipError (ERR_STATE) once if a gather met an index out of range."""
        self._check(self.lib.fleet_rollout_check_errors(self.h))

    # ---- the arrays as torch tensors (zero-copy views of the buffer's memory) -------------------------------------------------
    def _views(self) -> dict:
        if self._tensors is None:
            K, E, D, A = self.n_steps, self.num_envs, self.obs_dim, self.act_dim
            shapes = {"obs": (K, E, D), "actions": (K, E, A)}
            self._tensors = self._make_views({n: (shapes.get(n, (K, E)), "|u1" if n == "episode_starts" else "<f4")
                                              for n in _capi.ROLLOUT_ARRAY_NAMES})
        return self._tensors

    observations = property(lambda self: self._views()["obs"], doc="f32 [n_steps, num_envs, obs_dim]")
    actions = property(lambda self: self._views()["actions"], doc="f32 [n_steps, num_envs, act_dim]")
    rewards = property(lambda self: self._views()["rewards"], doc="f32 [n_steps, num_envs]")
    episode_starts = property(lambda self: self._views()["episode_starts"], doc="u8 [n_steps, num_envs]")
    values = property(lambda self: self._views()["values"], doc="f32 [n_steps, num_envs]")
    log_probs = property(lambda self: self._views()["log_probs"], doc="f32 [n_steps, num_envs]")
    advantages = property(lambda self: self._views()["advantages"], doc="f32 [n_steps, num_envs]")
    returns = property(lambda self: self._views()["returns"], doc="f32 [n_steps, num_envs]")

    def slot(self, t: int) -> RolloutSlot:
        """Views of time row t, for writing in place: pass `.obs` / `.episode_start` as obs_out / done_out of the step that
        produces the row, then the same tensors to `add`, which leaves them alone."""
        if not 0 <= t < self.n_steps:
            raise IndexError(f"slot {t} of a buffer of {self.n_steps} steps")
        v = self._views()
        return RolloutSlot(v["obs"][t], v["actions"][t], v["rewards"][t], v["episode_starts"][t], v["values"][t], v["log_probs"][t])

    # ---- SB3's surface ----------------------------------------------------------------------------------------------------
    def reset(self):
        """Start a new rollout at row 0 (the rows are overwritten as they are added, not cleared)."""
        self.pos, self.full = 0, False

    def add(self, obs, action, reward, episode_start, value, log_prob, terminal_value=None, done=None):
        """SB3's add: row `pos` <- the step's tensors (value may be [E, 1] as a critic returns it; reward float64 or float32,
        rounded once to float32).  terminal_value [E] with done [E]: SB3's time-limit bootstrap, reward += gamma * terminal_value
        on done envs (off by default, as in the reference)."""
        import torch

        if self.full:
            raise FleetHipError(_capi.ERR_STATE, "the rollout buffer is full: reset() starts the next rollout")
        self.use_torch_stream()
        E, D, A = self.num_envs, self.obs_dim, self.act_dim
        f32, u8 = (torch.float32,), (torch.uint8,)
        obs, action = self._tensor(obs, (E, D), f32), self._tensor(action, (E, A), f32)
        reward = self._tensor(reward, (E,), (torch.float64, torch.float32))
        episode_start, value, log_prob = self._tensor(episode_start, (E,), u8), self._tensor(value, (E,), f32), self._tensor(log_prob, (E,), f32)
        tv = dn = None
        if terminal_value is not None:
            if done is None:
                raise ValueError("terminal_value needs the step's dones")
            tv, dn = self._tensor(terminal_value, (E,), f32), self._tensor(done, (E,), u8)
        self.add_dev(self.pos, obs.data_ptr(), action.data_ptr(), reward.data_ptr(),
                     _capi.ACT_F64 if reward.dtype == torch.float64 else _capi.ACT_F32, episode_start.data_ptr(), value.data_ptr(),
                     log_prob.data_ptr(), None if tv is None else tv.data_ptr(), None if dn is None else dn.data_ptr())
        self.pos += 1
        self.full = self.pos == self.n_steps

    def compute_returns_and_advantage(self, last_values, dones):
        """SB3's GAE over the stored rows: last_values f32 [E] (or [E, 1]), dones u8 / bool [E] of the step after the last row."""
        import torch

        self.use_torch_stream()
        lv = self._tensor(last_values, (self.num_envs,), (torch.float32,))
        dn = self._tensor(dones, (self.num_envs,), (torch.uint8,))
        self.finish_dev(lv.data_ptr(), dn.data_ptr())

    def gather(self, indices, out: RolloutBatch | None = None) -> RolloutBatch:
        """The rows flat indices (int32 [B] on the device, i = env * n_steps + t) name, gathered by one launch."""
        import torch

        self.use_torch_stream()
        B = int(indices.numel())
        idx = self._tensor(indices, (B,), (torch.int32,))
        if out is None:
            dev = idx.device
            out = RolloutBatch(torch.empty((B, self.obs_dim), device=dev), torch.empty((B, self.act_dim), device=dev),
                               *(torch.empty(B, device=dev) for _ in range(4)))
        shapes = ((B, self.obs_dim), (B, self.act_dim), (B,), (B,), (B,), (B,))
        ptrs = [None if o is None else self._tensor(o, s, (torch.float32,)).data_ptr() for o, s in zip(out, shapes)]
        self.gather_dev(idx.data_ptr(), B, *ptrs)
        return out

    def get(self, batch_size: int | None = None, generator=None):
        """SB3's get: minibatches of `batch_size` rows (None: the whole buffer at once) over a fresh random permutation drawn by
        torch on the device (`generator`: a torch.Generator of that device, or None for the global one)."""
        import torch

        if not self.full:
            raise FleetHipError(_capi.ERR_STATE, "get() needs a full rollout buffer")
        n = self.n_steps * self.num_envs
        perm = torch.randperm(n, device=torch.device("cuda", self.device), dtype=torch.int32, generator=generator)
        batch_size = n if batch_size is None else int(batch_size)
        for start in range(0, n, batch_size):
            yield self.gather(perm[start:start + batch_size])
