"""`DeviceReplayBuffer`: stable-baselines3 2.3.2 `ReplayBuffer` in device memory.

The storage an off-policy algorithm (TD3, DDPG, SAC) fills and samples, on the GPU (fleetrl_amd/csrc/fleet_replay.hip,
include/fleet_hip.h `fleet_replay_*`): `add` stores one transition per env in one launch, `sample` draws a minibatch's indices on
the device (counter-based Philox: the same seed and call sequence give the same minibatches) and gathers it in the same launch.
Semantics are SB3's (optimize_memory_usage=False): a ring of `max(buffer_size // num_envs, 1)` rows, the observations and rewards
stored RAW (`FleetVecNormalize.original_torch()`) and normalised when they are sampled, with the normaliser's statistics of that
moment; `next_observations` holds the terminal observation for envs that finished; `dones` come back as `done * (1 - timeout)`.
Nothing crosses to the host.  The networks, the optimisers and the algorithm itself are the caller's (examples/td3_device_loop.py).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from . import _capi
from ._handle import _DeviceHandle

__all__ = ["DeviceReplayBuffer", "ReplayBatch"]

# SB3's ReplayBufferSamples
ReplayBatch = namedtuple("ReplayBatch", ["observations", "actions", "next_observations", "dones", "rewards"])


def _norm_handle(env):
    """The fleet_norm handle of a FleetVecNormalize / DeviceNormalizer, or None."""
    if env is None:
        return None
    norm = getattr(env, "norm", env)  # FleetVecNormalize carries a DeviceNormalizer
    h = getattr(norm, "h", None)
    if h is None or not hasattr(norm, "settings"):
        raise TypeError(f"env must be a FleetVecNormalize, a DeviceNormalizer or None, got {type(env).__name__}")
    return h


class DeviceReplayBuffer(_DeviceHandle):
    """One `fleet_replay_*` handle.  The `*_dev` methods take raw device addresses; every other method takes torch tensors on
    the buffer's device and launches on torch's current stream."""
    _prefix = "replay"

    def __init__(self, buffer_size: int, num_envs: int, obs_dim: int, act_dim: int, seed: int = 0, device: int = 0):
        self.buffer_size, self.num_envs, self.obs_dim, self.act_dim = int(buffer_size), int(num_envs), int(obs_dim), int(act_dim)
        self.seed = int(seed) & (2 ** 64 - 1)
        for name in ("buffer_size", "num_envs", "obs_dim", "act_dim"):
            if not -2 ** 31 <= getattr(self, name) < 2 ** 31:
                raise ValueError(f"{name} must fit a 32-bit integer, got {getattr(self, name)}")
        p = _capi.FleetReplayParams(C.sizeof(_capi.FleetReplayParams), self.num_envs, self.buffer_size, self.obs_dim, self.act_dim, 0,
                                    self.seed)
        self._open(device, p)
        self.rows = max(self.buffer_size // self.num_envs, 1)

    # ---- bookkeeping (the host's) -------------------------------------------------------------------------------------------
    def _size(self):
        pos, full, rows, calls = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        self._check(self.lib.fleet_replay_size(self.h, C.byref(pos), C.byref(full), C.byref(rows), C.byref(calls)))
        return pos.value, bool(full.value), rows.value, calls.value

    pos = property(lambda self: self._size()[0], doc="the ring row the next add writes")
    full = property(lambda self: self._size()[1], doc="whether the ring has wrapped")
    calls = property(lambda self: self._size()[3], doc="minibatches drawn so far (the index draw's call counter)")

    def size(self) -> int:
        """SB3's size(): rows that hold transitions."""
        pos, full, rows, _ = self._size()
        return rows if full else pos

    def set_position(self, pos: int, full: bool, calls: int = 0):
        """Resume: the write position, the wrap flag and the call counter of the index draw (an earlier counter replays its
        minibatches)."""
        self._check(self.lib.fleet_replay_set_position(self.h, int(pos), int(bool(full)), int(calls)))

    # ---- device pointers ------------------------------------------------------------------------------------------------
    def arrays_dev(self) -> dict:
        """name -> base address of the six arrays."""
        a = _capi.FleetReplayArrays()
        self._check(self.lib.fleet_replay_arrays(self.h, C.byref(a)))
        return {n: getattr(a, n) for n in _capi.REPLAY_ARRAY_NAMES}

    def add_dev(self, obs_ptr: int, next_obs_ptr: int, action_ptr: int, reward_ptr: int, reward_dtype: int, done_ptr: int,
                terminal_ptr: int | None = None, timeout_ptr: int | None = None):
        self._check(self.lib.fleet_replay_add_dev(self.h, obs_ptr, next_obs_ptr, action_ptr, reward_ptr, int(reward_dtype), done_ptr,
                                                  terminal_ptr, timeout_ptr))

    def gather_dev(self, rows_ptr: int, envs_ptr: int, batch: int, norm=None, obs_ptr=None, actions_ptr=None, next_obs_ptr=None,
                   dones_ptr=None, rewards_ptr=None):
        """`norm`: a FleetVecNormalize, a DeviceNormalizer or None."""
        self._check(self.lib.fleet_replay_gather_dev(self.h, rows_ptr, envs_ptr, int(batch), _norm_handle(norm), obs_ptr, actions_ptr,
                                                     next_obs_ptr, dones_ptr, rewards_ptr))

    def sample_dev(self, batch: int, norm=None, obs_ptr=None, actions_ptr=None, next_obs_ptr=None, dones_ptr=None, rewards_ptr=None,
                   rows_ptr=None, envs_ptr=None):
        self._check(self.lib.fleet_replay_sample_dev(self.h, int(batch), _norm_handle(norm), obs_ptr, actions_ptr, next_obs_ptr,
                                                     dones_ptr, rewards_ptr, rows_ptr, envs_ptr))

    def check_errors(self):
        """Waits for the buffer's stream; raises FleetHipError (ERR_STATE) once if a gather met an index out of range."""
        self._check(self.lib.fleet_replay_check_errors(self.h))

    # ---- the arrays as torch tensors (zero-copy views of the buffer's memory) -------------------------------------------------
    def _views(self) -> dict:
        if self._tensors is None:
            R, E, D, A = self.rows, self.num_envs, self.obs_dim, self.act_dim
            shapes = {"observations": (R, E, D), "next_observations": (R, E, D), "actions": (R, E, A)}
            self._tensors = self._make_views({n: (shapes.get(n, (R, E)), "|u1" if n in ("dones", "timeouts") else "<f4")
                                              for n in _capi.REPLAY_ARRAY_NAMES})
        return self._tensors

    observations = property(lambda self: self._views()["observations"], doc="f32 [rows, num_envs, obs_dim], raw")
    next_observations = property(lambda self: self._views()["next_observations"], doc="f32 [rows, num_envs, obs_dim], raw")
    actions = property(lambda self: self._views()["actions"], doc="f32 [rows, num_envs, act_dim]")
    rewards = property(lambda self: self._views()["rewards"], doc="f32 [rows, num_envs], raw")
    dones = property(lambda self: self._views()["dones"], doc="u8 [rows, num_envs]")
    timeouts = property(lambda self: self._views()["timeouts"], doc="u8 [rows, num_envs]")

    # ---- SB3's surface ----------------------------------------------------------------------------------------------------
    def add(self, obs, next_obs, action, reward, done, terminal=None, timeout=None):
        """SB3's add: ring row `pos` <- one transition per env.  obs / next_obs f32 [E, D] RAW (not normalised), action f32 [E, A],
        reward f64 or f32 [E] raw (rounded once to float32), done u8 / bool [E].  terminal f32 [E, D]: the raw terminal observations;
        the rows of done envs replace next_obs (`infos[i]["terminal_observation"]` in SB3's `_store_transition`), the others are
        not read.  timeout u8 [E]: `infos[i]["TimeLimit.truncated"]` (the reference's env reports its time limit as terminated,
        so None -- zeros -- is its behaviour)."""
        import torch

        self.use_torch_stream()
        E, D, A = self.num_envs, self.obs_dim, self.act_dim
        f32, u8 = (torch.float32,), (torch.uint8,)
        obs, next_obs, action = self._tensor(obs, (E, D), f32), self._tensor(next_obs, (E, D), f32), self._tensor(action, (E, A), f32)
        reward = self._tensor(reward, (E,), (torch.float64, torch.float32))
        done = self._tensor(done, (E,), u8)
        terminal = None if terminal is None else self._tensor(terminal, (E, D), f32)
        timeout = None if timeout is None else self._tensor(timeout, (E,), u8)
        self.add_dev(obs.data_ptr(), next_obs.data_ptr(), action.data_ptr(), reward.data_ptr(),
                     _capi.ACT_F64 if reward.dtype == torch.float64 else _capi.ACT_F32, done.data_ptr(),
                     None if terminal is None else terminal.data_ptr(), None if timeout is None else timeout.data_ptr())

    def _outputs(self, B, out, dev):
        import torch

        if out is None:
            out = ReplayBatch(torch.empty((B, self.obs_dim), device=dev), torch.empty((B, self.act_dim), device=dev),
                              torch.empty((B, self.obs_dim), device=dev), torch.empty((B, 1), device=dev),
                              torch.empty((B, 1), device=dev))
        shapes = ((B, self.obs_dim), (B, self.act_dim), (B, self.obs_dim), (B, 1), (B, 1))
        ptrs = [None if o is None else self._tensor(o, s, (torch.float32,)).data_ptr() for o, s in zip(out, shapes)]
        return out, ptrs

    def gather(self, rows, envs, env=None, out: ReplayBatch | None = None) -> ReplayBatch:
        """SB3's `_get_samples(batch_inds, env)` with given env indices: the transitions (rows[b], envs[b]) (int32 [B] on the
        device), normalised with `env`'s current statistics (a FleetVecNormalize, a DeviceNormalizer, or None: raw)."""
        import torch

        self.use_torch_stream()
        B = int(rows.numel())
        rows, envs = self._tensor(rows, (B,), (torch.int32,)), self._tensor(envs, (B,), (torch.int32,))
        out, ptrs = self._outputs(B, out, rows.device)
        self.gather_dev(rows.data_ptr(), envs.data_ptr(), B, env, *ptrs)
        return out

    def sample(self, batch_size: int, env=None, out: ReplayBatch | None = None, indices_out=None) -> ReplayBatch:
        """SB3's `sample(batch_size, env)`: indices drawn on the device (rows uniform over the filled part, envs uniform), gathered
        and normalised by the same launch.  indices_out: (rows, envs) int32 [B] tensors that receive the draw."""
        import torch

        self.use_torch_stream()
        B = int(batch_size)
        out, ptrs = self._outputs(B, out, torch.device("cuda", self.device))
        ri = ei = None
        if indices_out is not None:
            ri = self._tensor(indices_out[0], (B,), (torch.int32,)).data_ptr()
            ei = self._tensor(indices_out[1], (B,), (torch.int32,)).data_ptr()
        self.sample_dev(B, env, *ptrs, ri, ei)
        return out
