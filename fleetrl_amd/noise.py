"""Temporally correlated action noise on the device (include/fleet_hip.h "correlated action noise on the device", fleet_noise.hip):
the processes whose rows `DevicePolicy.explore(..., action_noise=proc)` adds to the actor's output.

    DevicePinkNoise   pink.PinkActionNoise / ColoredNoiseProcess per env: power-law noise of exponent beta over sequences of seq_len
                      samples (the episode's steps), unit scale -- `explore`'s sigma scales it
    DeviceOUNoise     SB3's OrnsteinUhlenbeckActionNoise per env; its rows carry mu and sigma: pass sigma = 1.0 to `explore`

`next(done)` gives one f32 [E, A] row block per call, on torch's current stream, and starts the envs with done != 0 afresh first,
as SB3's VectorizedActionNoise.reset(indices) does after the step that ended their episodes.  A row depends on (seed, global env id,
column, the env's own history of calls and resets) and on nothing else."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._handle import _DeviceHandle


class _DeviceNoise(_DeviceHandle):
    _prefix = "noise"
    kind = ""

    def _finish_open(self, device, params):
        self._open(device, params)
        self.num_envs, self.act_dim = int(params.num_envs), int(params.act_dim)

    def next_dev(self, done_ptr: int | None, eps_out_ptr: int):
        """Raw device addresses, on the handle's stream."""
        self._check(self.lib.fleet_noise_next_dev(self.h, done_ptr, eps_out_ptr))

    def next(self, done=None, out=None):
        """The next row of every env, f32 [E, A]; done (u8 / bool [E] or None): those envs start afresh first."""
        import torch

        self.use_torch_stream()
        E, A = self.num_envs, self.act_dim
        if out is None:
            out = torch.empty((E, A), device=torch.device("cuda", self.device), dtype=torch.float32)
        d = None if done is None else self._tensor(done, (E,), (torch.uint8, torch.bool))
        self.next_dev(None if d is None else d.data_ptr(), self._tensor(out, (E, A), (torch.float32,)).data_ptr())
        return out

    def reset(self, mask=None):
        """What `next` does to done envs, for the envs of `mask` (None: all), without emitting a row."""
        import torch

        self.use_torch_stream()
        m = None if mask is None else self._tensor(mask, (self.num_envs,), (torch.uint8, torch.bool))
        self._check(self.lib.fleet_noise_reset_dev(self.h, None if m is None else m.data_ptr()))

    def state_dict(self) -> dict:
        """Device tensors (copies, on torch's current stream) and the call count: what `load_state_dict` of a process created with
        the same parameters needs to continue the stream of rows."""
        import torch

        self.use_torch_stream()
        dev, E, A = torch.device("cuda", self.device), self.num_envs, self.act_dim
        calls = C.c_uint64()
        if self.kind == "pink":
            t, q = torch.empty(E, device=dev, dtype=torch.int32), torch.empty(E, device=dev, dtype=torch.int32)
            self._check(self.lib.fleet_noise_get_state_dev(self.h, t.data_ptr(), q.data_ptr(), None, C.byref(calls)))
            return {"kind": "pink", "t": t, "q": q, "calls": int(calls.value)}  # (q: the uint32's bits in an int32 tensor)
        x = torch.empty((E, A), device=dev, dtype=torch.float32)
        self._check(self.lib.fleet_noise_get_state_dev(self.h, None, None, x.data_ptr(), C.byref(calls)))
        return {"kind": "ou", "x": x, "calls": int(calls.value)}

    def load_state_dict(self, state: dict):
        import torch

        if state.get("kind") != self.kind:
            raise ValueError(f"the state belongs to a {state.get('kind')!r} process, this is a {self.kind!r} one")
        self.use_torch_stream()
        E, A = self.num_envs, self.act_dim
        if self.kind == "pink":
            t, q = self._tensor(state["t"], (E,), (torch.int32,)), self._tensor(state["q"], (E,), (torch.int32,))
            self._check(self.lib.fleet_noise_set_state_dev(self.h, t.data_ptr(), q.data_ptr(), None, int(state["calls"])))
        else:
            x = self._tensor(state["x"], (E, A), (torch.float32,))
            self._check(self.lib.fleet_noise_set_state_dev(self.h, None, None, x.data_ptr(), int(state["calls"])))

    def describe(self) -> dict:
        """What fleet_noise_describe reports."""
        p = _capi.FleetNoiseParams()
        self._check(self.lib.fleet_noise_describe(self.h, C.byref(p)))
        out = {"kind": self.kind, "num_envs": p.num_envs, "act_dim": p.act_dim, "env_id_offset": p.env_id_offset, "seed": p.seed}
        if self.kind == "pink":
            out.update(seq_len=p.seq_len, beta=p.beta, cache_bytes=p.cache_bytes)
        else:
            out.update(theta=p.theta, dt=p.dt)
        return out


class DevicePinkNoise(_DeviceNoise):
    """Pink (power-law) action noise per env: sequences of `seq_len` samples (2..4096; the episode's steps: a done env and an env
    whose sequence is used up take a new one), exponent `beta` (1: pink, 0: white, 2: red).  The handle keeps num_envs x seq_len x
    act_dim float32 on the device (157 MB at 4096 x 192 x 50).  A call in which envs take new sequences computes seq_len^2 terms per
    column of each: with episodes of equal length that started together, one slow call per episode."""
    kind = "pink"

    def __init__(self, num_envs: int, act_dim: int, seq_len: int, *, beta: float = 1.0, seed: int, env_id_offset: int = 0, device: int = 0):
        p = _capi.FleetNoiseParams()
        p.struct_bytes, p.kind = C.sizeof(_capi.FleetNoiseParams), _capi.NOISE_PINK
        p.num_envs, p.act_dim, p.seq_len, p.env_id_offset = int(num_envs), int(act_dim), int(seq_len), int(env_id_offset)
        p.beta, p.seed = float(beta), int(seed) & (2 ** 64 - 1)
        self.seq_len = int(seq_len)
        self._finish_open(device, p)


class DeviceOUNoise(_DeviceNoise):
    """Ornstein-Uhlenbeck action noise per env, x <- x + theta (mu - x) dt + sigma sqrt(dt) eps; mu, sigma: floats or arrays [act_dim]."""
    kind = "ou"

    def __init__(self, num_envs: int, act_dim: int, *, mu=0.0, sigma, theta: float = 0.15, dt: float = 1e-2, seed: int,
                 env_id_offset: int = 0, device: int = 0):
        p = _capi.FleetNoiseParams()
        p.struct_bytes, p.kind = C.sizeof(_capi.FleetNoiseParams), _capi.NOISE_OU
        p.num_envs, p.act_dim, p.env_id_offset = int(num_envs), int(act_dim), int(env_id_offset)
        p.theta, p.dt, p.seed = float(theta), float(dt), int(seed) & (2 ** 64 - 1)
        n = max(int(act_dim), 1)
        mu_a = np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), (n,)))
        sigma_a = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,)))
        p.mu, p.sigma = mu_a.ctypes.data, sigma_a.ctypes.data
        self._finish_open(device, p)
