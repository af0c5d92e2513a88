"""`FleetVecNormalize`: stable-baselines3 2.3.2 `VecNormalize` with its running statistics on the GPU.

The reference wraps every env in `VecNormalize(vec, norm_obs=True, norm_reward=True, clip_reward=10.0)`.  Here the statistics,
the normalise-and-clip pass and the discounted returns live on the device (fleetrl_amd/csrc/fleet_norm.hip, include/fleet_hip.h
`fleet_norm_*`): the host path inserts three launches between the step kernel and the transfers, and `step_torch` keeps
everything in HBM.  Semantics are SB3's, with two deliberate deviations:
  (a) the observations' batch moments are accumulated in float64 (SB3's np.mean / np.var accumulate the float32 array in
      float32);
  (b) the reward enters as the env's float64 reward rounded to float32 -- exactly what VecNormalize(FleetVecEnv) sees, since
      FleetVecEnv returns float32 rewards.

  DeviceNormalizer   thin handle over fleet_norm_* for device pointers / torch tensors (any producer of [E, D] observations)
  FleetVecNormalize  the VecNormalize surface over a FleetVecEnv
  sync_normalization SB3's sync_envs_normalization for these classes (eval envs)
"""
from __future__ import annotations

import ctypes as C
import io
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

from . import _capi
from ._capi import FleetHipError
from ._handle import _DeviceHandle

__all__ = ["DeviceNormalizer", "FleetVecNormalize", "RunningStats", "sync_normalization", "NormSettings", "NormState",
           "save_state", "load_state", "state_from_sb3"]

try:
    from stable_baselines3.common.vec_env import VecEnvWrapper as _SB3VecEnvWrapper
except ImportError:  # pragma: no cover - depends on the installation
    _SB3VecEnvWrapper = object


# FleetVecNormalize.original_torch()
OriginalTensors = namedtuple("OriginalTensors", ["obs", "reward", "terminal"])


@dataclass
class NormSettings:
    """VecNormalize's constructor arguments (SB3 2.3.2 defaults)."""
    training: bool = True
    norm_obs: bool = True
    norm_reward: bool = True
    clip_obs: float = 10.0
    clip_reward: float = 10.0
    gamma: float = 0.99
    epsilon: float = 1e-8

    def validate(self) -> "NormSettings":
        """Raises ValueError on what fleet_norm_create would refuse."""
        for name in ("clip_obs", "clip_reward", "gamma", "epsilon"):
            v = getattr(self, name)
            if not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
        if not self.clip_obs > 0 or not self.clip_reward > 0:
            raise ValueError(f"clip_obs and clip_reward must be > 0, got {self.clip_obs}, {self.clip_reward}")
        if not 0 <= self.gamma <= 1:
            raise ValueError(f"gamma must be in [0, 1], got {self.gamma}")
        if not self.epsilon > 0:
            raise ValueError(f"epsilon must be > 0, got {self.epsilon}")
        return self


@dataclass
class RunningStats:
    """SB3 RunningMeanStd's attributes (a snapshot: assign it back to `obs_rms` / `ret_rms` to change the device's)."""
    mean: np.ndarray
    var: np.ndarray
    count: float


@dataclass
class NormState:
    """Everything a normaliser carries from step to step (float64)."""
    obs_rms: RunningStats
    ret_rms: RunningStats
    returns: np.ndarray | None = None  # None: zero (SB3 does not save it)


def _stats(mean, var, count, shape) -> RunningStats:
    mean = np.array(mean, dtype=np.float64).reshape(shape)
    var = np.array(var, dtype=np.float64).reshape(shape)
    count = float(count)
    if not np.all(np.isfinite(mean)) or not np.all(np.isfinite(var)) or np.any(var < 0):
        raise ValueError("running statistics must be finite with var >= 0")
    if not (np.isfinite(count) and count > 0):
        raise ValueError(f"running count must be > 0, got {count}")
    return RunningStats(mean, var, count)


def save_state(path, settings: NormSettings, state: NormState) -> None:
    """`.npz` with the statistics and the settings (not `returns`: as in SB3 they start at zero after a load).  `path` is
    written as given (no `.npz` appended)."""
    buf = io.BytesIO()
    np.savez(buf, obs_mean=state.obs_rms.mean, obs_var=state.obs_rms.var, obs_count=np.float64(state.obs_rms.count),
             ret_mean=np.float64(state.ret_rms.mean), ret_var=np.float64(state.ret_rms.var), ret_count=np.float64(state.ret_rms.count),
             training=settings.training, norm_obs=settings.norm_obs, norm_reward=settings.norm_reward, clip_obs=settings.clip_obs,
             clip_reward=settings.clip_reward, gamma=settings.gamma, epsilon=settings.epsilon)
    with open(path, "wb") as fh:
        fh.write(buf.getvalue())


def load_state(path) -> tuple[NormSettings, NormState]:
    with np.load(path, allow_pickle=False) as z:
        s = NormSettings(training=bool(z["training"]), norm_obs=bool(z["norm_obs"]), norm_reward=bool(z["norm_reward"]),
                         clip_obs=float(z["clip_obs"]), clip_reward=float(z["clip_reward"]), gamma=float(z["gamma"]),
                         epsilon=float(z["epsilon"])).validate()
        D = int(np.asarray(z["obs_mean"]).size)
        st = NormState(_stats(z["obs_mean"], z["obs_var"], z["obs_count"], (D,)), _stats(z["ret_mean"], z["ret_var"], z["ret_count"], ()))
    return s, st


def state_from_sb3(vec_normalize) -> tuple[NormSettings, NormState]:
    """Settings and statistics of any object with SB3 VecNormalize's attributes (obs_rms / ret_rms with mean, var, count;
    clip_obs, clip_reward, gamma, epsilon, training, norm_obs, norm_reward) -- e.g. a `vec_normalize-*.pkl` the reference's
    pipeline saved.  Raises ValueError on parameters the device normaliser does not take (dict observations included)."""
    vn = vec_normalize
    g = lambda name, default: getattr(vn, name, default)  # noqa: E731
    s = NormSettings(training=bool(g("training", True)), norm_obs=bool(g("norm_obs", True)), norm_reward=bool(g("norm_reward", True)),
                     clip_obs=g("clip_obs", 10.0), clip_reward=g("clip_reward", 10.0), gamma=g("gamma", 0.99),
                     epsilon=g("epsilon", 1e-8)).validate()
    o, r = vn.obs_rms, vn.ret_rms
    if isinstance(o, dict):
        raise ValueError("dict observation spaces are not supported: FleetEnv's observations are one Box")
    mean = np.asarray(o.mean, dtype=np.float64)
    if mean.ndim != 1:
        raise ValueError(f"obs_rms.mean must have shape (obs_dim,), got {mean.shape}")
    if np.asarray(r.mean).size != 1:
        raise ValueError("ret_rms must be scalar")
    return s, NormState(_stats(o.mean, o.var, o.count, mean.shape), _stats(r.mean, r.var, r.count, ()))


def normalize_obs_np(obs, rms: RunningStats, clip_obs: float, epsilon: float) -> np.ndarray:
    """SB3 `_normalize_obs` in float64, rounded once to float32 (what the device computes)."""
    x = np.asarray(obs, dtype=np.float32).astype(np.float64)
    return np.clip((x - rms.mean) / np.sqrt(rms.var + epsilon), -clip_obs, clip_obs).astype(np.float32)


class DeviceNormalizer(_DeviceHandle):
    """One `fleet_norm_*` handle: SB3 VecNormalize's state and arithmetic for a batch of `num_envs` observations of `obs_dim`
    floats on `device`.  The `*_dev` calls take raw device addresses and are asynchronous on the normaliser's stream (its own
    unless `set_stream` / `use_torch_stream` adopted another)."""
    _prefix = "norm"

    def __init__(self, num_envs: int, obs_dim: int, device: int = 0, **settings):
        self.settings = NormSettings(**settings).validate()
        self.E, self.D = int(num_envs), int(obs_dim)
        self._open(device, self._params())

    def _params(self) -> _capi.FleetNormParams:
        s = self.settings
        return _capi.FleetNormParams(C.sizeof(_capi.FleetNormParams), self.E, self.D, int(bool(s.training)), int(bool(s.norm_obs)),
                                     int(bool(s.norm_reward)), float(s.clip_obs), float(s.clip_reward), float(s.gamma),
                                     float(s.epsilon))

    def configure(self, **changes):
        """Change flags / constants (training, norm_obs, norm_reward, clip_obs, clip_reward, gamma, epsilon)."""
        new = NormSettings(**{**self.settings.__dict__, **changes}).validate()
        old, self.settings = self.settings, new
        rc = self.lib.fleet_norm_configure(self.h, C.byref(self._params()))
        if rc != _capi.OK:
            self.settings = old
            self._check(rc)

    # ---- device pointers --------------------------------------------------------------------------------------------
    def reset_dev(self, raw_obs_ptr: int, obs_ptr: int):
        self._check(self.lib.fleet_norm_reset_dev(self.h, raw_obs_ptr, obs_ptr))

    def step_dev(self, raw_obs_ptr: int, raw_reward_ptr: int, done_ptr: int, raw_terminal_ptr: int | None, obs_ptr: int,
                 reward_ptr: int, terminal_ptr: int | None):
        self._check(self.lib.fleet_norm_step_dev(self.h, raw_obs_ptr, raw_reward_ptr, done_ptr, raw_terminal_ptr, obs_ptr,
                                                 reward_ptr, terminal_ptr))

    # ---- torch tensors (on torch's current stream) ----------------------------------------------------------------
    def _tensor(self, t, shape, dtype):  # stricter than the buffers': nothing is converted, and the address comes back
        import torch

        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or \
                t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError(f"expected a contiguous {dtype} tensor of shape {shape} on cuda:{self.device}")
        return t.data_ptr()

    def reset_torch(self, raw_obs, out=None):
        import torch

        self.use_torch_stream()
        out = out if out is not None else torch.empty_like(raw_obs)
        self.reset_dev(self._tensor(raw_obs, (self.E, self.D), torch.float32), self._tensor(out, (self.E, self.D), torch.float32))
        return out

    def step_torch(self, raw_obs, raw_reward, done, raw_terminal=None, obs_out=None, reward_out=None, terminal_out=None):
        """-> (obs f32 [E,D], reward f64 [E], terminal f32 [E,D] or None); outputs may alias their raw inputs (in place)."""
        import torch

        self.use_torch_stream()
        obs = obs_out if obs_out is not None else torch.empty_like(raw_obs)
        rew = reward_out if reward_out is not None else torch.empty_like(raw_reward)
        term = None
        if raw_terminal is not None:
            term = terminal_out if terminal_out is not None else torch.empty_like(raw_terminal)
        OD = (self.E, self.D)
        self.step_dev(self._tensor(raw_obs, OD, torch.float32), self._tensor(raw_reward, (self.E,), torch.float64),
                      self._tensor(done, (self.E,), torch.uint8),
                      None if raw_terminal is None else self._tensor(raw_terminal, OD, torch.float32),
                      self._tensor(obs, OD, torch.float32), self._tensor(rew, (self.E,), torch.float64),
                      None if term is None else self._tensor(term, OD, torch.float32))
        return obs, rew, term

    # ---- state (host, synchronous) --------------------------------------------------------------------------------
    def get_state(self) -> NormState:
        om, ov, rt = np.zeros(self.D), np.zeros(self.D), np.zeros(self.E)
        oc, rm, rv, rc_ = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.fleet_norm_get_state(self.h, om.ctypes.data, ov.ctypes.data, C.byref(oc), C.byref(rm), C.byref(rv),
                                                  C.byref(rc_), rt.ctypes.data))
        return NormState(RunningStats(om, ov, oc.value), RunningStats(np.float64(rm.value), np.float64(rv.value), rc_.value), rt)

    def set_state(self, obs_rms: RunningStats | None = None, ret_rms: RunningStats | None = None, returns=None):
        """Overwrite what is given (None: keep)."""
        args = [None] * 7
        keep = []
        if obs_rms is not None:
            o = _stats(obs_rms.mean, obs_rms.var, obs_rms.count, (self.D,))
            keep += [o.mean, o.var]
            args[0], args[1], args[2] = o.mean.ctypes.data, o.var.ctypes.data, C.byref(C.c_double(o.count))
        if ret_rms is not None:
            r = _stats(ret_rms.mean, ret_rms.var, ret_rms.count, ())
            args[3], args[4], args[5] = (C.byref(C.c_double(float(r.mean))), C.byref(C.c_double(float(r.var))),
                                         C.byref(C.c_double(r.count)))
        if returns is not None:
            rt = np.ascontiguousarray(returns, dtype=np.float64).reshape(self.E)
            keep.append(rt)
            args[6] = rt.ctypes.data
        self._check(self.lib.fleet_norm_set_state(self.h, *args))

    def original(self, obs: bool = True, reward: bool = True):
        """(raw obs [E,D] f32 or None, raw reward [E] f64 or None) of the last reset / step."""
        o = np.empty((self.E, self.D), np.float32) if obs else None
        r = np.empty(self.E) if reward else None
        self._check(self.lib.fleet_norm_original_host(self.h, None if o is None else o.ctypes.data, None if r is None else r.ctypes.data))
        return o, r


class FleetVecNormalize(_SB3VecEnvWrapper):
    """SB3 `VecNormalize` over a `FleetVecEnv`, with the statistics on the GPU (a subclass of SB3's `VecEnvWrapper` when SB3 is
    installed).  Rewards come back as float64 (the device's normalised values); `infos[i]["terminal_observation"]` is
    normalised, `infos[i]["episode"]` is the raw return (SB3's Monitor sits below VecNormalize)."""

    def __init__(self, venv, training: bool = True, norm_obs: bool = True, norm_reward: bool = True, clip_obs: float = 10.0,
                 clip_reward: float = 10.0, gamma: float = 0.99, epsilon: float = 1e-8):
        core = venv.core
        self.venv = venv
        self.norm = DeviceNormalizer(venv.num_envs, core.obs_dim, device=core.batch.device, training=training, norm_obs=norm_obs,
                                     norm_reward=norm_reward, clip_obs=clip_obs, clip_reward=clip_reward, gamma=gamma, epsilon=epsilon)
        if _SB3VecEnvWrapper is not object:
            _SB3VecEnvWrapper.__init__(self, venv)
        else:
            self.num_envs = venv.num_envs
            self.observation_space = venv.observation_space
            self.action_space = venv.action_space
            self.render_mode = None
        self._torch = None  # raw device buffers of step_torch

    # ---- settings (written through to the device) -------------------------------------------------------------------
    def _setting(name):  # noqa: N805 - property factory
        return property(lambda self: getattr(self.norm.settings, name), lambda self, v: self.norm.configure(**{name: v}))

    training = _setting("training")
    norm_obs = _setting("norm_obs")
    norm_reward = _setting("norm_reward")
    clip_obs = _setting("clip_obs")
    clip_reward = _setting("clip_reward")
    gamma = _setting("gamma")
    epsilon = _setting("epsilon")
    del _setting

    @property
    def obs_rms(self) -> RunningStats:
        return self.norm.get_state().obs_rms

    @obs_rms.setter
    def obs_rms(self, rms):
        self.norm.set_state(obs_rms=rms)

    @property
    def ret_rms(self) -> RunningStats:
        return self.norm.get_state().ret_rms

    @ret_rms.setter
    def ret_rms(self, rms):
        self.norm.set_state(ret_rms=rms)

    @property
    def returns(self) -> np.ndarray:
        return self.norm.get_state().returns

    # ---- the VecEnv protocol ----------------------------------------------------------------------------------------
    def reset(self):
        return self.venv._reset(norm=self.norm)

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        return self.venv._step_wait(norm=self.norm)

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def step_torch(self, actions, obs_out=None, reward_out=None, done_out=None, terminal_out=None):
        """The device path: FleetVecEnv.step_torch into raw buffers of this wrapper, then the normaliser, both on torch's current
        stream -> (obs f32 [E,D], reward f64 [E], done u8 [E]) normalised; `terminal_out` [E,D] gets the normalised terminal rows
        of the envs that finished."""
        import torch

        dev = actions.device
        E, D = self.num_envs, self.norm.D
        if self._torch is None or self._torch[0].device != dev:
            self._torch = (torch.empty((E, D), device=dev, dtype=torch.float32), torch.empty(E, device=dev, dtype=torch.float64),
                           torch.empty((E, D), device=dev, dtype=torch.float32))
        raw_obs, raw_rew, raw_term = self._torch
        done = done_out if done_out is not None else torch.empty(E, device=dev, dtype=torch.uint8)
        self.venv.step_torch(actions, obs_out=raw_obs, reward_out=raw_rew, done_out=done,
                             terminal_out=None if terminal_out is None else raw_term)
        obs, rew, _ = self.norm.step_torch(raw_obs, raw_rew, done, None if terminal_out is None else raw_term, obs_out=obs_out,
                                           reward_out=reward_out, terminal_out=terminal_out)
        return obs, rew, done

    def reset_torch(self, obs_out=None):
        """reset() on the device path: the env's reset into a raw buffer of this wrapper, then the normaliser's."""
        import torch

        dev = torch.device("cuda", self.norm.device)
        E, D = self.num_envs, self.norm.D
        if self._torch is None:
            self._torch = (torch.empty((E, D), device=dev, dtype=torch.float32), torch.empty(E, device=dev, dtype=torch.float64),
                           torch.empty((E, D), device=dev, dtype=torch.float32))
        batch = self.venv.core.batch
        batch.use_torch_stream(dev)
        self.venv._torch_stream = torch.cuda.current_stream(dev).cuda_stream
        self.venv.core.clear_start_overrides()
        batch.reset_dev(self._torch[0].data_ptr())
        return self.norm.reset_torch(self._torch[0], out=obs_out)

    def original_torch(self) -> OriginalTensors:
        """The device twin of get_original_obs / get_original_reward: the wrapper's own raw tensors of the last `step_torch` /
        `reset_torch` -- obs f32 [E,D], reward f64 [E], terminal f32 [E,D] -- as an off-policy buffer stores them
        (`DeviceReplayBuffer.add`).  They are views, overwritten by the next step: consume them (or copy them) before it.  After a
        reset only `obs` is meaningful.  `terminal` is valid only when the step was asked for the terminal rows (`terminal_out`
        given), and then only in the rows of envs that finished: the other rows are stale."""
        if self._torch is None:
            raise FleetHipError(_capi.ERR_STATE, "original_torch: no step_torch / reset_torch yet")
        return OriginalTensors(*self._torch)

    # ---- SB3 VecNormalize helpers (host NumPy, arbitrary arrays) -----------------------------------------------------
    def get_original_obs(self) -> np.ndarray:
        return self.norm.original(obs=True, reward=False)[0]

    def get_original_reward(self) -> np.ndarray:
        return self.norm.original(obs=False, reward=True)[1].astype(np.float32)

    def normalize_obs(self, obs) -> np.ndarray:
        if not self.norm_obs:
            return np.asarray(obs)
        return normalize_obs_np(obs, self.obs_rms, self.clip_obs, self.epsilon)

    def normalize_reward(self, reward) -> np.ndarray:
        if not self.norm_reward:
            return np.asarray(reward)
        r = np.asarray(reward, dtype=np.float64)
        return np.clip(r / np.sqrt(float(self.ret_rms.var) + self.epsilon), -self.clip_reward, self.clip_reward)

    def unnormalize_obs(self, obs) -> np.ndarray:
        if not self.norm_obs:
            return np.asarray(obs)
        rms = self.obs_rms
        return (np.asarray(obs, dtype=np.float64) * np.sqrt(rms.var + self.epsilon) + rms.mean).astype(np.float32)

    def unnormalize_reward(self, reward) -> np.ndarray:
        if not self.norm_reward:
            return np.asarray(reward)
        return np.asarray(reward, dtype=np.float64) * np.sqrt(float(self.ret_rms.var) + self.epsilon)

    # ---- persistence ---------------------------------------------------------------------------------------------
    def _state(self) -> NormState:
        return self.norm.get_state()

    def save(self, path) -> None:
        save_state(path, self.norm.settings, self._state())

    @classmethod
    def _with_state(cls, venv, settings: NormSettings, state: NormState) -> "FleetVecNormalize":
        D = venv.core.obs_dim
        if state.obs_rms.mean.shape != (D,):
            raise ValueError(f"the statistics are for obs_dim {state.obs_rms.mean.shape}, the env has {D}")
        self = cls(venv, **settings.__dict__)
        self.norm.set_state(obs_rms=state.obs_rms, ret_rms=state.ret_rms, returns=np.zeros(venv.num_envs))
        return self

    @classmethod
    def load(cls, path, venv) -> "FleetVecNormalize":
        """Settings and statistics from `save`; `returns` start at zero (as SB3's load)."""
        return cls._with_state(venv, *load_state(path))

    @classmethod
    def from_sb3(cls, vec_normalize, venv) -> "FleetVecNormalize":
        """From SB3's VecNormalize (or anything with its attributes, e.g. `VecNormalize.load(pkl, dummy)` of the reference's pipeline)."""
        return cls._with_state(venv, *state_from_sb3(vec_normalize))

    # ---- pass-through ------------------------------------------------------------------------------------------------
    def env_method(self, method_name: str, *method_args, indices=None, **method_kwargs):
        return self.venv.env_method(method_name, *method_args, indices=indices, **method_kwargs)

    def get_attr(self, attr_name: str, indices=None):
        return self.venv.get_attr(attr_name, indices)

    def set_attr(self, attr_name: str, value, indices=None):
        return self.venv.set_attr(attr_name, value, indices)

    def env_is_wrapped(self, wrapper_class, indices=None):
        return self.venv.env_is_wrapped(wrapper_class, indices)

    def seed(self, seed=None):
        return self.venv.seed(seed)

    def get_images(self):
        return self.venv.get_images()

    def render(self, mode=None):
        return None

    def close(self):
        self.norm.close()
        self.venv.close()


def sync_normalization(src, dst) -> None:
    """SB3's `sync_envs_normalization` for FleetVecNormalize (which it does not recognise): copy `src`'s obs_rms / ret_rms to
    `dst` (e.g. the training env's statistics to an eval env).  `src` may be any object with VecNormalize's attributes."""
    dst.obs_rms = src.obs_rms
    dst.ret_rms = src.ret_rms
