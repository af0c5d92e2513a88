"""`DevicePPOCollect` / `DeviceTD3Collect` / `DeviceSACCollect`: stable-baselines3's `collect_rollouts` as one enqueue-only call
(include/fleet_hip.h `fleet_collect_*`, include/fleet_hip_sac_loop.h `fleet_saccollect_*`, fleetrl_amd/csrc/fleet_collect.hip).

The other half of `learn()` beside `DevicePPOTrain.train` / `DeviceTD3Train.train`: per env step the exploration launch
(`DevicePolicy.sample` / `explore` / `sample_uniform`), the env's step, the normaliser's step and the buffer's `add`, each the launch
the pieces make on their own, in their order -- the buffers, the normaliser's statistics, the noise process and the env end up bit-equal
to the loops of examples/ppo_device_train.py and examples/td3_pink_noise.py -- and one launch per step that keeps SB3's
`ep_info_buffer` on the device: the last `stats_window` finished episodes in the order `Monitor` reports them.  One block of statistics
(`STATS`: what SB3 logs as `rollout/*`) is written at the end.  The observation a rollout ends on, its `episode_start` flags and the
raw observation an off-policy loop keeps are the handle's: the next call starts from them.  Deterministic from (the handles' state, seed,
first_step).  Out of scope: the time-limit bootstrap, gSDE, `train_freq` in episodes, callbacks.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import FleetHipError
from ._handle import _DeviceHandle

__all__ = ["DevicePPOCollect", "DeviceTD3Collect", "DeviceSACCollect", "STATS", "SB3_NAMES"]

# the statistics block f64[16]: the means over the ring (NaN while it is empty), the episodes that finished in the call, the episodes
# appended so far, the env steps taken after the call; then zeros
STATS = ("ep_rew_mean", "ep_len_mean", "episodes", "total_episodes", "num_steps")
# SB3's logger keys where it has one, in STATS' order (time/total_timesteps is num_steps * num_envs)
SB3_NAMES = ("rollout/ep_rew_mean", "rollout/ep_len_mean", None, None, None)


class _DeviceCollect(_DeviceHandle):
    """One `fleet_collect_*` handle on `env` (a `FleetVecEnv`, or a `FleetVecNormalize` over one) and `policy` (a `DevicePolicy`; for
    `DeviceSACCollect` a `DeviceSACNetworks`), which must outlive it.  `stats_window`: SB3's `stats_window_size`, the episodes
    `rollout/ep_*_mean` average over."""
    _prefix = "collect"
    _create_entry = "fleet_collect_create"  # the create call of the family's handle: what the actor's kind decides

    def __init__(self, env, policy, stats_window: int = 100):
        self.env, self.policy = env, policy
        self.venv = getattr(env, "venv", env)  # the FleetVecEnv under a FleetVecNormalize
        self.norm = getattr(env, "norm", None)
        self.batch = self.venv.core.batch
        self.lib = _capi.load_library()
        self.device = int(self.batch.device)
        self.num_envs, self.obs_dim, self.act_dim = int(self.venv.num_envs), int(policy.obs_dim), int(policy.act_dim)
        self.stats_window = int(stats_window)
        h = C.c_void_p()
        p = _capi.FleetCollectParams(C.sizeof(_capi.FleetCollectParams), self.stats_window)
        rc = getattr(self.lib, self._create_entry)(self.batch.h, None if self.norm is None else self.norm.h, policy.h, C.byref(p), C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self.lib.fleet_collect_last_error(None).decode())
        self.h = h
        self._constants = {}  # _per_action's device tensors of float arguments
        self._lent = ()       # the buffer and the noise process of the last call: use_torch_stream moves them too

    # ---- streams -----------------------------------------------------------------------------------------------------------------
    def set_stream(self, hip_stream):
        """The handle has no stream of its own: the env's, the normaliser's and the policy's are set."""
        self.batch.set_stream(hip_stream)
        self.venv._torch_stream = hip_stream
        for h in (self.norm, self.policy, *self._lent):
            if h is not None:
                h.set_stream(hip_stream)

    def use_torch_stream(self, device=None):
        """The env, the normaliser, the policy and what the last call was lent all launch on torch's current stream from now on."""
        import torch

        cur = torch.cuda.current_stream(self.device if device is None else device).cuda_stream
        if getattr(self.venv, "_torch_stream", None) != cur:
            self.batch.set_stream(cur)
            self.venv._torch_stream = cur
        for h in (self.norm, self.policy, *self._lent):
            if h is not None:
                h.use_torch_stream(device)

    # ---- the handle --------------------------------------------------------------------------------------------------------------
    def describe(self) -> dict:
        """What fleet_collect_describe reports (arrays of two as tuples)."""
        i = _capi.FleetCollectInfo()
        self._check(self.lib.fleet_collect_describe(self.h, C.byref(i)))
        out = {n: getattr(i, n) for n, _ in i._fields_ if n != "reserved"}
        return {n: (tuple(v) if isinstance(v, C.Array) else v) for n, v in out.items()}

    def _views(self) -> dict:
        if self._tensors is None:
            import torch

            from ._handle import _DeviceArray

            d, dev = self.describe(), torch.device("cuda", self.device)
            E, D = self.num_envs, self.obs_dim
            view = lambda ptr, shape, typestr: torch.as_tensor(_DeviceArray(ptr, shape, typestr, self), device=dev)  # noqa: E731
            self._tensors = {"obs": [view(p, (E, D), "<f4") for p in d["carry_obs"]], "raw": [view(p, (E, D), "<f4") for p in d["raw_obs"]],
                             "start": [view(p, (E,), "|u1") for p in d["carry_start"]], "last_values": view(d["last_values"], (E,), "<f4")}
        return self._tensors

    def _side(self) -> int:
        return int(self.describe()["cur"])

    carry_obs = property(lambda self: self._views()["obs"][self._side()], doc="f32 [E, D]: the observation the next call starts from")
    carry_start = property(lambda self: self._views()["start"][self._side()], doc="u8 [E]: its episode_start / done flags")
    raw_obs = property(lambda self: self._views()["raw"][self._side()], doc="f32 [E, D]: the raw observation behind carry_obs")
    last_values = property(lambda self: self._views()["last_values"], doc="f32 [E]: the bootstrap values of the last PPO call")

    def reset(self, clear_episodes: bool = False):
        """SB3's `_setup_learn`: the env's reset (and the normaliser's) into the carry, episode_start = 1; `clear_episodes` also
        empties the episode ring.  On torch's current stream, no host synchronisation."""
        self.use_torch_stream()
        self.venv.core.clear_start_overrides()
        self._check(self.lib.fleet_collect_reset_dev(self.h, int(bool(clear_episodes))))

    def _stats(self, stats_out):
        import torch

        if stats_out is None:
            stats_out = torch.empty(_capi.COLLECT_STATS, device=torch.device("cuda", self.device), dtype=torch.float64)
        return stats_out, self._tensor(stats_out, (_capi.COLLECT_STATS,), (torch.float64,)).data_ptr()

    def episodes(self):
        """SB3's `ep_info_buffer`: (returns f64 [n], lengths i32 [n]) of the last n <= stats_window finished episodes, oldest first,
        and the number appended so far.  Synchronous."""
        W = self.stats_window
        ret, length, count = np.zeros(W, np.float64), np.zeros(W, np.int32), C.c_uint64()
        self._check(self.lib.fleet_collect_episodes_read(self.h, ret.ctypes.data, length.ctypes.data, C.byref(count)))
        n = min(count.value, W)
        order = [(count.value - n + i) % W for i in range(n)]
        return ret[order], length[order], count.value

    def episodes_dev(self, done, ep_return, ep_len):
        """The episode launch on given device tensors u8 [E], f64 [E], i32 [E] (any E) instead of the env's records."""
        import torch

        self.use_torch_stream()
        E = int(done.numel())
        done = self._tensor(done, (E,), (torch.uint8,))
        ep_return, ep_len = self._tensor(ep_return, (E,), (torch.float64,)), self._tensor(ep_len, (E,), (torch.int32,))
        self._check(self.lib.fleet_collect_episodes_dev(self.h, done.data_ptr(), ep_return.data_ptr(), ep_len.data_ptr(), E))

    def finish(self, first_step: int = 0, steps: int = 0, stats_out=None):
        """The closing launch on its own -> the statistics f64 [16] on the device."""
        self.use_torch_stream()
        stats_out, ptr = self._stats(stats_out)
        self._check(self.lib.fleet_collect_finish_dev(self.h, int(first_step) & (2 ** 64 - 1), int(steps), ptr))
        return stats_out

    def check_errors(self):
        """Passes through to the env's and to the last call's buffer's: waits for the stream, raises FleetHipError (ERR_STATE) on a
        device error."""
        self.batch.check_errors()
        for h in self._lent:
            if hasattr(h, "check_errors"):
                h.check_errors()


class DevicePPOCollect(_DeviceCollect):
    """`OnPolicyAlgorithm.collect_rollouts` on the device: `collect` fills a `DeviceRolloutBuffer` and computes its returns and
    advantages; `DevicePPOTrain.train` takes the buffer from there.  The policy needs a critic head."""

    def collect_dev(self, args: "_capi.FleetCollectPpoArgs"):
        """Raw device addresses in a FleetCollectPpoArgs, on the stream the borrowed handles share."""
        args.struct_bytes = C.sizeof(_capi.FleetCollectPpoArgs)
        self._check(self.lib.fleet_collect_ppo_dev(self.h, C.byref(args)))

    def collect(self, buffer, log_std, *, seed: int, first_step: int, env_id_offset: int = 0, stats_out=None):
        """All `buffer.n_steps` rows on torch's current stream, no host synchronisation.  log_std: the torch parameter f32 [act_dim] (a
        float or an array also does, as for `DevicePolicy.sample`).  first_step: the env steps taken so far -- the noise's counter, which
        must never repeat over a run.  Returns the statistics f64 [16] on the device: `STATS`, then zeros.  The buffer is full
        afterwards."""
        self._lent = (buffer,)
        self.use_torch_stream()
        a = _capi.FleetCollectPpoArgs()
        a.n_steps, a.env_id_offset, a.buffer = int(buffer.n_steps), int(env_id_offset), buffer.h.value
        a.log_std = self._per_action("log_std", log_std).data_ptr()
        a.seed, a.first_step = int(seed) & (2 ** 64 - 1), int(first_step) & (2 ** 64 - 1)
        stats_out, a.stats = self._stats(stats_out)
        buffer.pos, buffer.full = 0, False
        self.collect_dev(a)
        buffer.pos, buffer.full = buffer.n_steps, True
        return stats_out


class DeviceTD3Collect(_DeviceCollect):
    """`OffPolicyAlgorithm.collect_rollouts` on the device for `train_freq = (n_steps, "step")`: `collect` adds `n_steps` raw transitions
    per env to a `DeviceReplayBuffer`."""

    def collect_dev(self, args: "_capi.FleetCollectOffpolicyArgs"):
        """Raw device addresses in a FleetCollectOffpolicyArgs, on the stream the borrowed handles share."""
        args.struct_bytes = C.sizeof(_capi.FleetCollectOffpolicyArgs)
        self._check(self.lib.fleet_collect_offpolicy_dev(self.h, C.byref(args)))

    def collect(self, replay, n_steps: int, *, learning_starts: int, sigma, noise=None, shift=None, low: float = -1.0, high: float = 1.0,
                seed: int, first_step: int, env_id_offset: int = 0, stats_out=None):
        """`n_steps` env steps on torch's current stream, no host synchronisation.  Global step s = first_step + t draws uniform actions
        while s < learning_starts and clip(actor(obs) + shift + sigma * eps, low, high) afterwards; eps is the next row of `noise` (a
        `DevicePinkNoise` or a `DeviceOUNoise`, restarted per env by the step's done flags) or, without one, white noise keyed by (seed,
        s).  sigma, shift: floats, arrays or device tensors f32 [act_dim].  Returns the statistics f64 [16] on the device."""
        self._lent = (replay,) if noise is None else (replay, noise)
        self.use_torch_stream()
        a = _capi.FleetCollectOffpolicyArgs()
        a.n_steps, a.env_id_offset, a.replay = int(n_steps), int(env_id_offset), replay.h.value
        a.learning_starts = max(int(learning_starts), 0)
        a.sigma = self._per_action("sigma", sigma).data_ptr()
        a.shift = None if shift is None else self._per_action("shift", shift).data_ptr()
        a.noise_lo, a.noise_hi = float(low), float(high)
        a.noise = None if noise is None else noise.h.value
        a.seed, a.first_step = int(seed) & (2 ** 64 - 1), int(first_step) & (2 ** 64 - 1)
        stats_out, a.stats = self._stats(stats_out)
        self.collect_dev(a)
        return stats_out


class DeviceSACCollect(_DeviceCollect):
    """`OffPolicyAlgorithm.collect_rollouts` on the device for SAC with `train_freq = (n_steps, "step")`: `collect` adds `n_steps` raw
    transitions per env to a `DeviceReplayBuffer`, the actions drawn by `nets` (a `DeviceSACNetworks`, which stands where the others
    have their policy: `set_stream` and `use_torch_stream` move it).  `DeviceSACTrain.train` takes the buffer from there."""
    _create_entry = "fleet_saccollect_create"

    def __init__(self, env, nets, stats_window: int = 100):
        super().__init__(env, nets, stats_window)
        self.nets = nets

    def collect_dev(self, args: "_capi.FleetSacCollectArgs"):
        """Raw device addresses in a FleetSacCollectArgs, on the stream the borrowed handles share."""
        args.struct_bytes = C.sizeof(_capi.FleetSacCollectArgs)
        self._check(self.lib.fleet_saccollect_sac_dev(self.h, C.byref(args)))

    def collect(self, replay, n_steps: int, *, learning_starts: int, low: float = -1.0, high: float = 1.0, seed: int, first_step: int,
                env_id_offset: int = 0, stats_out=None):
        """`n_steps` env steps on torch's current stream, no host synchronisation.  Global step s = first_step + t draws uniform actions
        in [low, high) while s < learning_starts (`DeviceSACNetworks.sample_uniform`) and the squashed-Gaussian sample
        tanh(mean + exp(log_std) * eps) afterwards (`DeviceSACNetworks.act` on the carry observation), both keyed by (seed, s).  The
        buffer gets the action the env got.  Returns the statistics f64 [16] on the device."""
        self._lent = (replay,)
        self.use_torch_stream()
        a = _capi.FleetSacCollectArgs()
        a.n_steps, a.env_id_offset, a.replay = int(n_steps), int(env_id_offset), replay.h.value
        a.learning_starts = max(int(learning_starts), 0)
        a.noise_lo, a.noise_hi = float(low), float(high)
        a.seed, a.first_step = int(seed) & (2 ** 64 - 1), int(first_step) & (2 ** 64 - 1)
        stats_out, a.stats = self._stats(stats_out)
        self.collect_dev(a)
        return stats_out
