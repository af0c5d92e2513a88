"""`DeviceEvalCallback`: stable-baselines3's `EvalCallback` as one enqueue-only call (include/fleet_hip.h `fleet_eval_*`,
include/fleet_hip_sac_loop.h `fleet_saceval_*`, fleetrl_amd/csrc/fleet_eval.hip).

The third call of an SB3-style iteration beside `DevicePPOCollect.collect` and `DevicePPOTrain.train`: every `eval_freq` steps
`evaluate(num_timesteps)` copies the training normaliser's statistics to the evaluation env's (`sync_envs_normalization`), runs
`n_eval_episodes` deterministic episodes (`evaluate_policy`: the forward, the env's step and the normaliser's step, each the launch the
pieces make on their own -- the episode lists are bit-equal to `sync_normalization` + `fleetrl_amd.evaluate_policy`), forms mean and std,
and keeps the best weights, all on the device: the host does not wait, and does not learn whether the agent improved until it asks
(`results()`).  A SAC agent (`DeviceSACNetworks`) is evaluated with its deterministic action tanh(mean); its snapshot is the whole
image, the actor and the critics.  Out of scope: stochastic evaluation, `real_time` envs, `callback_on_new_best`, success rates.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import FleetHipError
from ._handle import _DeviceHandle

__all__ = ["DeviceEvalCallback", "STATS"]

# the statistics block f64[16]; then zeros
STATS = ("mean_reward", "std_reward", "mean_ep_length", "std_ep_length", "episodes", "best_mean_reward", "new_best", "num_timesteps",
         "evaluations")


class DeviceEvalCallback(_DeviceHandle):
    """One `fleet_eval_*` handle on `policy` (a `DevicePolicy`, or a `DeviceSACNetworks`) and `eval_venv` (a `FleetVecEnv`, or a
    `FleetVecNormalize` over one), which must outlive it.  monitor: the env counts as `Monitor`-wrapped (what `make_vec_env` gives SB3): an episode's reward is the env's own
    raw episode return; without it, the sum of what the env's step returns (the normalised rewards on a `FleetVecNormalize`).
    train_normalizer (a `FleetVecNormalize` or a `DeviceNormalizer`): its statistics go to the evaluation env's before every
    evaluation.  max_episodes: the episode lists' length (default `n_eval_episodes`)."""
    _prefix = "eval"

    def __init__(self, policy, eval_venv, n_eval_episodes: int = 5, monitor: bool = True, train_normalizer=None, max_episodes: int | None = None):
        self.env, self.policy = eval_venv, policy
        self.venv = getattr(eval_venv, "venv", eval_venv)  # the FleetVecEnv under a FleetVecNormalize
        self.norm = getattr(eval_venv, "norm", None)
        core = self.venv.core
        if int(core.params.real_time):
            raise ValueError("DeviceEvalCallback: a real_time env is refused: its episodes have no fixed length in steps, and the number "
                             "of steps an evaluation takes is fixed when it is enqueued")
        self.train_norm = getattr(train_normalizer, "norm", train_normalizer)
        if self.train_norm is not None and self.norm is None:
            raise ValueError("DeviceEvalCallback: train_normalizer needs an evaluation env with a normaliser (a FleetVecNormalize)")
        self.batch = core.batch
        self.lib = _capi.load_library()
        self.device = int(self.batch.device)
        self.num_envs, self.obs_dim, self.act_dim = int(self.venv.num_envs), int(policy.obs_dim), int(policy.act_dim)
        self.n_eval_episodes, self.monitor = int(n_eval_episodes), bool(monitor)
        self.max_episodes = self.n_eval_episodes if max_episodes is None else int(max_episodes)
        self.episode_steps = int(core.params.episode_steps)
        h = C.c_void_p()
        p = _capi.FleetEvalParams(C.sizeof(_capi.FleetEvalParams), self.max_episodes)
        from .sac import DeviceSACNetworks

        self._sac = isinstance(policy, DeviceSACNetworks)  # the create and the load entries are then fleet_saceval_*'s
        create = self.lib.fleet_saceval_create if self._sac else self.lib.fleet_eval_create
        rc = create(self.batch.h, None if self.norm is None else self.norm.h, policy.h, C.byref(p), C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self.lib.fleet_eval_last_error(None).decode())
        self.h = h
        self._pending = None  # (num_timesteps, stats) of the last evaluation enqueued and not yet read
        self.evaluations_timesteps, self.evaluations_results, self.evaluations_length = [], [], []  # SB3's three lists

    # ---- streams -----------------------------------------------------------------------------------------------------------------
    def set_stream(self, hip_stream):
        """The handle has no stream of its own: the env's, the normaliser's and the policy's are set."""
        self.batch.set_stream(hip_stream)
        self.venv._torch_stream = hip_stream
        for h in (self.norm, self.policy):
            if h is not None:
                h.set_stream(hip_stream)

    def use_torch_stream(self, device=None):
        """The env, the normaliser and the policy all launch on torch's current stream from now on."""
        import torch

        cur = torch.cuda.current_stream(self.device if device is None else device).cuda_stream
        if getattr(self.venv, "_torch_stream", None) != cur:
            self.batch.set_stream(cur)
            self.venv._torch_stream = cur
        for h in (self.norm, self.policy):
            if h is not None:
                h.use_torch_stream(device)

    # ---- the handle --------------------------------------------------------------------------------------------------------------
    def describe(self) -> dict:
        """What fleet_eval_describe reports."""
        i = _capi.FleetEvalInfo()
        self._check(self.lib.fleet_eval_describe(self.h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in i._fields_}

    def arrays(self) -> dict:
        """Zero-copy tensors over the handle's block: obs, raw_obs [E, D], actions [E, A], raw_reward, reward, done, sums, lengths, counts
        [E], ep_reward, ep_length [max_episodes], listed, best_mean_reward, evaluations, gate [1], snapshot [snapshot_floats]."""
        if self._tensors is None:
            import torch

            from ._handle import _DeviceArray

            d, dev = self.describe(), torch.device("cuda", self.device)
            E, D, A, M = self.num_envs, self.obs_dim, self.act_dim, self.max_episodes
            spec = {"obs": ((E, D), "<f4"), "raw_obs": ((E, D), "<f4"), "actions": ((E, A), "<f4"), "raw_reward": ((E,), "<f8"), "reward": ((E,), "<f8"),
                    "done": ((E,), "|u1"), "sums": ((E,), "<f8"), "lengths": ((E,), "<i4"), "counts": ((E,), "<i4"), "ep_reward": ((M,), "<f8"),
                    "ep_length": ((M,), "<i4"), "listed": ((1,), "<i8"), "best_mean_reward": ((1,), "<f8"), "evaluations": ((1,), "<i8"),
                    "gate": ((1,), "<i4"), "snapshot": ((int(d["snapshot_floats"]),), "<f4")}
            self._tensors = {n: torch.as_tensor(_DeviceArray(d[n], shape, typestr, self), device=dev) for n, (shape, typestr) in spec.items()}
        return self._tensors

    def n_steps(self, n_eval_episodes: int | None = None) -> int:
        """The env steps SB3's loop takes: ceil(n_eval_episodes / num_envs) episodes of `episode_steps` steps."""
        n = self.n_eval_episodes if n_eval_episodes is None else int(n_eval_episodes)
        return -(-n // self.num_envs) * self.episode_steps

    def _stats(self, stats_out):
        import torch

        if stats_out is None:
            stats_out = torch.empty(_capi.EVAL_STATS, device=torch.device("cuda", self.device), dtype=torch.float64)
        return stats_out, self._tensor(stats_out, (_capi.EVAL_STATS,), (torch.float64,)).data_ptr()

    def run_dev(self, args: "_capi.FleetEvalArgs"):
        """Raw device addresses in a FleetEvalArgs, on the stream the borrowed handles share."""
        args.struct_bytes = C.sizeof(_capi.FleetEvalArgs)
        self._check(self.lib.fleet_eval_run_dev(self.h, C.byref(args)))

    def evaluate(self, num_timesteps: int = 0, *, n_eval_episodes: int | None = None, stats_out=None):
        """One evaluation on torch's current stream, no host synchronisation.  Returns the statistics f64 [16] on the device: `STATS`,
        then zeros.  `results()` reads what was enqueued."""
        self.use_torch_stream()
        self.venv.core.clear_start_overrides()
        n = self.n_eval_episodes if n_eval_episodes is None else int(n_eval_episodes)
        a = _capi.FleetEvalArgs()
        a.n_eval_episodes, a.n_steps, a.reward_source = n, self.n_steps(n), int(self.monitor)
        a.sync_from = None if self.train_norm is None else self.train_norm.h.value
        a.num_timesteps = int(num_timesteps) & (2 ** 64 - 1)
        stats_out, a.stats = self._stats(stats_out)
        self.run_dev(a)
        self._pending = (int(num_timesteps), stats_out)
        return stats_out

    def results(self) -> dict:
        """Synchronises.  The last evaluation as SB3 logs it; its episodes (in SB3's order) are appended to `evaluations_timesteps` /
        `evaluations_results` / `evaluations_length`.  The device keeps one evaluation's lists: an evaluation that was followed by
        another before `results()` was called is not listed (its effect on the best weights stands)."""
        if self._pending is None:
            raise FleetHipError(_capi.ERR_STATE, "DeviceEvalCallback.results: no evaluation has been enqueued since the last call")
        rewards, lengths = self.episodes()  # (waits for the stream: the statistics block is written)
        (steps, stats), self._pending = self._pending, None
        s = stats.cpu().numpy()
        self.evaluations_timesteps.append(steps)
        self.evaluations_results.append(rewards.tolist())
        self.evaluations_length.append(lengths.tolist())
        return {"eval/mean_reward": float(s[0]), "eval/mean_ep_length": float(s[2]), "std_reward": float(s[1]), "best_mean_reward": float(s[5]),
                "new_best": bool(s[6]), "num_timesteps": int(s[7])}

    def episodes(self):
        """(rewards f64 [n], lengths i32 [n]) of the last evaluation, in the order SB3 meets them.  Synchronous."""
        M = self.max_episodes
        ret, length, count = np.zeros(M, np.float64), np.zeros(M, np.int32), C.c_uint64()
        self._check(self.lib.fleet_eval_episodes_read(self.h, ret.ctypes.data, length.ctypes.data, C.byref(count)))
        n = min(count.value, M)
        return ret[:n], length[:n]

    def save_npz(self, path):
        """SB3's `evaluations.npz`: timesteps, results, ep_lengths (what `results()` has read so far)."""
        np.savez(path, timesteps=self.evaluations_timesteps, results=self.evaluations_results, ep_lengths=self.evaluations_length)

    # ---- the pieces on their own ---------------------------------------------------------------------------------------------------
    def sync_normalization(self, src=None):
        """`sync_envs_normalization` on the device: `src`'s (default: train_normalizer's) obs_rms and ret_rms into the evaluation
        env's normaliser, one launch, no host synchronisation."""
        src = self.train_norm if src is None else getattr(src, "norm", src)
        self.use_torch_stream()
        rc = self.lib.fleet_eval_sync_norm_dev(None if self.norm is None else self.norm.h, None if src is None else src.h)
        if rc != _capi.OK:
            raise FleetHipError(rc, self.lib.fleet_eval_last_error(None).decode())

    def clear(self):
        """The clearing launch on its own: sums, lengths, counts and the list count."""
        self.use_torch_stream()
        self._check(self.lib.fleet_eval_clear_dev(self.h))

    def episodes_dev(self, done, reward, ep_return=None, ep_len=None, *, n_eval_episodes: int, monitor: bool = False):
        """The bookkeeping launch on given device tensors u8 [E], f64 [E] (and f64 [E], i32 [E] with monitor), E <= num_envs."""
        import torch

        self.use_torch_stream()
        E = int(done.numel())
        done, reward = self._tensor(done, (E,), (torch.uint8,)), self._tensor(reward, (E,), (torch.float64,))
        ep_return = None if ep_return is None else self._tensor(ep_return, (E,), (torch.float64,))
        ep_len = None if ep_len is None else self._tensor(ep_len, (E,), (torch.int32,))
        self._check(self.lib.fleet_eval_episodes_dev(self.h, done.data_ptr(), reward.data_ptr(), None if ep_return is None else ep_return.data_ptr(),
                                                     None if ep_len is None else ep_len.data_ptr(), E, int(n_eval_episodes), int(bool(monitor))))

    # ---- the snapshot ------------------------------------------------------------------------------------------------------------
    def load_best_into(self, policy=None):
        """The best weights so far into `policy` (default: the evaluated one), a `DevicePolicy` (for a SAC agent: a `DeviceSACNetworks`)
        of the same layout; one launch."""
        policy = self.policy if policy is None else policy
        self.use_torch_stream()
        policy.use_torch_stream()
        load = self.lib.fleet_saceval_best_load_dev if self._sac else self.lib.fleet_eval_best_load_dev
        self._check(load(self.h, policy.h))

    def best_parameters(self, like=None):
        """The best weights so far as torch tensors in torch's layout and order (W, b per layer, the actor's then the critic's): written
        into `like` (e.g. the parameters `DevicePolicy.load_torch` reads) or into new tensors; one launch."""
        import torch

        shapes = [s for pair in self.policy._shapes for s in pair]
        if like is None:
            like = [torch.empty(tuple(s), device=torch.device("cuda", self.device), dtype=torch.float32) for s in shapes]
        self.use_torch_stream()
        ptrs, keep = self.policy._pointers("best_parameters", like)
        self._check(self.lib.fleet_eval_best_export_dev(self.h, ptrs, len(keep)))
        return list(like)

    def check_errors(self):
        """Passes through to the env's: waits for the stream, raises FleetHipError (ERR_STATE) on a device error."""
        self.batch.check_errors()
