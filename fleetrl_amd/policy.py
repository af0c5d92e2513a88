"""`DevicePolicy`: the deterministic forward pass of a trained stable-baselines3 MLP policy on the device, and `evaluate_policy`,
SB3's evaluation loop with everything but the episode quotas on the GPU.

The forward is one launch (fleetrl_amd/csrc/fleet_policy.hip, include/fleet_hip.h `fleet_policy_*`): it takes raw or normalised
observations, applies a normaliser's frozen statistics where asked, runs the actor and optionally the critic, and writes float32
actions `FleetVecEnv.step_torch` reads directly.  The weights come from a state dict, from the `policy.pth` of an SB3 archive (read
with `zipfile` and `torch.load(weights_only=True)`: SB3 itself is not needed) or from plain arrays.

Exploration is one launch as well (`fleet_explore_act_dev`): `sample` draws PPO's Gaussian action, its clipped twin for the env,
the summed log-probability and the value; `explore` adds TD3's action noise to the deterministic action; `sample_uniform` is the
warm-up's `action_space.sample()`.  The noise is counter-based (Philox4x32-10 keyed by seed, global env id, step and column), so a
run is reproducible from (seed, step) alone.  `predict` and `evaluate_policy` stay deterministic; training -- the backward pass --
stays the caller's.
"""
from __future__ import annotations

import ctypes as C
import io
import re
import zipfile

import numpy as np

from . import _capi
from ._mlp import _MlpHandle, _arrays
from .replay import _norm_handle

__all__ = ["DevicePolicy", "evaluate_policy"]

# keys of an SB3 policy's state dict that carry nothing the deterministic forward needs
_IGNORED = re.compile(r"^(actor_target|critic|critic_target)\.|^actor\.log_std\.(weight|bias)$")


def _chain(sd: dict, prefix: str) -> list:
    """The linear layers `<prefix>.<n>.weight / .bias` of an nn.Sequential, in the order of n."""
    idx = sorted({int(m.group(1)) for k in sd for m in [re.match(re.escape(prefix) + r"\.(\d+)\.weight$", k)] if m})
    for n in idx:
        if f"{prefix}.{n}.bias" not in sd:
            raise ValueError(f"state dict has {prefix}.{n}.weight but no {prefix}.{n}.bias")
    return [(sd[f"{prefix}.{n}.weight"], sd[f"{prefix}.{n}.bias"]) for n in idx]


def _single(sd: dict, prefix: str) -> list:
    if f"{prefix}.weight" not in sd or f"{prefix}.bias" not in sd:
        raise ValueError(f"state dict has no {prefix}.weight / {prefix}.bias")
    return [(sd[f"{prefix}.weight"], sd[f"{prefix}.bias"])]


def parse_state_dict(sd: dict, activation: str | None = None) -> dict:
    """The networks of an SB3 policy's state dict as the arguments of `DevicePolicy`: {"layers", "critic_layers", "activation",
    "output"}.  Three families, told apart by their keys; anything else is refused with a ValueError that names the key."""
    keys = list(sd)

    def refuse(key, what):
        raise ValueError(f"unsupported policy: state-dict key {key!r} ({what}); DevicePolicy runs MlpPolicy networks with separate "
                         "actor and critic trunks over a flat observation")

    for k in keys:
        if "features_extractor" in k:
            refuse(k, "a learned features extractor: a CNN or a dict observation space")
        if k.startswith("mlp_extractor.shared_net."):
            refuse(k, "a trunk shared by actor and critic")
        if k == "log_std" and getattr(sd[k], "ndim", 1) > 1:
            refuse(k, "generalised state-dependent exploration")
    if any(k.startswith(("mlp_extractor.", "action_net.")) for k in keys):  # PPO / A2C
        known = re.compile(r"^(mlp_extractor\.(policy_net|value_net)\.\d+\.(weight|bias)|(action_net|value_net)\.(weight|bias)|log_std)$")
        for k in keys:
            if not known.match(k):
                refuse(k, "not part of an on-policy MlpPolicy")
        critic = None
        if "value_net.weight" in sd:
            critic = _chain(sd, "mlp_extractor.value_net") + _single(sd, "value_net")
        return {"layers": _chain(sd, "mlp_extractor.policy_net") + _single(sd, "action_net"), "critic_layers": critic,
                "activation": activation or "tanh", "output": "clip"}
    if any(k.startswith("actor.") for k in keys):
        known = re.compile(r"^actor\.(mu|latent_pi)\.\d+\.(weight|bias)$|^actor\.mu\.(weight|bias)$")
        for k in keys:
            if not known.match(k) and not _IGNORED.match(k):
                refuse(k, "not part of an off-policy MlpPolicy's actor")
        if any(k.startswith("actor.latent_pi.") for k in keys) or "actor.mu.weight" in sd:  # SAC: tanh(mu(latent_pi(obs)))
            layers = _chain(sd, "actor.latent_pi") + _single(sd, "actor.mu")
        else:  # TD3 / DDPG: mu = Sequential(Linear, ReLU, ..., Linear, Tanh)
            layers = _chain(sd, "actor.mu")
            if not layers:
                raise ValueError("state dict has no actor.mu.<n>.weight")
        return {"layers": layers, "critic_layers": None, "activation": activation or "relu", "output": "tanh"}
    refuse(keys[0] if keys else "<empty>", "no known policy family")


class DevicePolicy(_MlpHandle):
    """One `fleet_policy_*` handle: an actor and optionally a critic, each a chain of at most 4 linear layers of width <= 512 over
    the same observation of at most 8192 columns.  `layers` / `critic_layers`: [(W [out, in], b [out]), ...] (torch's layout;
    tensors or arrays).  activation: "tanh" | "relu" after every layer but the last; output: "none" | "clip" (to [low, high]) |
    "tanh" after the actor's last layer.  The critic's output is left as it is."""
    _prefix = "policy"

    def __init__(self, layers, critic_layers=None, activation: str = "tanh", output: str = "clip", low: float = -1.0,
                 high: float = 1.0, device: int = 0):
        self._set_transforms(activation, output)
        heads = [_arrays(layers)] + ([] if critic_layers is None else [_arrays(critic_layers)])
        if not heads[0]:
            raise ValueError("a policy needs at least one layer")
        self.obs_dim = int(heads[0][0][0].shape[1]) if heads[0][0][0].ndim == 2 else 0
        p = _capi.FleetPolicyParams()
        p.struct_bytes, p.obs_dim, p.n_heads = C.sizeof(_capi.FleetPolicyParams), self.obs_dim, len(heads)
        self._fill_head(p.head[0], "head 0", heads[0], self.obs_dim, output, low, high)
        for h, head in enumerate(heads[1:], 1):
            self._fill_head(p.head[h], f"head {h}", head, self.obs_dim)
        self.act_dim = int(heads[0][-1][0].shape[0])
        self.value_dim = int(heads[1][-1][0].shape[0]) if len(heads) > 1 else 0
        self._create(device, p, heads)

    # ---- constructors from SB3's files ---------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, activation: str | None = None, low: float = -1.0, high: float = 1.0, device: int = 0):
        """PPO / A2C (`mlp_extractor.policy_net.*`, `action_net.*`, and the critic `mlp_extractor.value_net.*`, `value_net.*`):
        the deterministic action is the mean clipped to the action space, tanh hidden layers unless `activation` says otherwise.
        TD3 / DDPG (`actor.mu.<n>.*`): ReLU, tanh output.  SAC (`actor.latent_pi.*`, `actor.mu.*`): tanh(mu), ReLU.  The
        activation is not stored in a state dict: pass the one the policy was trained with when it was not the default."""
        return cls(**parse_state_dict(dict(sd), activation), low=low, high=high, device=device)

    @classmethod
    def from_sb3_zip(cls, path, activation: str | None = None, low: float = -1.0, high: float = 1.0, device: int = 0):
        """From the `policy.pth` of an archive `model.save()` wrote."""
        return cls.from_state_dict(read_sb3_state_dict(path), activation, low=low, high=high, device=device)

    # ---- weights -------------------------------------------------------------------------------------------------------------
    def load_host(self, layers, critic_layers=None):
        """New weights of the same shapes from host arrays; FleetHipError (ERR_INVALID) when one is not finite."""
        heads = [_arrays(layers)] + ([] if critic_layers is None else [_arrays(critic_layers)])
        if [(w.shape, b.shape) for head in heads for w, b in head] != self._shapes:
            raise ValueError("load_host: the shapes differ from the policy's")
        packed = self._pack(heads)
        self._check(self.lib.fleet_policy_load_host(self.h, packed.ctypes.data))

    def load_torch(self, parameters):
        """New weights from torch's parameter tensors on the policy's device, in declaration order (W, b per layer, the actor's
        then the critic's): copied and re-laid by one launch on torch's current stream, no host synchronisation -- what a training
        loop calls after an optimiser step."""
        ptrs, keep = self._pointers("load_torch", parameters)
        self._check(self.lib.fleet_policy_load_dev(self.h, ptrs, len(keep)))

    # ---- the forward -----------------------------------------------------------------------------------------------------------
    def forward_dev(self, obs_ptr: int, num_envs: int, norm=None, actions_ptr: int | None = None, values_ptr: int | None = None):
        """Raw device addresses, on the policy's stream.  `norm`: a FleetVecNormalize, a DeviceNormalizer or None."""
        self._check(self.lib.fleet_policy_forward_dev(self.h, obs_ptr, int(num_envs), _norm_handle(norm), actions_ptr, values_ptr))

    def act(self, obs, normalizer=None, out=None, values_out=None):
        """obs f32 [E, obs_dim] on the policy's device -> actions f32 [E, act_dim], on torch's current stream.  normalizer (a
        FleetVecNormalize or a DeviceNormalizer): `obs` is RAW and goes through its statistics inside the launch.  values_out
        f32 [E, value_dim]: the critic's output as well (one launch for both)."""
        import torch

        self.use_torch_stream()
        E = int(obs.shape[0]) if obs.ndim == 2 else 0
        obs = self._tensor(obs, (E, self.obs_dim), (torch.float32,))
        if out is None:
            out = torch.empty((E, self.act_dim), device=obs.device, dtype=torch.float32)
        vp = None
        if values_out is not None:
            vp = self._tensor(values_out, (E, max(self.value_dim, 1)), (torch.float32,)).data_ptr()
        self.forward_dev(obs.data_ptr(), E, normalizer, self._tensor(out, (E, self.act_dim), (torch.float32,)).data_ptr(), vp)
        return out

    # ---- exploration ---------------------------------------------------------------------------------------------------------
    def explore_dev(self, obs_ptr: int | None, num_envs: int, norm, args: "_capi.FleetExploreArgs"):
        """Raw device addresses in a FleetExploreArgs, on the policy's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetExploreArgs)
        self._check(self.lib.fleet_explore_act_dev(self.h, obs_ptr, int(num_envs), _norm_handle(norm), C.byref(args)))

    def _explore(self, mode, obs, E, scale, shift, low, high, seed, step, env_id_offset, normalizer, actions_out, env_actions_out,
                 log_prob_out, values_out, mean_out, noise, noise_given, want_log_prob):
        import torch

        self.use_torch_stream()
        dev, f32, A = torch.device("cuda", self.device), (torch.float32,), self.act_dim
        a = _capi.FleetExploreArgs()
        a.mode, a.noise_mode = mode, _capi.EXPLORE_NOISE_GIVEN if noise_given else _capi.EXPLORE_NOISE_DRAW
        a.seed, a.step, a.env_id_offset = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(env_id_offset)
        a.noise_lo, a.noise_hi = float(low), float(high)
        keep = [self._per_action("scale", scale)] if scale is not None else []
        a.scale = keep[0].data_ptr() if keep else None
        if shift is not None:
            keep.append(self._per_action("shift", shift))
            a.shift = keep[-1].data_ptr()
        if obs is not None:
            obs = self._tensor(obs, (E, self.obs_dim), f32)

        def out(t, shape, make=True):
            if t is None:
                if not make:
                    return None
                t = torch.empty(shape, device=dev, dtype=torch.float32)
            return self._tensor(t, shape, f32)

        actions, env_actions = out(actions_out, (E, A)), out(env_actions_out, (E, A))
        log_prob = out(log_prob_out, (E,), want_log_prob)
        values = out(values_out, (E, max(self.value_dim, 1)), False)
        mean, noise = out(mean_out, (E, A), False), out(noise, (E, A), False)
        if noise_given and noise is None:
            raise ValueError("noise_given needs the noise tensor")
        a.actions, a.env_actions = actions.data_ptr(), env_actions.data_ptr()
        for name, t in (("log_prob", log_prob), ("values", values), ("mean", mean), ("noise", noise)):
            setattr(a, name, None if t is None else t.data_ptr())
        self.explore_dev(None if obs is None else obs.data_ptr(), E, normalizer, a)
        return actions, env_actions, log_prob, values

    def sample(self, obs, log_std, *, seed: int, step: int, env_id_offset: int = 0, normalizer=None, actions_out=None,
               env_actions_out=None, log_prob_out=None, values_out=None, mean_out=None, noise=None, noise_given: bool = False):
        """PPO's rollout step in one launch: obs f32 [E, obs_dim] -> (actions, env_actions, log_prob, values), SB3's
        DiagGaussianDistribution with the state-independent `log_std` (a torch parameter f32 [act_dim], read when the launch
        runs; a float or an array also does).  actions = mean + exp(log_std) * eps is what the buffer keeps, env_actions its
        output transform (the clip) is what the env steps on, log_prob f32 [E] is torch's Normal.log_prob of the stored action
        summed over the columns, values (None unless values_out is given) the critic's output.  eps is Philox noise of (seed,
        env_id_offset + row, step, column).  The *_out tensors may be the rows of `DeviceRolloutBuffer.slot(t)`; `noise` f32
        [E, act_dim] receives eps, or supplies it with noise_given.  A float `log_std` is cached on the device; one that changes
        from call to call costs a host synchronisation each time (pass the parameter tensor instead).  env_id_offset >= 0."""
        E = int(obs.shape[0]) if obs.ndim == 2 else 0
        return self._explore(_capi.EXPLORE_GAUSSIAN, obs, E, log_std, None, 0.0, 0.0, seed, step, env_id_offset, normalizer,
                             actions_out, env_actions_out, log_prob_out, values_out, mean_out, noise, noise_given, True)

    def explore(self, obs, sigma, *, shift=None, low: float = -1.0, high: float = 1.0, seed: int | None = None, step: int | None = None,
                env_id_offset: int = 0, normalizer=None, actions_out=None, env_actions_out=None, values_out=None, mean_out=None,
                noise=None, noise_given: bool = False, action_noise=None, done=None):
        """TD3 / DDPG's exploration step in one launch (SB3's `_sample_action` with NormalActionNoise): actions = env_actions =
        clip(act(obs) + shift + sigma * eps, low, high).  sigma, shift: floats, arrays or device tensors f32 [act_dim]; a float
        is cached on the device, and one that changes from call to call (a decaying sigma) costs a host synchronisation each
        time: keep such a value in a device tensor.
        action_noise (a DevicePinkNoise or a DeviceOUNoise of the same E and act_dim): eps is `action_noise.next(done)` -- `done` the
        env's done flags of the step before, so that an env's process starts afresh with its episode -- read through the given-noise
        path; seed, step and env_id_offset are then the process's own and not looked at here, `noise` (when given) receives the
        rows.  Without it, seed and step are required."""
        E = int(obs.shape[0]) if obs.ndim == 2 else 0
        if action_noise is not None:
            if noise_given:
                raise ValueError("action_noise and noise_given exclude each other")
            noise, noise_given, seed, step = action_noise.next(done, out=noise), True, 0, 0
        elif seed is None or step is None:
            raise TypeError("explore() needs seed= and step= unless action_noise= is given")
        return self._explore(_capi.EXPLORE_ACTION_NOISE, obs, E, sigma, shift, low, high, seed, step, env_id_offset, normalizer,
                             actions_out, env_actions_out, None, values_out, mean_out, noise, noise_given, False)

    def sample_uniform(self, num_envs: int, *, low: float = -1.0, high: float = 1.0, seed: int, step: int, env_id_offset: int = 0,
                       actions_out=None, env_actions_out=None, noise=None, noise_given: bool = False):
        """The warm-up's `action_space.sample()`: uniform actions low + (high - low) * u in [low, high), no network (where the
        float32 sum rounds up to `high` the kernel returns the float below it; low == high gives low)."""
        return self._explore(_capi.EXPLORE_UNIFORM, None, int(num_envs), None, None, low, high, seed, step, env_id_offset, None,
                             actions_out, env_actions_out, None, None, None, noise, noise_given, False)

    def predict(self, observation, state=None, episode_start=None, deterministic: bool = True):
        """SB3's `predict` for host callers: NumPy observations [E, obs_dim] (or one observation [obs_dim]) -> (actions, None)."""
        import torch

        if not deterministic:
            raise NotImplementedError("DevicePolicy computes the deterministic action only")
        x = np.asarray(observation, dtype=np.float32)
        single = x.ndim == 1
        x = np.array(x.reshape(-1, self.obs_dim))  # (a copy: torch wants a writable array)
        a = self.act(torch.from_numpy(x).to(torch.device("cuda", self.device))).cpu().numpy()
        return (a[0] if single else a), None

    def describe(self) -> dict:
        """What fleet_policy_describe reports: the shape of the network and `tile_rows`, the env rows one workgroup takes."""
        p = _capi.FleetPolicyParams()
        self._check(self.lib.fleet_policy_describe(self.h, C.byref(p)))
        return {"obs_dim": p.obs_dim, "n_heads": p.n_heads, "tile_rows": p.tile_rows,
                "heads": [self._head_dict(p.head[h]) for h in range(p.n_heads)]}


def read_sb3_state_dict(path) -> dict:
    """`policy.pth` of an SB3 archive as a state dict of CPU tensors (weights only: nothing in the archive is executed)."""
    import torch

    with zipfile.ZipFile(path) as zf:
        if "policy.pth" not in zf.namelist():
            raise ValueError(f"{path}: no policy.pth in the archive")
        return torch.load(io.BytesIO(zf.read("policy.pth")), map_location="cpu", weights_only=True)


def _quota_bookkeeping(done_log, reward_log, length_log, counts, targets, episode_rewards, episode_lengths) -> None:
    """SB3's inner loop over a block of steps that was read back: step by step, env by env, an env below its quota that finished
    contributes its episode."""
    for t in range(done_log.shape[0]):
        for i in np.flatnonzero(done_log[t]):
            if counts[i] < targets[i]:
                episode_rewards.append(float(reward_log[t, i]))
                episode_lengths.append(int(length_log[t, i]))
                counts[i] += 1


def _venv_parts(venv):
    """(torch device, steps per read-back, reset into a given tensor, whether `step` rounds its rewards to float32) of a
    FleetVecNormalize, a FleetVecEnv, or an object that has `device`, `episode_steps`, `reset_torch` and `step_torch` itself."""
    import torch

    inner = getattr(venv, "venv", venv)  # the FleetVecEnv under a FleetVecNormalize
    core = getattr(inner, "core", None)
    if core is None:
        return torch.device(venv.device), int(venv.episode_steps), (lambda obs: venv.reset_torch(obs_out=obs)), False
    dev = torch.device("cuda", core.batch.device)
    if hasattr(venv, "reset_torch"):
        return dev, int(core.params.episode_steps), (lambda obs: venv.reset_torch(obs_out=obs)), False

    def reset(obs):
        core.batch.use_torch_stream(dev)
        inner._torch_stream = torch.cuda.current_stream(dev).cuda_stream
        core.clear_start_overrides()
        core.batch.reset_dev(obs.data_ptr())

    return dev, int(core.params.episode_steps), reset, True  # (FleetVecEnv.step_wait hands SB3 float32 rewards)


def evaluate_policy(policy, venv, n_eval_episodes: int = 10, deterministic: bool = True, return_episode_rewards: bool = False):
    """stable-baselines3 2.3.2 `evaluate_policy` on an env without `Monitor`, on the device: env i owes
    `(n_eval_episodes + i) // n_envs` episodes, an episode's reward is the sum of what the env's step returns (float64 sums of
    the normalised rewards on a `FleetVecNormalize`), the result is (mean, std) or the two lists, episodes in the order SB3 meets
    them (step by step, env by env).  `venv`: a FleetVecEnv or a FleetVecNormalize.  Observations, actions, rewards, dones and the
    running sums stay on the device; the host reads the block's dones and sums back once per `episode_steps` steps to test the
    quotas, so the loop ends on the step SB3's would when episodes end on such a boundary (they do: every env of a FleetVecEnv
    runs episodes of `episode_steps` steps), and up to one block later otherwise."""
    import torch

    if not deterministic:
        raise NotImplementedError("evaluate_policy: stochastic actions are out of scope; deterministic=True only")
    n_envs = int(venv.num_envs)
    dev, block, reset, round32 = _venv_parts(venv)
    targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")
    counts = np.zeros(n_envs, dtype="int")
    episode_rewards, episode_lengths = [], []
    obs = torch.empty((n_envs, policy.obs_dim), device=dev, dtype=torch.float32)
    actions = torch.empty((n_envs, policy.act_dim), device=dev, dtype=torch.float32)
    reward = torch.empty(n_envs, device=dev, dtype=torch.float64)
    done = torch.empty(n_envs, device=dev, dtype=torch.uint8)
    sums = torch.zeros(n_envs, device=dev, dtype=torch.float64)
    lengths = torch.zeros(n_envs, device=dev, dtype=torch.int64)
    done_log = torch.empty((block, n_envs), device=dev, dtype=torch.uint8)
    sum_log = torch.empty((block, n_envs), device=dev, dtype=torch.float64)
    len_log = torch.empty((block, n_envs), device=dev, dtype=torch.int64)
    reset(obs)
    while (counts < targets).any():
        for t in range(block):
            policy.act(obs, out=actions)
            venv.step_torch(actions, obs_out=obs, reward_out=reward, done_out=done)
            sums += reward.float() if round32 else reward
            lengths += 1
            done_log[t].copy_(done)
            sum_log[t].copy_(sums)
            len_log[t].copy_(lengths)
            over = done != 0
            sums.masked_fill_(over, 0.0)
            lengths.masked_fill_(over, 0)
        _quota_bookkeeping(done_log.cpu().numpy(), sum_log.cpu().numpy(), len_log.cpu().numpy(), counts, targets, episode_rewards,
                           episode_lengths)
    if return_episode_rewards:
        return episode_rewards, episode_lengths
    return float(np.mean(episode_rewards)), float(np.std(episode_rewards))
