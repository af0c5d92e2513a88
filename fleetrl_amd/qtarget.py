"""`DeviceTD3Target`: the target networks of a TD3 / DDPG agent on the device (include/fleet_hip.h `fleet_qtarget_*`,
fleetrl_amd/csrc/fleet_qtarget.hip).

The two blocks of an off-policy gradient step that need no gradient move into the library: `target` computes the bootstrap target
`r + (1 - d) * gamma * min_c Q'_c(s', clip(pi'(s') + clip(sigma * eps)))` of a minibatch in one launch, `polyak` blends the online
networks' parameters into the targets in one launch.  The target networks are therefore no `nn.Module`s: they live in the handle,
start as copies of the online networks (`load_torch`) and come back out with `export_torch` (checkpoints).  The losses, their backward
passes and the optimiser steps stay torch's.
"""
from __future__ import annotations

import ctypes as C
import re

from . import _capi
from ._mlp import _MlpHandle, _arrays
from .policy import _chain, read_sb3_state_dict

__all__ = ["DeviceTD3Target", "parse_target_state_dict"]

_KNOWN = re.compile(r"^(actor_target\.mu|critic_target\.qf[01])\.\d+\.(weight|bias)$")
# the online networks beside the targets in an SB3 TD3 / DDPG policy's state dict: nothing the targets need
_IGNORED = re.compile(r"^(actor\.mu|critic\.qf\d+)\.\d+\.(weight|bias)$")


def parse_target_state_dict(sd: dict) -> dict:
    """The target networks of an SB3 TD3 / DDPG policy's state dict as the arguments of `DeviceTD3Target`: {"actor_layers",
    "critics_layers"}, from `actor_target.mu.<n>.*` and `critic_target.qf0.<n>.*` (and `qf1`: TD3's twin).  The online networks'
    keys are passed over; anything else is refused with a ValueError that names the key."""
    for k in sd:
        if not _KNOWN.match(k) and not _IGNORED.match(k):
            raise ValueError(f"unsupported policy: state-dict key {k!r} is not part of a TD3 / DDPG MlpPolicy's target networks "
                             "(actor_target.mu.<n>, critic_target.qf0.<n>, critic_target.qf1.<n>)")
    actor = _chain(sd, "actor_target.mu")
    if not actor:
        raise ValueError("state dict has no actor_target.mu.<n>.weight")
    critics = [c for c in (_chain(sd, "critic_target.qf0"), _chain(sd, "critic_target.qf1")) if c]
    if not _chain(sd, "critic_target.qf0"):
        raise ValueError("state dict has no critic_target.qf0.<n>.weight")
    return {"actor_layers": actor, "critics_layers": critics}


class DeviceTD3Target(_MlpHandle):
    """One `fleet_qtarget_*` handle: a target actor over `obs_dim` columns and one (DDPG) or two (TD3) target critics over
    `obs_dim + act_dim` columns -- the observation, then the action -- each a chain of at most 4 linear layers of width <= 512.
    actor_layers: [(W [out, in], b [out]), ...]; critics_layers: one such list per critic, the last width 1.  activation: "tanh" |
    "relu" after every layer but the last, of every network; output: "none" | "clip" (to [low, high]) | "tanh" after the actor's
    last layer."""
    _prefix = "qtarget"

    def __init__(self, actor_layers, critics_layers, activation: str = "relu", output: str = "tanh", low: float = -1.0,
                 high: float = 1.0, device: int = 0):
        self._set_transforms(activation, output)
        nets = [_arrays(actor_layers)] + [_arrays(c) for c in critics_layers]
        if not nets[0] or len(nets) < 2 or len(nets) > 3 or not all(nets):
            raise ValueError("the targets are an actor and one or two critics, each of at least one layer")
        self.obs_dim = int(nets[0][0][0].shape[1]) if nets[0][0][0].ndim == 2 else 0
        self.act_dim = int(nets[0][-1][0].shape[0])
        self.n_critics = len(nets) - 1
        p = _capi.FleetQTargetParams()
        p.struct_bytes, p.obs_dim, p.n_critics = C.sizeof(_capi.FleetQTargetParams), self.obs_dim, self.n_critics
        self._fill_head(p.actor, "actor", nets[0], self.obs_dim, output, low, high)
        for c, net in enumerate(nets[1:]):
            self._fill_head(p.critic[c], f"critic {c}", net, self.obs_dim + self.act_dim)
        self._create(device, p, nets)

    # ---- constructors from SB3's files ---------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, activation: str = "relu", output: str = "tanh", low: float = -1.0, high: float = 1.0, device: int = 0):
        """From an SB3 TD3 / DDPG policy's state dict: `actor_target.mu.<n>.*`, `critic_target.qf0.<n>.*` and, for TD3,
        `critic_target.qf1.<n>.*`.  The activation is not stored in a state dict: pass the one the policy was trained with when it
        was not ReLU."""
        return cls(**parse_target_state_dict(dict(sd)), activation=activation, output=output, low=low, high=high, device=device)

    @classmethod
    def from_sb3_zip(cls, path, activation: str = "relu", output: str = "tanh", low: float = -1.0, high: float = 1.0, device: int = 0):
        """From the `policy.pth` of an archive `model.save()` wrote."""
        return cls.from_state_dict(read_sb3_state_dict(path), activation, output, low=low, high=high, device=device)

    # ---- weights -------------------------------------------------------------------------------------------------------------
    def load_torch(self, parameters):
        """A hard update: the targets become copies of torch's parameter tensors on the handle's device (W, b per layer: the
        actor's, then each critic's), re-laid by one launch on torch's current stream, no host synchronisation."""
        ptrs, keep = self._pointers("load_torch", parameters)
        self._check(self.lib.fleet_qtarget_load_dev(self.h, ptrs, len(keep)))

    def polyak(self, parameters, tau: float):
        """SB3's `polyak_update(online, target, tau)` in one launch: target <- fmaf(tau, online, target * (1 - tau)), float32.
        `parameters`: the ONLINE networks' tensors, ordered as for `load_torch`.  Enqueues only."""
        ptrs, keep = self._pointers("polyak", parameters)
        self._check(self.lib.fleet_qtarget_polyak_dev(self.h, ptrs, len(keep), float(tau)))

    def export_torch(self, out_tensors=None) -> list:
        """The target weights in torch's layout, into `out_tensors` (ordered and shaped as for `load_torch`; made when None)."""
        import torch

        if out_tensors is None:
            dev = torch.device("cuda", self.device)
            out_tensors = [torch.empty(tuple(s), device=dev, dtype=torch.float32) for pair in self._shapes for s in pair]
        ptrs, keep = self._pointers("export_torch", out_tensors)
        self._check(self.lib.fleet_qtarget_export_dev(self.h, ptrs, len(keep)))
        return keep

    # ---- the target ----------------------------------------------------------------------------------------------------------
    def target_dev(self, next_obs_ptr: int, rewards_ptr: int, dones_ptr: int, batch: int, args: "_capi.FleetQTargetArgs"):
        """Raw device addresses in a FleetQTargetArgs, on the handle's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetQTargetArgs)
        self._check(self.lib.fleet_qtarget_target_dev(self.h, next_obs_ptr, rewards_ptr, dones_ptr, int(batch), C.byref(args)))

    def target(self, next_obs, rewards, dones, *, gamma: float, sigma, noise_clip: float, low: float = -1.0, high: float = 1.0,
               seed: int, step: int, row_offset: int = 0, out=None, next_actions_out=None, q_out=None, noise=None,
               noise_given: bool = False):
        """The learning targets of a minibatch in one launch, on torch's current stream: next_obs f32 [B, obs_dim] (normalised, as
        `DeviceReplayBuffer.sample` returns it), rewards f32 [B] and dones f32 [B] (or [B, 1]) -> y f32 [B] (`out`, made when None),
        y = rewards + ((1 - dones) * gamma) * min_c Q'_c(next_obs, a'), a' = clip(pi'(next_obs) + clip(sigma * eps, +-noise_clip),
        low, high).  sigma: a float, an array or a device tensor f32 [act_dim] (0: DDPG).  eps is Philox noise of (seed, row_offset +
        row, step, column) -- give the target a seed of its own, not the exploration's -- or `noise` f32 [B, act_dim] with
        noise_given; without it a given `noise` receives the draw.  next_actions_out f32 [B, act_dim] and q_out f32 [B, n_critics]
        receive a' and the critics' outputs."""
        import torch

        self.use_torch_stream()
        f32, A = (torch.float32,), self.act_dim
        B = int(next_obs.shape[0]) if next_obs.ndim == 2 else 0
        next_obs = self._tensor(next_obs, (B, self.obs_dim), f32)
        rewards, dones = self._tensor(rewards, (B,), f32), self._tensor(dones, (B,), f32)
        if out is None:
            out = torch.empty((B,), device=next_obs.device, dtype=torch.float32)
        a = _capi.FleetQTargetArgs()
        a.noise_mode = _capi.EXPLORE_NOISE_GIVEN if noise_given else _capi.EXPLORE_NOISE_DRAW
        a.seed, a.step, a.row_offset = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(row_offset)
        a.gamma, a.noise_clip, a.act_lo, a.act_hi = float(gamma), float(noise_clip), float(low), float(high)
        sig = self._per_action("sigma", sigma)
        a.sigma = sig.data_ptr()
        a.target_q = self._tensor(out, (B,), f32).data_ptr()
        if noise_given and noise is None:
            raise ValueError("noise_given needs the noise tensor")
        keep = [sig]
        for name, t, shape in (("noise", noise, (B, A)), ("next_actions", next_actions_out, (B, A)), ("q", q_out, (B, self.n_critics))):
            if t is not None:
                keep.append(self._tensor(t, shape, f32))
                setattr(a, name, keep[-1].data_ptr())
        self.target_dev(next_obs.data_ptr(), rewards.data_ptr(), dones.data_ptr(), B, a)
        return out

    def describe(self) -> dict:
        """What fleet_qtarget_describe reports: the shapes of the networks and `tile_rows`, the rows one workgroup takes."""
        p = _capi.FleetQTargetParams()
        self._check(self.lib.fleet_qtarget_describe(self.h, C.byref(p)))
        return {"obs_dim": p.obs_dim, "act_dim": self.act_dim, "n_critics": p.n_critics, "tile_rows": p.tile_rows,
                "actor": self._head_dict(p.actor), "critics": [self._head_dict(p.critic[c]) for c in range(p.n_critics)]}
