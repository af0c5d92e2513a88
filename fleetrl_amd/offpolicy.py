"""`DeviceTD3Train`: stable-baselines3's `TD3.train()` (and DDPG's) as one enqueue-only call (include/fleet_hip.h `fleet_offpolicy_*`,
fleetrl_amd/csrc/fleet_offpolicy.hip).

`gradient_steps` times: `DeviceReplayBuffer.sample` draws and gathers a minibatch, `DeviceTD3Target.target` forms the bootstrap target on
the target networks, `DeviceTD3Grad.critic_grad` and the critic optimiser's `DeviceAdam.step` update the online critics and -- on every
`policy_delay`-th update -- `actor_grad`, the actor optimiser's step and the Polyak update follow.  Every launch is the one the pieces
make on their own, in their order: the weights, the optimisers' states and the replay buffer's call counter end up bit-equal to the loop
of examples/td3_device_adam.py.  The Polyak update reads the ONLINE weight image, which the optimisers keep equal to torch's parameters:
one contiguous stream, no pointer array.  One block of statistics (`STATS`: what SB3 logs as `train/*`) is written at the end.
Deterministic from (buffer, weights, optimiser states, seed, first_update) to the weights.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._capi import FleetHipError
from ._handle import _ImageBorrower
from .replay import _norm_handle

__all__ = ["DeviceTD3Train", "STATS", "SB3_NAMES"]

# the statistics block f64[16]: the means over the call's gradient steps (the actor's over its actor steps, NaN without one), the last
# step's critic loss, the last actor step's actor loss (or NaN), the update count after the call, the call's actor steps; then zeros
STATS = ("critic_loss", "critic_0_loss", "critic_1_loss", "actor_loss", "last_critic_loss", "last_actor_loss", "n_updates", "actor_steps")
# SB3's logger keys where it has one, in STATS' order
SB3_NAMES = ("train/critic_loss", None, None, "train/actor_loss", None, None, "train/n_updates", None)


class DeviceTD3Train(_ImageBorrower):
    """One `fleet_offpolicy_*` handle on `replay` (a `DeviceReplayBuffer`), `targets` (the target networks' `DeviceTD3Target`), `grad` (a
    `DeviceTD3Grad`) and the optimisers `adam_actor` (`nets="actor"`) and `adam_critic` (`nets="critic"`), the last three on ONE second
    `DeviceTD3Target` that holds the online networks; all must outlive it.  A call takes at most `max_steps` gradient steps of at most
    `grad.max_batch` rows.  The optimisers' betas, eps and max_grad_norm are `adam_actor`'s and `adam_critic`'s."""
    _prefix = "offpolicy"

    def __init__(self, replay, targets, grad, adam_actor, adam_critic, max_steps: int = 1024):
        self.replay, self.targets, self.grad, self.adam_actor, self.adam_critic = replay, targets, grad, adam_actor, adam_critic
        self.nets = grad.nets
        self.lib = _capi.load_library()
        self._owner, self.device = grad.nets, grad.nets.device
        self.act_dim, self.max_steps = grad.act_dim, int(max_steps)
        h = C.c_void_p()
        p = _capi.FleetOffpolicyParams(C.sizeof(_capi.FleetOffpolicyParams), self.max_steps)
        rc = self.lib.fleet_offpolicy_create(replay.h, targets.h, grad.h, adam_actor.h, adam_critic.h, C.byref(p), C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self.lib.fleet_offpolicy_last_error(None).decode())
        self.h = h
        self._grad_cache = {}
        self._constants = {}  # _per_action's device tensors of float arguments
        self._shapes = {k: list(v) for k, v in grad._shapes.items()}
        self._ptrs = {}  # slot -> (the parameters, their pointer array, their addresses) of the last call

    def describe(self) -> dict:
        """What fleet_offpolicy_describe reports."""
        i = _capi.FleetOffpolicyInfo()
        self._check(self.lib.fleet_offpolicy_describe(self.h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in i._fields_ if n != "reserved"}

    def use_torch_stream(self, device=None):
        """The online networks, the target networks and the replay buffer all launch on torch's current stream from now on."""
        self._owner.use_torch_stream(device)
        self.targets.use_torch_stream(device)
        self.replay.use_torch_stream(device)

    def train_dev(self, args: "_capi.FleetOffpolicyArgs", actor_params, actor_grads, n_actor: int, critic_params, critic_grads, n_critic: int):
        """Raw device addresses in a FleetOffpolicyArgs and four (c_void_p * n) arrays, on the stream the borrowed handles share."""
        args.struct_bytes = C.sizeof(_capi.FleetOffpolicyArgs)
        self._check(self.lib.fleet_offpolicy_td3_dev(self.h, C.byref(args), actor_params, actor_grads, int(n_actor), critic_params,
                                                     critic_grads, int(n_critic)))

    def _param_pointers(self, slot, into):
        import torch

        into = list(into)
        hit = self._ptrs.get(slot)
        if hit is not None and len(hit[0]) == len(into) and all(a is b and a.data_ptr() == q for a, b, q in zip(hit[0], into, hit[2])):
            return hit[1]
        ptrs = [self._tensor(p.detach(), s, (torch.float32,)).data_ptr() for p, s in zip(into, self._shapes[slot])]
        self._ptrs[slot] = (into, (C.c_void_p * len(ptrs))(*ptrs), ptrs)
        return self._ptrs[slot][1]

    def train(self, actor_params, critic_params, *, gradient_steps: int, batch_size: int, gamma: float, tau: float, policy_delay: int,
              sigma, noise_clip: float, lr: float, seed: int, first_update: int, env=None, low: float = -1.0, high: float = 1.0,
              stats_out=None):
        """The whole update on torch's current stream, no host synchronisation.  actor_params / critic_params: the online networks' torch
        parameters (W, b per layer; critic 0's then critic 1's); they are stepped in place (and the online image with them), their
        `.grad` holds the last step's gradients.  sigma: the target-policy smoothing noise's scale, a float, an array or a device
        tensor f32 [act_dim] (0: DDPG); its noise is keyed by (seed, first_update + g).  first_update: the gradient steps taken so far.
        env: a FleetVecNormalize or a DeviceNormalizer whose statistics normalise the minibatches, or None.  Returns the statistics
        f64 [16] on the device: `STATS`, then zeros."""
        import torch

        self.use_torch_stream()
        a = _capi.FleetOffpolicyArgs()
        a.gradient_steps, a.batch_size, a.policy_delay = int(gradient_steps), int(batch_size), int(policy_delay)
        a.gamma, a.tau, a.noise_clip, a.act_lo, a.act_hi, a.lr = float(gamma), float(tau), float(noise_clip), float(low), float(high), float(lr)
        for o, opt in enumerate((self.adam_actor, self.adam_critic)):
            a.beta1[o], a.beta2[o], a.eps[o], a.max_grad_norm[o] = opt.betas[0], opt.betas[1], opt.eps, opt.max_grad_norm
        a.seed, a.first_update = int(seed) & (2 ** 64 - 1), int(first_update) & (2 ** 64 - 1)
        sig = self._per_action("sigma", sigma)
        a.sigma = sig.data_ptr()
        a.norm = _norm_handle(env)
        if stats_out is None:
            stats_out = torch.empty(_capi.TRAIN_STATS, device=torch.device("cuda", self.device), dtype=torch.float64)
        a.stats = self._tensor(stats_out, (_capi.TRAIN_STATS,), (torch.float64,)).data_ptr()
        ga = self._grad_pointers("actor", actor_params, self._shapes["actor"], "the actor's")
        gc = self._grad_pointers("critic", critic_params, self._shapes["critic"], "critic 0's, then critic 1's")
        self.train_dev(a, self._param_pointers("actor", actor_params), ga, len(self._shapes["actor"]),
                       self._param_pointers("critic", critic_params), gc, len(self._shapes["critic"]))
        return stats_out

    def polyak(self, tau: float):
        """The targets' image <- fmaf(tau, the online image, the targets' image * (1 - tau)) in one launch on torch's current stream: what
        `targets.polyak(online_parameters, tau)` gives, bit for bit, while the online image holds torch's parameters."""
        self.use_torch_stream()
        self._check(self.lib.fleet_offpolicy_polyak_dev(self.h, float(tau)))
