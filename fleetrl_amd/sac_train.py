"""`DeviceSACTrain`: stable-baselines3's `SAC.train()` as one enqueue-only call (include/fleet_hip.h `fleet_sactrain_*`,
fleetrl_amd/csrc/fleet_sactrain.hip).

`gradient_steps` times, in SB3's order of effects: `DeviceReplayBuffer.sample` draws and gathers a minibatch; with a learned entropy
coefficient alpha = exp(log_ent_coef) is formed BEFORE its optimiser steps; `DeviceSACNetworks.target` forms the soft bootstrap target;
`DeviceTD3Grad.critic_grad`, the critics' gradients times `loss_scale` and the critic optimiser's `DeviceAdam.step` update the critics;
`DeviceSACGrad.actor_grad` and the actor optimiser's step update the actor on the critics just stepped, and the entropy coefficient's
optimiser steps `log_ent_coef`; on the steps g of the call with `g % target_update_interval == 0` the target image is moved towards the
online image.  Every launch is the one the pieces make on their own (`fleetrl_amd.sac.gradient_step` with `alpha` for its `torch.exp`),
in their order: the weights, the optimisers' states and the replay buffer's call counter end up bit-equal.  One block of statistics
(`SAC_TRAIN_STATS`: what SB3 logs as `train/*`) is written at the end.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._capi import FleetHipError
from ._handle import _ImageBorrower
from .replay import _norm_handle
from .sac import CRITIC_LOSS_SCALE

__all__ = ["DeviceSACTrain", "SAC_TRAIN_STATS", "SAC_TRAIN_SB3_NAMES"]

# the statistics block f64[16]: the means over the call's gradient steps (ent_coef_loss: NaN with a fixed alpha), the last step's losses,
# the update count after the call, the call's target updates, the mean log-probability and the mean min-Q of the actor steps; then zeros
SAC_TRAIN_STATS = ("critic_loss", "actor_loss", "ent_coef", "ent_coef_loss", "last_critic_loss", "last_actor_loss", "n_updates",
                   "target_updates", "log_prob_mean", "qmin_mean")
# SB3's logger keys where it has one, in SAC_TRAIN_STATS' order
SAC_TRAIN_SB3_NAMES = ("train/critic_loss", "train/actor_loss", "train/ent_coef", "train/ent_coef_loss", None, None, "train/n_updates", None,
                       None, None)


class DeviceSACTrain(_ImageBorrower):
    """One `fleet_sactrain_*` handle on `replay` (a `DeviceReplayBuffer`), `targets` (the target critics' `DeviceSACNetworks`), `grad` (a
    `DeviceSACGrad`) and the optimisers `adam_actor` (`nets="actor"`), `adam_critic` (`nets="critic"`) and -- for a learned entropy
    coefficient -- `ent_adam` (`DeviceAdam(nets, [log_ent_coef], nets="none")`), the last four on ONE second `DeviceSACNetworks` that
    holds the online networks; all must outlive it.  A call takes at most `max_steps` gradient steps of at most `grad.max_batch` rows.
    The optimisers' betas, eps and max_grad_norm are the three `DeviceAdam`s'."""
    _prefix = "sactrain"

    def __init__(self, replay, targets, grad, adam_actor, adam_critic, ent_adam=None, max_steps: int = 1024):
        self.replay, self.targets, self.grad = replay, targets, grad
        self.adam_actor, self.adam_critic, self.ent_adam = adam_actor, adam_critic, ent_adam
        self.nets = grad.nets
        self.lib = _capi.load_library()
        self._owner, self.device = grad.nets, grad.nets.device
        self.act_dim, self.max_steps = grad.act_dim, int(max_steps)
        h = C.c_void_p()
        p = _capi.FleetSacTrainParams(C.sizeof(_capi.FleetSacTrainParams), self.max_steps)
        rc = self.lib.fleet_sactrain_create(replay.h, targets.h, grad.h, adam_actor.h, adam_critic.h, getattr(ent_adam, "h", None),
                                            C.byref(p), C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self.lib.fleet_sactrain_last_error(None).decode())
        self.h = h
        self._grad_cache = {}
        self._constants = {}  # a fixed float ent_coef's device tensor
        self._shapes = {k: list(v) for k, v in grad._shapes.items()}
        self._ptrs = {}  # slot -> (the parameters, their pointer array, their addresses) of the last call

    def describe(self) -> dict:
        """What fleet_sactrain_describe reports."""
        i = _capi.FleetSacTrainInfo()
        self._check(self.lib.fleet_sactrain_describe(self.h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in i._fields_ if n != "reserved"}

    def use_torch_stream(self, device=None):
        """The online networks, the target networks and the replay buffer all launch on torch's current stream from now on."""
        self._owner.use_torch_stream(device)
        self.targets.use_torch_stream(device)
        self.replay.use_torch_stream(device)

    def train_dev(self, args: "_capi.FleetSacTrainArgs", actor_params, actor_grads, n_actor: int, critic_params, critic_grads, n_critic: int):
        """Raw device addresses in a FleetSacTrainArgs and four (c_void_p * n) arrays, on the stream the borrowed handles share."""
        args.struct_bytes = C.sizeof(_capi.FleetSacTrainArgs)
        self._check(self.lib.fleet_sactrain_sac_dev(self.h, C.byref(args), actor_params, actor_grads, int(n_actor), critic_params,
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

    def train(self, actor_params, critic_params, *, gradient_steps: int, batch_size: int, gamma: float, tau: float, lr: float, seed: int,
              target_seed: int, first_update: int, target_update_interval: int = 1, ent_coef=None, log_ent_coef=None, target_entropy=None,
              loss_scale: float = CRITIC_LOSS_SCALE, env=None, stats_out=None):
        """The whole update on torch's current stream, no host synchronisation.  actor_params / critic_params: the online networks' torch
        parameters (W, b per layer; the actor's last pair the ONE `[2A, H]` pair; critic 0's then critic 1's); they are stepped in place
        (and the online image with them), their `.grad` holds the last step's gradients (the critics' times `loss_scale`).  Give exactly
        one of `ent_coef` (fixed: a device tensor f32 [1] or a float) and `log_ent_coef` (learned: the one-element leaf tensor the
        handle's `ent_adam` was made on; it is stepped in place).  seed / target_seed: the Philox keys of the actor step's and of the
        target's draws, both under step `first_update + g`.  first_update: the gradient steps taken so far.  target_update_interval: the
        targets move on the steps g of the CALL with g % interval == 0 (SB3's test).  target_entropy: default -act_dim (SB3's "auto").
        env: a FleetVecNormalize or a DeviceNormalizer whose statistics normalise the minibatches, or None.  Returns the statistics
        f64 [16] on the device: `SAC_TRAIN_STATS`, then zeros."""
        import torch

        if (ent_coef is None) == (log_ent_coef is None):
            raise ValueError("give exactly one of ent_coef (fixed) and log_ent_coef (learned)")
        self.use_torch_stream()
        f32 = (torch.float32,)
        a = _capi.FleetSacTrainArgs()
        a.gradient_steps, a.batch_size, a.target_update_interval = int(gradient_steps), int(batch_size), int(target_update_interval)
        a.gamma, a.tau, a.lr, a.loss_scale = float(gamma), float(tau), float(lr), float(loss_scale)
        a.target_entropy = -float(self.act_dim) if target_entropy is None else float(target_entropy)
        for o, opt in enumerate((self.adam_actor, self.adam_critic, self.ent_adam)):
            if opt is None:
                opt = self.adam_actor  # (not read: there is no third optimiser)
            a.beta1[o], a.beta2[o], a.eps[o], a.max_grad_norm[o] = opt.betas[0], opt.betas[1], opt.eps, opt.max_grad_norm
        a.seed, a.target_seed = int(seed) & (2 ** 64 - 1), int(target_seed) & (2 ** 64 - 1)
        a.first_update = int(first_update) & (2 ** 64 - 1)
        dev = torch.device("cuda", self.device)
        keep = []
        if log_ent_coef is not None:
            if log_ent_coef.grad is None:
                log_ent_coef.grad = torch.zeros_like(log_ent_coef)
            keep += [self._tensor(log_ent_coef.detach(), (1,), f32), self._tensor(log_ent_coef.grad, (1,), f32)]
            a.log_ent_coef, a.log_ent_coef_grad = keep[0].data_ptr(), keep[1].data_ptr()
        elif isinstance(ent_coef, torch.Tensor):
            keep.append(self._tensor(ent_coef.detach(), (1,), f32))
            a.ent_coef = keep[0].data_ptr()
        else:
            hit = self._constants.get("ent_coef")
            if hit is None or hit[0] != float(ent_coef):
                hit = self._constants["ent_coef"] = (float(ent_coef), torch.full((1,), float(ent_coef), device=dev, dtype=torch.float32))
            a.ent_coef = hit[1].data_ptr()
        a.norm = _norm_handle(env)
        if stats_out is None:
            stats_out = torch.empty(_capi.TRAIN_STATS, device=dev, dtype=torch.float64)
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
        self._check(self.lib.fleet_sactrain_polyak_dev(self.h, float(tau)))

    def alpha(self, log_ent_coef, out=None):
        """alpha = (float)exp((double)log_ent_coef) in one launch on torch's current stream, into `out` f32 [1] (made when None): the
        double exponential rounded once -- `numpy.float32(numpy.exp(numpy.float64(x)))` --, within one ulp of `torch.exp`."""
        import torch

        self.use_torch_stream()
        f32 = (torch.float32,)
        x = self._tensor(log_ent_coef.detach(), (1,), f32)
        if out is None:
            out = torch.empty(1, device=x.device, dtype=torch.float32)
        self._check(self.lib.fleet_sactrain_alpha_dev(self.h, x.data_ptr(), self._tensor(out, (1,), f32).data_ptr()))
        return out

    def scale(self, params, s: float):
        """The `.grad` of the critics' parameters (critic 0's, then critic 1's) times (float)s in one launch on torch's current stream:
        `torch._foreach_mul_([p.grad for p in params], s)`, bit for bit."""
        self.use_torch_stream()
        gc = self._grad_pointers("critic", params, self._shapes["critic"], "critic 0's, then critic 1's")
        self._check(self.lib.fleet_sactrain_scale_dev(self.h, gc, len(self._shapes["critic"]), float(s)))
