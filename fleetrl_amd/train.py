"""`DevicePPOTrain`: stable-baselines3's `PPO.train()` as one enqueue-only call (include/fleet_hip.h `fleet_train_*`,
fleetrl_amd/csrc/fleet_train.hip).

`n_epochs` passes over a finished `DeviceRolloutBuffer` in freshly shuffled minibatches: per minibatch one launch
shuffles, gathers and normalises the advantages, `DevicePPOGrad`'s two launches form the gradients and `DeviceAdam`'s two clip, step
and refresh the policy's weight image.  With SB3's `clip_range_vf` set, the gather also stages the buffer's values and the gradient
launches clip the value prediction around them (`fleet_train_ppo_vclip_dev`): still five launches per minibatch.  With SB3's
`target_kl` set (`fleet_train_ppo_kl_dev`) the device itself stops the update at the first minibatch whose `approx_kl` exceeds
`1.5 * target_kl`, before that minibatch's optimiser step: the remaining launches of the call read one word and return, the
statistics count what ran (`KL_STATS`), and the optimiser's step count is settled when it is next asked for.
The shuffle is a keyed bijection evaluated on the device -- no `torch.randperm`,
no permutation in memory --, every sum has a stated order, and one block of statistics (`STATS`: what SB3 logs as `train/*`) is
written at the end.  Deterministic from (buffer, weights, optimiser state, seed, first_epoch) to the weights.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._capi import FleetHipError
from ._handle import _ImageBorrower
from .ppo import check_clip_range_vf

__all__ = ["DevicePPOTrain", "STATS", "KL_STATS", "check_target_kl"]

# the statistics block f64[16]: the means over all minibatches, the last minibatch's loss, the number of minibatches, the buffer's
# explained variance, mean(exp(log_std)) after the last step; then zeros
STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss", "n_updates", "explained_variance", "std")
# SB3's logger keys, in STATS' order
SB3_NAMES = ("train/policy_gradient_loss", "train/value_loss", "train/entropy_loss", "train/approx_kl", "train/clip_fraction", "train/loss",
             "train/n_updates", "train/explained_variance", "train/std")
# slots 9 .. 13 of a `target_kl` call: optimiser steps taken, epochs entered (what SB3 adds to `_n_updates`), 1.0 when the update
# stopped early, the approx_kl that was compared last, and its mean over the LAST epoch entered -- SB3 clears its list every epoch, so
# this one, not STATS' approx_kl over all epochs, is what it logs as train/approx_kl
KL_STATS = ("n_steps", "n_epochs", "early_stop", "last_approx_kl", "epoch_approx_kl")
KL_SB3_NAMES = ("train/optimizer_steps", "train/epochs", "train/early_stop", "train/last_approx_kl", "train/approx_kl_last_epoch")


def check_target_kl(target_kl):
    """None, or the positive finite float."""
    if target_kl is None:
        return None
    kl = float(target_kl)
    if not (kl > 0.0 and kl != float("inf")):
        raise ValueError(f"`target_kl` must be positive and finite, pass `None` to deactivate early stopping (got {target_kl!r})")
    return kl


class DevicePPOTrain(_ImageBorrower):
    """One `fleet_train_*` handle on `buffer` (a `DeviceRolloutBuffer`), `grad` (a `DevicePPOGrad`) and `adam` (a `DeviceAdam` over both
    heads and `log_std`), which lie on one `DevicePolicy` and must outlive it.  Minibatches hold at most `grad.max_batch` rows.  It
    launches on the policy's stream; the optimiser's betas, eps and max_grad_norm are `adam`'s."""
    _prefix = "train"

    def __init__(self, buffer, grad, adam):
        self.buffer, self.grad, self.adam, self.policy = buffer, grad, adam, grad.policy
        self.lib = _capi.load_library()
        self._owner, self.device = grad.policy, grad.policy.device
        h = C.c_void_p()
        rc = self.lib.fleet_train_create(buffer.h, grad.h, adam.h, C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self.lib.fleet_train_last_error(None).decode())
        self.h = h
        self._grad_cache = {}
        self._shapes = list(grad._shapes)
        self._ptrs = None  # (the parameters, their pointer array, their addresses) of the last call

    def describe(self) -> dict:
        """What fleet_train_describe reports, and `old_values_offset` (fleet_train_describe_vclip): the bytes from `staging` to the
        old values f32 [max_batch] that the last value-clipped minibatch staged."""
        i = _capi.FleetTrainInfo()
        self._check(self.lib.fleet_train_describe(self.h, C.byref(i)))
        off = C.c_uint64()
        self._check(self.lib.fleet_train_describe_vclip(self.h, C.byref(off)))
        return {**{n: getattr(i, n) for n, _ in i._fields_}, "old_values_offset": int(off.value)}

    def use_torch_stream(self, device=None):
        """The policy and the buffer both launch on torch's current stream from now on."""
        self._owner.use_torch_stream(device)
        self.buffer.use_torch_stream(device)

    def train_dev(self, args: "_capi.FleetTrainPpoArgs", param_ptrs, grad_ptrs, count: int):
        """Raw device addresses in a FleetTrainPpoArgs and two (c_void_p * count) arrays, on the policy's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetTrainPpoArgs)
        self._check(self.lib.fleet_train_ppo_dev(self.h, C.byref(args), param_ptrs, grad_ptrs, int(count)))

    def train_vclip_dev(self, args: "_capi.FleetTrainPpoVclipArgs", param_ptrs, grad_ptrs, count: int):
        """The same through fleet_train_ppo_vclip_dev: a FleetTrainPpoVclipArgs, whose `base` is a FleetTrainPpoArgs."""
        args.struct_bytes, args.base.struct_bytes = C.sizeof(_capi.FleetTrainPpoVclipArgs), C.sizeof(_capi.FleetTrainPpoArgs)
        self._check(self.lib.fleet_train_ppo_vclip_dev(self.h, C.byref(args), param_ptrs, grad_ptrs, int(count)))

    def train_kl_dev(self, args: "_capi.FleetTrainPpoKlArgs", param_ptrs, grad_ptrs, count: int):
        """The same through fleet_train_ppo_kl_dev: a FleetTrainPpoKlArgs, whose `base` is a FleetTrainPpoArgs."""
        args.struct_bytes, args.base.struct_bytes = C.sizeof(_capi.FleetTrainPpoKlArgs), C.sizeof(_capi.FleetTrainPpoArgs)
        self._check(self.lib.fleet_train_ppo_kl_dev(self.h, C.byref(args), param_ptrs, grad_ptrs, int(count)))

    def _param_pointers(self, into):
        import torch

        into = list(into)
        hit = self._ptrs
        if hit is not None and len(hit[0]) == len(into) and all(a is b and a.data_ptr() == q for a, b, q in zip(hit[0], into, hit[2])):
            return hit[1]
        ptrs = [self._tensor(p.detach(), s, (torch.float32,)).data_ptr() for p, s in zip(into, self._shapes)]
        self._ptrs = (into, (C.c_void_p * len(ptrs))(*ptrs), ptrs)
        return self._ptrs[1]

    def train(self, into, *, n_epochs: int, batch_size: int, clip_range: float, vf_coef: float, ent_coef: float, lr: float,
              normalize_advantage: bool = True, seed: int, first_epoch: int, stats_out=None, clip_range_vf=None, target_kl=None):
        """The whole update on torch's current stream, no host synchronisation.  into: the torch parameters in
        `DevicePolicy.load_torch`'s order, then log_std; they are stepped in place (and the policy's image with them), their `.grad`
        holds the last minibatch's gradients.  Epoch e shuffles under (seed, first_epoch + e): pass the number of epochs trained so far.
        clip_range_vf: None, or SB3's positive float (the value loss on the prediction clipped around the buffer's values).
        target_kl: None (`fleet_train_ppo_dev` / `fleet_train_ppo_vclip_dev`, untouched), or SB3's positive float: the update stops at the first minibatch whose float32
        `approx_kl`, as float64, exceeds `1.5 * target_kl` -- before that minibatch's optimiser step and every later epoch; a NaN
        does not stop it.  The stopping minibatch's statistics count in the means.  One difference from SB3: after a stop `.grad`
        holds the STOPPING minibatch's gradients, which were formed but never applied (SB3 does not call `backward()` for it).
        The call stays enqueue-only, but it cannot be captured into a graph, and `adam.describe()["step"]` asked for right
        afterwards waits for the update to finish.
        Returns the statistics f64 [16] on the device: `STATS`, then zeros -- with target_kl `STATS`, `KL_STATS`, two zeros."""
        import torch

        cv = check_clip_range_vf(clip_range_vf)
        kl = check_target_kl(target_kl)
        if not self.buffer.full:
            raise FleetHipError(_capi.ERR_STATE, "train() needs a full rollout buffer")
        self.use_torch_stream()
        k = None if kl is None else _capi.FleetTrainPpoKlArgs()
        v = None if cv is None or k is not None else _capi.FleetTrainPpoVclipArgs()
        a = k.base if k is not None else (_capi.FleetTrainPpoArgs() if v is None else v.base)
        a.n_epochs, a.batch_size, a.normalize_advantage = int(n_epochs), int(batch_size), int(bool(normalize_advantage))
        a.clip_range, a.vf_coef, a.ent_coef, a.lr = float(clip_range), float(vf_coef), float(ent_coef), float(lr)
        a.beta1, a.beta2, a.eps, a.max_grad_norm = self.adam.betas[0], self.adam.betas[1], self.adam.eps, self.adam.max_grad_norm
        a.seed, a.first_epoch = int(seed), int(first_epoch)
        if stats_out is None:
            stats_out = torch.empty(_capi.TRAIN_STATS, device=torch.device("cuda", self.device), dtype=torch.float64)
        a.stats = self._tensor(stats_out, (_capi.TRAIN_STATS,), (torch.float64,)).data_ptr()
        grads = self._grad_pointers("train", into, self._shapes, "the actor's then the critic's, then log_std")
        if k is not None:
            k.target_kl, k.clip_range_vf = kl, 0.0 if cv is None else cv
            self.train_kl_dev(k, self._param_pointers(into), grads, len(self._shapes))
        elif v is None:
            self.train_dev(a, self._param_pointers(into), grads, len(self._shapes))
        else:
            v.clip_range_vf = cv
            self.train_vclip_dev(v, self._param_pointers(into), grads, len(self._shapes))
        return stats_out

    def indices(self, n: int, seed: int, epoch: int, start: int = 0, count: int | None = None, out=None):
        """The shuffle on its own: perm(n, seed, epoch, start .. start + count - 1) as int32 [count] on the device, one launch."""
        import torch

        self._owner.use_torch_stream()
        count = int(n) - int(start) if count is None else int(count)
        if count < 0:
            raise ValueError(f"count must be >= 0, got {count}")
        if out is None:
            out = torch.empty(count, device=torch.device("cuda", self.device), dtype=torch.int32)
        if count == 0:
            return out
        ptr = self._tensor(out, (count,), (torch.int32,)).data_ptr()
        self._check(self.lib.fleet_train_indices_dev(self.h, int(n), int(seed), int(epoch), int(start), count, ptr))
        return out
