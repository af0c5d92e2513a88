"""`DevicePPOGrad`: the gradients of PPO's minibatch loss on the device (include/fleet_hip.h `fleet_ppo_*`,
fleetrl_amd/csrc/fleet_ppo.hip).

What SB3's `PPO.train` does with one minibatch before the optimiser -- `evaluate_actions`, the clipped loss and `loss.backward()`
-- in two launches on a two-head `DevicePolicy`'s weights: the gradients land in the `.grad` of torch's own
parameters, so `clip_grad_norm_` and `opt.step()` follow unchanged.  Deterministic by construction: no atomics, every sum in a fixed
order.  `clip_range_vf` is SB3's: `None` for the plain squared error, a positive float to clip the value prediction around the batch's
`old_values` inside the same two launches (`fleet_ppo_grad_vclip_dev`).  The optimiser and the advantage normalisation stay the
caller's.  The device policy's image is what is differentiated: call `policy.load_torch(params)` after every optimiser step.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._handle import _ImageBorrower

__all__ = ["DevicePPOGrad", "STATS", "check_clip_range_vf"]

STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")


def check_clip_range_vf(clip_range_vf):
    """None, or the positive finite float: SB3 refuses the rest in the same words."""
    if clip_range_vf is None:
        return None
    cv = float(clip_range_vf)
    if not (cv > 0.0 and cv != float("inf")):
        raise ValueError(f"`clip_range_vf` must be positive, pass `None` to deactivate vf clipping (got {clip_range_vf!r})")
    return cv


class DevicePPOGrad(_ImageBorrower):
    """One `fleet_ppo_*` handle on `policy` (a `DevicePolicy` with a critic of width 1, which must outlive it) for minibatches of at
    most `max_batch` rows.  It launches on the policy's stream."""
    _prefix = "ppo"

    def __init__(self, policy, max_batch: int):
        self.policy = policy
        self.obs_dim, self.act_dim, self.max_batch = policy.obs_dim, policy.act_dim, int(max_batch)
        self._open_on(policy, "fleet_ppo_create", _capi.FleetPpoParams(C.sizeof(_capi.FleetPpoParams), self.max_batch))
        self._shapes = [tuple(s) for pair in policy._shapes for s in pair] + [(self.act_dim,)]
        self.tile_rows = self.describe()["tile_rows"]

    def describe(self) -> dict:
        """What fleet_ppo_describe reports: max_batch, the bytes of the scratch, the rows one workgroup of the rows launch takes."""
        p, nbytes, rows = _capi.FleetPpoParams(), C.c_uint64(), C.c_int32()
        self._check(self.lib.fleet_ppo_describe(self.h, C.byref(p), C.byref(nbytes), C.byref(rows)))
        return {"max_batch": p.max_batch, "scratch_bytes": int(nbytes.value), "tile_rows": int(rows.value)}

    def grad_dev(self, args: "_capi.FleetPpoGradArgs", grad_ptrs, count: int):
        """Raw device addresses in a FleetPpoGradArgs and a (c_void_p * count) array, on the policy's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetPpoGradArgs)
        self._check(self.lib.fleet_ppo_grad_dev(self.h, C.byref(args), grad_ptrs, int(count)))

    def grad_vclip_dev(self, args: "_capi.FleetPpoGradVclipArgs", grad_ptrs, count: int):
        """The same through fleet_ppo_grad_vclip_dev: a FleetPpoGradVclipArgs, whose `base` is a FleetPpoGradArgs."""
        args.struct_bytes, args.base.struct_bytes = C.sizeof(_capi.FleetPpoGradVclipArgs), C.sizeof(_capi.FleetPpoGradArgs)
        self._check(self.lib.fleet_ppo_grad_vclip_dev(self.h, C.byref(args), grad_ptrs, int(count)))

    def grad_gated_dev(self, args: "_capi.FleetPpoGradGatedArgs", grad_ptrs, count: int):
        """The same through fleet_ppo_grad_gated_dev: a FleetPpoGradGatedArgs, whose `base` is a FleetPpoGradArgs."""
        args.struct_bytes, args.base.struct_bytes = C.sizeof(_capi.FleetPpoGradGatedArgs), C.sizeof(_capi.FleetPpoGradArgs)
        self._check(self.lib.fleet_ppo_grad_gated_dev(self.h, C.byref(args), grad_ptrs, int(count)))

    def grad(self, batch, log_std, clip_range: float, vf_coef: float, ent_coef: float, *, into, values_out=None, log_prob_out=None,
             advantages=None, stats_out=None, clip_range_vf=None, gate=None):
        """The loss of one minibatch and its gradients, two launches on torch's current stream, no host synchronisation.
        batch: what `DeviceRolloutBuffer.get` yields (observations f32 [B, obs_dim], actions f32 [B, act_dim], old_log_prob,
        advantages, returns f32 [B]); `advantages` replaces the batch's (the normalised ones).  log_std: the torch parameter f32
        [act_dim], read when the launch runs.  into: the torch parameters in `DevicePolicy.load_torch`'s order, then log_std; their
        `.grad` is allocated on the first call and OVERWRITTEN by every call (there is nothing to zero).  values_out, log_prob_out
        f32 [B]: the critic's (unclipped) values and the new log-probabilities.  clip_range_vf: None, or SB3's positive float: the value
        loss is then taken on `old_values + clamp(values - old_values, -clip_range_vf, clip_range_vf)` with the batch's `old_values`
        f32 [B].  gate: None, or (skip, decided, threshold) for early stopping on approx_kl (`fleet_ppo_grad_gated_dev`): two
        DIFFERENT one-element int32 / uint32 device tensors and a float.  When `skip` (written by something enqueued earlier) is
        nonzero, both launches return at once and write nothing; otherwise they run as without a gate and also write
        `decided = float64(stats[4]) > threshold`.  Returns stats f32 [8] on the device: `STATS`, then two zeros."""
        import torch

        cv = check_clip_range_vf(clip_range_vf)
        if gate is not None:
            skip, decided, threshold = gate
            threshold = float(threshold)
            if threshold != threshold:
                raise ValueError("gate: the threshold is NaN")
        self.use_torch_stream()
        f32 = (torch.float32,)
        obs = batch.observations
        B = int(obs.shape[0]) if obs.ndim == 2 else 0
        adv = batch.advantages if advantages is None else advantages
        v = None if cv is None else _capi.FleetPpoGradVclipArgs()
        a = _capi.FleetPpoGradArgs() if v is None else v.base
        a.B = B
        keep = [self._tensor(obs, (B, self.obs_dim), f32), self._tensor(batch.actions, (B, self.act_dim), f32),
                self._tensor(batch.old_log_prob, (B,), f32), self._tensor(adv.detach(), (B,), f32), self._tensor(batch.returns, (B,), f32),
                self._tensor(log_std.detach(), (self.act_dim,), f32)]
        a.obs, a.actions, a.old_log_prob, a.advantages, a.returns, a.log_std = (t.data_ptr() for t in keep)
        a.clip_range, a.vf_coef, a.ent_coef = float(clip_range), float(vf_coef), float(ent_coef)
        if stats_out is None:
            stats_out = torch.empty(8, device=obs.device, dtype=torch.float32)
        a.stats = self._tensor(stats_out, (8,), f32).data_ptr()
        for name, t in (("values", values_out), ("log_prob", log_prob_out)):
            if t is not None:
                keep.append(self._tensor(t, (B,), f32))
                setattr(a, name, keep[-1].data_ptr())
        arr = self._grad_pointers("grad", into, self._shapes, "the actor's then the critic's, then log_std")
        if gate is not None:
            words = (torch.int32, torch.uint32) if hasattr(torch, "uint32") else (torch.int32,)
            g = _capi.FleetPpoGradGatedArgs()
            g.base = a  # (a copy: `a` is complete by now)
            keep += [self._tensor(skip, (1,), words), self._tensor(decided, (1,), words)]
            g.gate.skip, g.gate.decided, g.gate.threshold = keep[-2].data_ptr(), keep[-1].data_ptr(), threshold
            if cv is not None:
                keep.append(self._tensor(batch.old_values, (B,), f32))
                g.old_values, g.clip_range_vf = keep[-1].data_ptr(), cv
            self.grad_gated_dev(g, arr, len(self._shapes))
            return stats_out
        if v is None:
            self.grad_dev(a, arr, len(self._shapes))
        else:
            keep.append(self._tensor(batch.old_values, (B,), f32))
            v.old_values, v.clip_range_vf = keep[-1].data_ptr(), cv
            self.grad_vclip_dev(v, arr, len(self._shapes))
        return stats_out
