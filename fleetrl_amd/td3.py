"""`DeviceTD3Grad`: the critic and actor minibatch gradients of a TD3 / DDPG agent on the device (include/fleet_hip.h `fleet_td3_*`,
fleetrl_amd/csrc/fleet_td3.hip).

What SB3's `TD3.train` does with one minibatch between the target and the optimisers -- the two critic forwards, `F.mse_loss` summed
over the critics and its backward; on a delayed step `-critic.q1_forward(obs, actor(obs)).mean()` and its backward into the actor --
in two entries of two launches each.  The gradients land in the `.grad` of torch's own parameters, so the optimisers follow
unchanged.  Deterministic by construction: no atomics, every sum in a fixed order.  The networks that are differentiated are the
image of a `DeviceTD3Target` made from the ONLINE actor and critics (a second one beside the targets'): call its
`load_torch(params)` after every optimiser step.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from ._handle import _ImageBorrower

__all__ = ["DeviceTD3Grad", "CRITIC_STATS", "ACTOR_STATS"]

CRITIC_STATS = ("critic_loss", "critic_0_loss", "critic_1_loss")
ACTOR_STATS = ("actor_loss",)


class DeviceTD3Grad(_ImageBorrower):
    """One `fleet_td3_*` handle on `nets` (a `DeviceTD3Target` that holds the online networks, which must outlive it) for minibatches
    of at most `max_batch` rows.  It launches on `nets`' stream."""
    _prefix = "td3"

    def __init__(self, nets, max_batch: int):
        self.nets = nets
        self.obs_dim, self.act_dim, self.n_critics, self.max_batch = nets.obs_dim, nets.act_dim, nets.n_critics, int(max_batch)
        self._open_on(nets, "fleet_td3_create", _capi.FleetTd3Params(C.sizeof(_capi.FleetTd3Params), self.max_batch))
        flat = [tuple(s) for pair in nets._shapes for s in pair]
        n_actor = 2 * len(nets.describe()["actor"]["widths"])
        self._shapes = {"actor": flat[:n_actor], "critic": flat[n_actor:]}
        self.tile_rows = self.describe()["tile_rows"]

    def describe(self) -> dict:
        """What fleet_td3_describe reports: max_batch, the bytes of the scratch, the rows one workgroup of a rows launch takes."""
        p, nbytes, rows = _capi.FleetTd3Params(), C.c_uint64(), C.c_int32()
        self._check(self.lib.fleet_td3_describe(self.h, C.byref(p), C.byref(nbytes), C.byref(rows)))
        return {"max_batch": p.max_batch, "scratch_bytes": int(nbytes.value), "tile_rows": int(rows.value)}

    def critic_grad_dev(self, args: "_capi.FleetTd3CriticArgs", grad_ptrs, count: int):
        """Raw device addresses in a FleetTd3CriticArgs and a (c_void_p * count) array, on the networks handle's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetTd3CriticArgs)
        self._check(self.lib.fleet_td3_critic_grad_dev(self.h, C.byref(args), grad_ptrs, int(count)))

    def actor_grad_dev(self, args: "_capi.FleetTd3ActorArgs", grad_ptrs, count: int):
        args.struct_bytes = C.sizeof(_capi.FleetTd3ActorArgs)
        self._check(self.lib.fleet_td3_actor_grad_dev(self.h, C.byref(args), grad_ptrs, int(count)))

    def critic_grad(self, batch_or_tensors, target_q, *, into, q_out=None, stats_out=None):
        """The critic loss of one minibatch and its gradients, two launches on torch's current stream, no host synchronisation.
        batch_or_tensors: what `DeviceReplayBuffer.sample` yields (observations f32 [B, obs_dim], actions f32 [B, act_dim]) or the
        pair (obs, actions); target_q f32 [B] (or [B, 1]): what `DeviceTD3Target.target` wrote.  into: the critics' torch parameters,
        W, b per layer, critic 0's then critic 1's; their `.grad` is allocated on the first call and OVERWRITTEN by every call (there
        is nothing to zero).  q_out f32 [B, n_critics]: the critics' outputs.  Returns stats f32 [8] on the device: `CRITIC_STATS`
        (the summed loss, then each critic's), then zeros."""
        import torch

        self.use_torch_stream()
        f32 = (torch.float32,)
        if hasattr(batch_or_tensors, "observations"):
            obs, actions = batch_or_tensors.observations, batch_or_tensors.actions
        else:
            obs, actions = batch_or_tensors
        B = int(obs.shape[0]) if obs.ndim == 2 else 0
        a = _capi.FleetTd3CriticArgs()
        a.B = B
        keep = [self._tensor(obs, (B, self.obs_dim), f32), self._tensor(actions, (B, self.act_dim), f32),
                self._tensor(target_q.detach(), (B,), f32)]
        a.obs, a.actions, a.target_q = (t.data_ptr() for t in keep)
        if stats_out is None:
            stats_out = torch.empty(8, device=obs.device, dtype=torch.float32)
        a.stats = self._tensor(stats_out, (8,), f32).data_ptr()
        if q_out is not None:
            keep.append(self._tensor(q_out, (B, self.n_critics), f32))
            a.q = keep[-1].data_ptr()
        arr = self._grad_pointers("critic", into, self._shapes["critic"], "critic 0's, then critic 1's")
        self.critic_grad_dev(a, arr, len(self._shapes["critic"]))
        return stats_out

    def actor_grad(self, obs, *, into, actions_out=None, q_out=None, stats_out=None):
        """The actor loss -mean(Q_0(obs, pi(obs))) of one minibatch and its gradients in the ACTOR's parameters, two launches on torch's
        current stream.  obs f32 [B, obs_dim]; into: the actor's torch parameters, W, b per layer (`.grad` as for `critic_grad`; the
        critics' `.grad` is not touched).  actions_out f32 [B, act_dim]: pi(obs); q_out f32 [B]: Q_0(obs, pi(obs)).  Returns stats f32
        [8] on the device: `ACTOR_STATS`, then zeros."""
        import torch

        self.use_torch_stream()
        f32 = (torch.float32,)
        B = int(obs.shape[0]) if obs.ndim == 2 else 0
        a = _capi.FleetTd3ActorArgs()
        a.B = B
        keep = [self._tensor(obs, (B, self.obs_dim), f32)]
        a.obs = keep[0].data_ptr()
        if stats_out is None:
            stats_out = torch.empty(8, device=obs.device, dtype=torch.float32)
        a.stats = self._tensor(stats_out, (8,), f32).data_ptr()
        for name, t, shape in (("actions_out", actions_out, (B, self.act_dim)), ("q", q_out, (B,))):
            if t is not None:
                keep.append(self._tensor(t, shape, f32))
                setattr(a, name, keep[-1].data_ptr())
        arr = self._grad_pointers("actor", into, self._shapes["actor"], "the actor's")
        self.actor_grad_dev(a, arr, len(self._shapes["actor"]))
        return stats_out
