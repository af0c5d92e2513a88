"""`DeviceSACNetworks`: the networks of a SAC agent on the device (include/fleet_hip.h `fleet_sac_*`, fleetrl_amd/csrc/fleet_sac.hip).

SB3's SAC actor -- `latent_pi`, then the two heads `mu` and `log_std` over the same input -- is stored as ONE chain whose last layer is
`[2A, H]`: rows 0..A-1 `mu`, rows A..2A-1 `log_std`.  The handle is a `fleet_qtarget` handle, so everything a `DeviceTD3Target` does
with its weights (`load_torch`, `polyak`, `export_torch`, `describe`) works tensor for tensor, `DeviceTD3Grad(nets, B).critic_grad`
gives the critics' gradients and `DeviceAdam(nets, ..., nets="critic")` steps them.  Two launches are this module's own: `act`, the
stochastic squashed-Gaussian action `tanh(mean + exp(log_std) * eps)` with its log-probability, and `target`, the entropy-regularised
bootstrap target `r + (1 - d) * gamma * (min_c Q'_c(s', a') - alpha * log pi(a'|s'))` with `a'` drawn from the ONLINE actor and the
critics of a second, TARGETS handle.

`DeviceSACGrad` adds the backward side (include/fleet_hip.h `fleet_sac_actor_grad_dev`, fleetrl_amd/csrc/fleet_td3.hip): the actor loss
`mean(alpha * log pi(a|s) - min_c Q_c(s, a))` with its gradient in the actor's parameters, and the entropy-coefficient loss with the
gradient of `log_ent_coef`, in two launches.  `actor_update` and `gradient_step` compose SB3's whole `SAC.train` step from it,
`critic_update`, `DeviceAdam` and `polyak`: torch's share of a gradient step is one `exp` of a one-element tensor.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import _capi
from ._capi import FleetHipError
from ._mlp import _arrays
from .policy import _chain, _single, read_sb3_state_dict
from .qtarget import DeviceTD3Target
from .replay import _norm_handle
from .td3 import DeviceTD3Grad

__all__ = ["DeviceSACNetworks", "DeviceSACGrad", "parse_sac_state_dict", "critic_update", "actor_update", "gradient_step",
           "fused_head_parameters", "CRITIC_LOSS_SCALE", "SAC_ACTOR_STATS"]

# what `DeviceSACGrad.actor_grad` returns in stats[0..4] (ent_coef_loss: 0 when log_ent_coef is not given)
SAC_ACTOR_STATS = ("actor_loss", "ent_coef_loss", "log_prob_mean", "qmin_mean", "ent_coef")

# SB3's SAC critic loss is 0.5 * sum_c mse(q_c, y); the TD3 gradient launches form sum_c mse(q_c, y)
CRITIC_LOSS_SCALE = 0.5

_KNOWN = re.compile(r"^actor\.latent_pi\.\d+\.(weight|bias)$|^actor\.(mu|log_std)\.(weight|bias)$|"
                    r"^(critic|critic_target)\.qf[01]\.\d+\.(weight|bias)$")


def critic_update(nets, targets, grad, adam, batch, critic_params, *, gamma: float, ent_coef, seed: int, step: int, stats_out=None,
                  loss_scale: float = CRITIC_LOSS_SCALE):
    """The critic half of one `SAC.train` gradient step, short of the Polyak update: `nets.target` (one launch), `grad.critic_grad` (a
    `DeviceTD3Grad` on `nets`; two launches), the gradients times `loss_scale` -- the launches' loss is sum_c mse(q_c, y), SB3's is 0.5
    times that --, and `adam.step()` (a `DeviceAdam` on `nets` with `nets="critic"`).  batch: what `DeviceReplayBuffer.sample` yields.
    stats_out f32 [8] receives the launches' UNSCALED losses (`loss_scale * stats_out[0]` is SB3's `critic_loss`).  Returns the
    target y f32 [B].  `targets.polyak(online_parameters, tau)` is the caller's, after whatever steps the actor."""
    import torch

    y = nets.target(targets, batch.next_observations, batch.rewards, batch.dones, gamma=gamma, ent_coef=ent_coef, seed=seed, step=step)
    grad.critic_grad(batch, y, into=critic_params, stats_out=stats_out)
    if loss_scale != 1.0:
        torch._foreach_mul_([p.grad for p in critic_params], float(loss_scale))
    adam.step()
    return y


def actor_update(grad, adam, obs, actor_params, *, ent_coef, seed: int, step: int, log_ent_coef=None, ent_adam=None, target_entropy=None,
                 stats_out=None, **outputs):
    """The actor half of one `SAC.train` gradient step: `grad.actor_grad` (a `DeviceSACGrad`; two launches) and `adam.step()` (a
    `DeviceAdam` on the networks with `nets="actor"`).  With `log_ent_coef` (a one-element leaf tensor on the device) the launches also
    write its `.grad`, and `ent_adam` -- a `DeviceAdam(nets, [log_ent_coef], nets="none")` -- steps it.  The critics are the image's:
    call this after `critic_update`, as SB3 does.  `outputs`: `actor_grad`'s optional tensors.  Returns the stats (`SAC_ACTOR_STATS`)."""
    if (log_ent_coef is None) != (ent_adam is None):
        raise ValueError("log_ent_coef and ent_adam are given together: a learned entropy coefficient has its own optimiser")
    stats = grad.actor_grad(obs, ent_coef=ent_coef, seed=seed, step=step, into=actor_params, log_ent_coef=log_ent_coef,
                            target_entropy=target_entropy, stats_out=stats_out, **outputs)
    adam.step()
    if ent_adam is not None:
        ent_adam.step()
    return stats


def gradient_step(nets, targets, grad, actor_adam, critic_adam, batch, actor_params, critic_params, *, gamma: float, tau: float, seed: int,
                  target_seed: int, step: int, ent_coef=None, log_ent_coef=None, ent_adam=None, target_entropy=None, alpha_out=None,
                  critic_stats_out=None, actor_stats_out=None):
    """One gradient step of SB3's `SAC.train`, in SB3's order of effects, with no autograd: (1) alpha = exp(log_ent_coef), read BEFORE
    its optimiser step, into `alpha_out` f32 [1] (made when None) -- or the fixed `ent_coef`; (2) `critic_update` under `target_seed`;
    (3) `actor_update` under `seed`, on the critics just stepped, which also steps `log_ent_coef`; (4) `targets.polyak` over the online
    parameters.  Give exactly one of `ent_coef` (fixed: a device tensor f32 [1] or a float) and `log_ent_coef` with `ent_adam`
    (learned).  Returns (critic stats, actor stats, alpha)."""
    import torch

    if (ent_coef is None) == (log_ent_coef is None):
        raise ValueError("give exactly one of ent_coef (fixed) and log_ent_coef (learned)")
    if log_ent_coef is not None:
        alpha = torch.exp(log_ent_coef.detach(), out=alpha_out)
    else:
        alpha = ent_coef
    cs = torch.empty(8, device=batch.observations.device, dtype=torch.float32) if critic_stats_out is None else critic_stats_out
    critic_update(nets, targets, grad, critic_adam, batch, critic_params, gamma=gamma, ent_coef=alpha, seed=target_seed, step=step,
                  stats_out=cs)
    st = actor_update(grad, actor_adam, batch.observations, actor_params, ent_coef=alpha, seed=seed, step=step, log_ent_coef=log_ent_coef,
                      ent_adam=ent_adam, target_entropy=target_entropy, stats_out=actor_stats_out)
    targets.polyak(list(actor_params) + list(critic_params), tau)
    return cs, st, alpha


def fused_head_parameters(actor):
    """The ONE `[2A, H]` / `[2A]` parameter pair of an SB3 SAC actor's two heads, made so that torch's own tensors follow it: one
    concatenated leaf per kind is allocated (the one copy this costs), and `actor.mu.{weight,bias}` / `actor.log_std.{weight,bias}` are
    re-pointed at its two halves -- `.data` AND `.grad` become views of the pair's storage and of the pair's `.grad`.  From then on a
    gradient written into the pair is the `.grad` of torch's `mu` and `log_std`, and an optimiser step on either side moves both, with
    no copy.  `actor`: anything with `mu` and `log_std` linear modules of one shape.  Returns (weight [2A, H], bias [2A]) leaves with
    zeroed `.grad`.  An optimiser built over `actor.parameters()` BEFORE this call keeps working: the parameter objects stay."""
    import torch

    pair = []
    for kind in ("weight", "bias"):
        m, l = getattr(actor.mu, kind), getattr(actor.log_std, kind)
        if m.shape != l.shape:
            raise ValueError(f"actor.mu.{kind} {tuple(m.shape)} and actor.log_std.{kind} {tuple(l.shape)} differ in shape")
        A = m.shape[0]
        full = torch.cat([m.detach(), l.detach()], 0).contiguous().requires_grad_(True)
        full.grad = torch.zeros_like(full)
        m.data, l.data = full.data[:A], full.data[A:]
        m.grad, l.grad = full.grad[:A], full.grad[A:]
        pair.append(full)
    return tuple(pair)


def parse_sac_state_dict(sd: dict, which: str = "online") -> dict:
    """The networks of an SB3 SAC policy's state dict as the arguments of `DeviceSACNetworks`: {"actor_layers", "critics_layers"}.
    The actor is `actor.latent_pi.<n>.*` followed by ONE layer, `actor.mu` and `actor.log_std` concatenated in that order along the
    output axis; the critics are `critic.qf<k>.<n>.*` (which="online") or `critic_target.qf<k>.<n>.*` (which="target"; SAC has no
    target actor, so the targets handle carries the online one, which nothing reads).  Any other key is refused by name."""
    if which not in ("online", "target"):
        raise ValueError(f"which must be 'online' or 'target', got {which!r}")
    for k in sd:
        if not _KNOWN.match(k):
            raise ValueError(f"unsupported policy: state-dict key {k!r} is not part of a SAC MlpPolicy (actor.latent_pi.<n>, actor.mu, "
                             "actor.log_std, critic.qf<k>.<n>, critic_target.qf<k>.<n>)")
    (mw, mb), (lw, lb) = _single(sd, "actor.mu")[0], _single(sd, "actor.log_std")[0]
    mw, mb, lw, lb = (np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32) for t in (mw, mb, lw, lb))
    if mw.shape != lw.shape or mb.shape != lb.shape:
        raise ValueError(f"actor.mu {mw.shape} and actor.log_std {lw.shape} differ in shape")
    actor = _chain(sd, "actor.latent_pi") + [(np.concatenate([mw, lw], 0), np.concatenate([mb, lb], 0))]
    prefix = "critic" if which == "online" else "critic_target"
    if not _chain(sd, f"{prefix}.qf0"):
        raise ValueError(f"state dict has no {prefix}.qf0.<n>.weight")
    critics = [c for c in (_chain(sd, f"{prefix}.qf0"), _chain(sd, f"{prefix}.qf1")) if c]
    return {"actor_layers": actor, "critics_layers": critics}


class DeviceSACNetworks(DeviceTD3Target):
    """One handle `fleet_sac_create` made: a squashed-Gaussian actor over `obs_dim` columns whose last layer is `[2 * act_dim, H]` (mu
    rows, then log_std rows) and one or two critics over `obs_dim + act_dim` columns.  actor_layers: [(W [out, in], b [out]), ...];
    critics_layers: one such list per critic, the last width 1.  activation: "tanh" | "relu" after every layer but the last, of
    every network (SB3's SAC default: "relu").  act_dim <= 256."""

    def __init__(self, actor_layers, critics_layers, activation: str = "relu", device: int = 0):
        self._set_transforms(activation, "none")
        nets = [_arrays(actor_layers)] + [_arrays(c) for c in critics_layers]
        if not nets[0] or len(nets) < 2 or len(nets) > 3 or not all(nets):
            raise ValueError("the networks are an actor and one or two critics, each of at least one layer")
        self.obs_dim = int(nets[0][0][0].shape[1]) if nets[0][0][0].ndim == 2 else 0
        wide = int(nets[0][-1][0].shape[0])
        self.act_dim = wide // 2  # (an odd width: refused by the library, with its reason)
        self.n_critics = len(nets) - 1
        p = _capi.FleetSacParams()
        p.struct_bytes, p.obs_dim, p.n_critics = C.sizeof(_capi.FleetSacParams), self.obs_dim, self.n_critics
        self._fill_head(p.actor, "actor", nets[0], self.obs_dim)
        for c, net in enumerate(nets[1:]):
            self._fill_head(p.critic[c], f"critic {c}", net, self.obs_dim + self.act_dim)
        self._create(device, p, nets)

    def _open(self, device: int, params, *more):
        """fleet_sac_create: the one entry of the handle's life that is not fleet_qtarget_*."""
        self.lib = _capi.load_library()
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.fleet_sac_create(self.device, C.byref(params), *more, C.byref(h))
        if rc != _capi.OK:
            raise FleetHipError(rc, self.lib.fleet_sac_last_error(None).decode())
        self.h = h
        self._stream = None

    # ---- constructors from SB3's files ---------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, sd, which: str = "online", activation: str = "relu", device: int = 0):
        """From an SB3 SAC policy's state dict (`parse_sac_state_dict`).  The activation is not stored in a state dict: pass the one
        the policy was trained with when it was not ReLU."""
        return cls(**parse_sac_state_dict(dict(sd), which), activation=activation, device=device)

    @classmethod
    def from_sb3_zip(cls, path, which: str = "online", activation: str = "relu", device: int = 0):
        """From the `policy.pth` of an archive `model.save()` wrote."""
        return cls.from_state_dict(read_sb3_state_dict(path), which, activation, device)

    # ---- the action ------------------------------------------------------------------------------------------------------------
    def act_dev(self, obs_ptr: int, num_envs: int, norm, args: "_capi.FleetSacActArgs"):
        """Raw device addresses in a FleetSacActArgs, on the handle's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetSacActArgs)
        self._check(self.lib.fleet_sac_act_dev(self.h, obs_ptr, int(num_envs), _norm_handle(norm), C.byref(args)))

    def act(self, obs, *, seed: int = 0, step: int = 0, deterministic: bool = False, env_id_offset: int = 0, normalizer=None, noise=None,
            noise_given: bool = False, actions_out=None, gaussian_actions_out=None, log_prob_out=None, mean_out=None, log_std_out=None):
        """SAC's action in one launch, on torch's current stream: obs f32 [E, obs_dim] -> actions f32 [E, act_dim], the squashed
        action tanh(mean + exp(log_std) * eps) that both the env and the replay buffer get (SB3's `Actor.forward`), log_std clamped
        to [-20, 2].  eps is Philox noise of (seed, env_id_offset + row, step, column) -- the bits `DevicePolicy.sample` draws under
        the same key -- or `noise` f32 [E, act_dim] with noise_given; without it a given `noise` receives the draw.
        log_prob_out f32 [E]: SB3's `SquashedDiagGaussianDistribution.log_prob`; gaussian_actions_out: the pre-squash action;
        mean_out / log_std_out: the heads (log_std clamped).  deterministic: tanh(mean), no noise, no log-probability.  normalizer:
        `obs` is RAW and goes through its statistics inside the launch.  Returns the actions."""
        import torch

        self.use_torch_stream()
        f32, A = (torch.float32,), self.act_dim
        E = int(obs.shape[0]) if obs.ndim == 2 else 0
        obs = self._tensor(obs, (E, self.obs_dim), f32)
        if actions_out is None:
            actions_out = torch.empty((E, A), device=obs.device, dtype=torch.float32)
        a = _capi.FleetSacActArgs()
        a.noise_mode = _capi.EXPLORE_NOISE_GIVEN if noise_given else _capi.EXPLORE_NOISE_DRAW
        a.deterministic, a.env_id_offset = int(bool(deterministic)), int(env_id_offset)
        a.seed, a.step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        if noise_given and noise is None:
            raise ValueError("noise_given needs the noise tensor")
        keep = [self._tensor(actions_out, (E, A), f32)]
        a.actions = keep[0].data_ptr()
        for name, t, shape in (("noise", noise, (E, A)), ("gaussian_actions", gaussian_actions_out, (E, A)), ("log_prob", log_prob_out, (E,)),
                               ("mean", mean_out, (E, A)), ("log_std", log_std_out, (E, A))):
            if t is not None:
                keep.append(self._tensor(t, shape, f32))
                setattr(a, name, keep[-1].data_ptr())
        self.act_dev(obs.data_ptr(), E, normalizer, a)
        return actions_out

    # ---- the warm-up's draw -----------------------------------------------------------------------------------------------------
    def sample_uniform_dev(self, num_envs: int, args: "_capi.FleetSacUniformArgs"):
        """Raw device addresses in a FleetSacUniformArgs (include/fleet_hip_sac_loop.h), on the handle's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetSacUniformArgs)
        self._check(self.lib.fleet_saccollect_uniform_dev(self.h, int(num_envs), C.byref(args)))

    def sample_uniform(self, num_envs: int, *, low: float = -1.0, high: float = 1.0, seed: int, step: int, env_id_offset: int = 0,
                       actions_out=None):
        """The warm-up's `action_space.sample()` (SB3: while num_timesteps < learning_starts) without a policy handle: uniform actions
        f32 [num_envs, act_dim] in [low, high), one launch on torch's current stream, no network.  The kernel and the bits are
        `DevicePolicy.sample_uniform`'s under the same (seed, step, env_id_offset + row)."""
        import torch

        self.use_torch_stream()
        E = int(num_envs)
        if actions_out is None:
            actions_out = torch.empty((max(E, 0), self.act_dim), device=torch.device("cuda", self.device), dtype=torch.float32)
        a = _capi.FleetSacUniformArgs()
        a.env_id_offset, a.lo, a.hi = int(env_id_offset), float(low), float(high)
        a.seed, a.step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        a.actions = self._tensor(actions_out, (E, self.act_dim), (torch.float32,)).data_ptr()
        self.sample_uniform_dev(E, a)
        return actions_out

    # ---- the target ----------------------------------------------------------------------------------------------------------
    def soft_target_dev(self, targets, next_obs_ptr: int, rewards_ptr: int, dones_ptr: int, batch: int, args: "_capi.FleetSacTargetArgs"):
        """Raw device addresses in a FleetSacTargetArgs, on the handle's stream; `targets`: the DeviceSACNetworks of the targets.
        (`target_dev` stays the inherited fleet_qtarget_target_dev, which refuses a squashed handle.)"""
        args.struct_bytes = C.sizeof(_capi.FleetSacTargetArgs)
        self._check(self.lib.fleet_sac_target_dev(self.h, getattr(targets, "h", None), next_obs_ptr, rewards_ptr, dones_ptr, int(batch),
                                                  C.byref(args)))

    def target(self, targets, next_obs, rewards, dones, *, gamma: float, ent_coef, seed: int, step: int, row_offset: int = 0, out=None,
               next_actions_out=None, next_log_prob_out=None, q_out=None, noise=None, noise_given: bool = False):
        """SAC's learning targets of a minibatch in one launch, called on the ONLINE networks: `targets` is the DeviceSACNetworks that
        holds the target critics.  next_obs f32 [B, obs_dim] (normalised, as `DeviceReplayBuffer.sample` returns it), rewards f32 [B]
        and dones f32 [B] (or [B, 1]) -> y f32 [B] (`out`, made when None),
        y = rewards + ((1 - dones) * gamma) * (min_c Q'_c(next_obs, a') - alpha * log pi(a' | next_obs)), a' and its log-probability
        what `act` gives on next_obs under (seed, row_offset + row, step).  ent_coef: alpha itself as a device tensor f32 [1], read
        when the launch runs (a float also does, through a cached tensor: one that changes costs a host synchronisation).  Give the
        target a seed of its own, not the acting seed.  next_actions_out f32 [B, act_dim], next_log_prob_out f32 [B] and q_out f32
        [B, n_critics] receive a', its log-probability and the target critics' outputs."""
        import torch

        self.use_torch_stream()
        if isinstance(targets, DeviceTD3Target):
            targets.use_torch_stream()
        f32, A = (torch.float32,), self.act_dim
        B = int(next_obs.shape[0]) if next_obs.ndim == 2 else 0
        next_obs = self._tensor(next_obs, (B, self.obs_dim), f32)
        rewards, dones = self._tensor(rewards, (B,), f32), self._tensor(dones, (B,), f32)
        if out is None:
            out = torch.empty((B,), device=next_obs.device, dtype=torch.float32)
        a = _capi.FleetSacTargetArgs()
        a.noise_mode = _capi.EXPLORE_NOISE_GIVEN if noise_given else _capi.EXPLORE_NOISE_DRAW
        a.seed, a.step, a.row_offset = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), int(row_offset)
        a.gamma = float(gamma)
        if isinstance(ent_coef, torch.Tensor):
            alpha = self._tensor(ent_coef.detach(), (1,), f32)
        else:
            hit = self._constants.get("ent_coef")
            if hit is None or hit[0] != float(ent_coef):
                hit = self._constants["ent_coef"] = (float(ent_coef), torch.full((1,), float(ent_coef), device=next_obs.device, dtype=torch.float32))
            alpha = hit[1]
        a.ent_coef = alpha.data_ptr()
        a.target_q = self._tensor(out, (B,), f32).data_ptr()
        if noise_given and noise is None:
            raise ValueError("noise_given needs the noise tensor")
        keep = [alpha]
        for name, t, shape in (("noise", noise, (B, A)), ("next_actions", next_actions_out, (B, A)), ("next_log_prob", next_log_prob_out, (B,)),
                               ("q", q_out, (B, self.n_critics))):
            if t is not None:
                keep.append(self._tensor(t, shape, f32))
                setattr(a, name, keep[-1].data_ptr())
        self.soft_target_dev(targets, next_obs.data_ptr(), rewards.data_ptr(), dones.data_ptr(), B, a)
        return out

    def describe(self) -> dict:
        """What fleet_qtarget_describe reports (the actor's last width is 2 * act_dim), and `squashed`: True."""
        d = super().describe()
        d["squashed"] = True
        return d


class DeviceSACGrad(DeviceTD3Grad):
    """`DeviceTD3Grad` on a `DeviceSACNetworks` (the ONLINE networks) with SAC's actor entry.  `critic_grad` is inherited unchanged; the
    inherited TD3 `actor_grad` is replaced by the squashed-Gaussian one (the library refuses the TD3 entry on such networks)."""

    def __init__(self, nets, max_batch: int):
        if not isinstance(nets, DeviceSACNetworks):
            raise TypeError("DeviceSACGrad works on a DeviceSACNetworks; a TD3 actor's gradient is DeviceTD3Grad's")
        super().__init__(nets, max_batch)

    def sac_actor_grad_dev(self, args: "_capi.FleetSacActorArgs", grad_ptrs, count: int):
        """Raw device addresses in a FleetSacActorArgs and a (c_void_p * count) array, on the networks handle's stream."""
        args.struct_bytes = C.sizeof(_capi.FleetSacActorArgs)
        self._check(self.lib.fleet_sac_actor_grad_dev(self.h, C.byref(args), grad_ptrs, int(count)))

    def actor_grad(self, obs, *, ent_coef, seed: int, step: int, into, row_offset: int = 0, log_ent_coef=None, target_entropy=None, noise=None,
                   noise_given: bool = False, actions_out=None, log_prob_out=None, q_out=None, dheads_out=None, stats_out=None):
        """SAC's actor loss mean(alpha * log pi(a|obs) - min_c Q_c(obs, a)), a = the squashed sample `DeviceSACNetworks.act` draws under
        (seed, row_offset + row, step), and its gradient in the ACTOR's parameters: two launches on torch's current stream, no host
        synchronisation.  obs f32 [B, obs_dim]; ent_coef: alpha as a device tensor f32 [1], read when the launches run (a float also
        does, through a cached tensor).  into: the actor's torch parameters, W, b per layer -- SB3's `latent_pi`, then the ONE
        `[2A, H]` pair (`parse_sac_state_dict`; `fused_head_parameters` makes it from a torch actor); their `.grad` is overwritten, the
        critics' is not touched.  log_ent_coef: a one-element device leaf tensor -- its `.grad` receives
        -(mean(log pi) + target_entropy) (target_entropy: default -act_dim, SB3's "auto").  noise f32 [B, act_dim]: read with
        noise_given, else it receives the draw.  actions_out [B, act_dim], log_prob_out [B], q_out [B, n_critics], dheads_out
        [B, 2 * act_dim] (the last layer's delta: d mean, then d log_std).  Returns stats f32 [8]: `SAC_ACTOR_STATS`, then zeros."""
        import torch

        self.use_torch_stream()
        f32, A = (torch.float32,), self.act_dim
        B = int(obs.shape[0]) if obs.ndim == 2 else 0
        a = _capi.FleetSacActorArgs()
        a.B, a.row_offset = B, int(row_offset)
        a.noise_mode = _capi.EXPLORE_NOISE_GIVEN if noise_given else _capi.EXPLORE_NOISE_DRAW
        a.seed, a.step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
        a.target_entropy = -float(A) if target_entropy is None else float(target_entropy)
        keep = [self._tensor(obs, (B, self.obs_dim), f32)]
        a.obs = keep[0].data_ptr()
        if isinstance(ent_coef, torch.Tensor):
            alpha = self._tensor(ent_coef.detach(), (1,), f32)
        else:
            hit = self.nets._constants.get("ent_coef")
            if hit is None or hit[0] != float(ent_coef):
                hit = self.nets._constants["ent_coef"] = (float(ent_coef), torch.full((1,), float(ent_coef), device=keep[0].device, dtype=torch.float32))
            alpha = hit[1]
        keep.append(alpha)
        a.ent_coef = alpha.data_ptr()
        if stats_out is None:
            stats_out = torch.empty(8, device=keep[0].device, dtype=torch.float32)
        a.stats = self._tensor(stats_out, (8,), f32).data_ptr()
        if noise_given and noise is None:
            raise ValueError("noise_given needs the noise tensor")
        if log_ent_coef is not None:
            if log_ent_coef.grad is None:
                log_ent_coef.grad = torch.zeros_like(log_ent_coef)
            keep += [self._tensor(log_ent_coef.detach(), (1,), f32), self._tensor(log_ent_coef.grad, (1,), f32)]
            a.log_ent_coef, a.log_ent_coef_grad = keep[-2].data_ptr(), keep[-1].data_ptr()
        for name, t, shape in (("noise", noise, (B, A)), ("actions_out", actions_out, (B, A)), ("log_prob_out", log_prob_out, (B,)),
                               ("q_out", q_out, (B, self.n_critics)), ("dheads_out", dheads_out, (B, 2 * A))):
            if t is not None:
                keep.append(self._tensor(t, shape, f32))
                setattr(a, name, keep[-1].data_ptr())
        arr = self._grad_pointers("actor", into, self._shapes["actor"], "the actor's")
        self.sac_actor_grad_dev(a, arr, len(self._shapes["actor"]))
        return stats_out
