"""stable-baselines3 2.3.2's `PPO.train`, `TD3.train` (DDPG with one critic, delay 1, sigma 0) and the critic half of `SAC.train`, restated
as plain torch on the CPU: `torch.nn.functional`, autograd, `torch.optim.Adam`, `torch.nn.utils.clip_grad_norm_`.  The END-TO-END
reference of the one-call updates (tests/test_update_ref_cpu.py, tests/test_update_ref_gpu.py): it shares no arithmetic with the library
or with the project's bit models -- only WHICH rows form a minibatch is handed in, as integer indices or as gathered minibatches.

Every function is parametrised by `dtype`, so the same code gives ref64 and ref32 (eps_ref = |ref32 - ref64|), and takes
  reverse_rows   every minibatch with its rows in reverse order,
  transposed     every matrix product written (W x^T)^T instead of x W^T,
which together give a second float32 evaluation of the same mathematics with other rounding, and
  mutant         one deliberate misreading of SB3 (MUTANTS), to show that the comparison sees it.
Every function returns, beside the weights, optimiser states and logged means, a KINK LOG: per kind of branch the signed distances
x - threshold of every value that was compared, in the order of evaluation.  `kink_margins` of the float64 and the float32 log gives
per kind the smallest float64 distance and the largest |x32 - x64|: where the first is many times the second, no correct float32
evaluation takes the other branch.
"""
import numpy as np
import torch
import torch.nn.functional as F

F64 = np.float64
MUTANTS = {
    "ppo": ("advantage_over_buffer", "kl_stop_after_step", "vclip_around_new"),
    "td3": ("stale_critic_in_actor_loss", "polyak_every_step", "u_mod_delay"),
    "sac": ("no_half", "next_action_from_target_actor"),
}


# ---- the kink log ----------------------------------------------------------------------------------------------------------------------
class KinkLog:
    def __init__(self):
        self.kinds = {}

    def add(self, kind, x):
        x = x.detach().to(torch.float64).numpy() if isinstance(x, torch.Tensor) else np.asarray(x, F64)
        self.kinds.setdefault(kind, []).append(np.array(x, F64).reshape(-1))


def kink_margins(log64: KinkLog, log32: KinkLog) -> dict:
    """kind -> (the smallest |distance| of the float64 run, the largest |x32 - x64|); the deviation is inf where the two runs did not
    compare the same values (one of them took another branch)."""
    out = {}
    for kind in sorted(set(log64.kinds) | set(log32.kinds)):
        a, b = log64.kinds.get(kind, []), log32.kinds.get(kind, [])
        dist = min((float(np.abs(x).min()) for x in a if x.size), default=np.inf)
        if len(a) != len(b) or any(x.shape != y.shape for x, y in zip(a, b)):
            out[kind] = (dist, np.inf)
        else:
            out[kind] = (dist, max((float(np.abs(x - y).max()) for x, y in zip(a, b) if x.size), default=0.0))
    return out


# ---- shared pieces ---------------------------------------------------------------------------------------------------------------------
def _params(layers, dtype):
    """[(W, b), ...] float32 arrays -> [W, b, ...] leaf tensors of `dtype`."""
    return [torch.from_numpy(np.array(t, np.float32)).to(dtype).requires_grad_(True) for w, b in layers for t in (w, b)]


def _tensor(a, dtype):
    """Data: float64 values (float32 ones widen exactly) rounded once to `dtype`."""
    return torch.from_numpy(np.array(a, F64)).to(dtype)


def _mlp(ps, x, activation, log, transposed):
    n = len(ps) // 2
    for i in range(n):
        w, b = ps[2 * i], ps[2 * i + 1]
        x = (w @ x.t()).t() + b if transposed else F.linear(x, w, b)
        if i < n - 1:
            if activation == "relu":
                log.add("relu", x)
                x = torch.relu(x)
            else:
                x = torch.tanh(x)
    return x


def _adam_state(opt, ps):
    st = [opt.state.get(p, {}) for p in ps]
    z = lambda p: np.zeros(tuple(p.shape), F64)  # noqa: E731  (a parameter that was never stepped has no state yet)
    steps = {int(s["step"]) for s in st if "step" in s}
    assert len(steps) <= 1
    return {"exp_avg": [s["exp_avg"].to(torch.float64).numpy().copy() if "exp_avg" in s else z(p) for s, p in zip(st, ps)],
            "exp_avg_sq": [s["exp_avg_sq"].to(torch.float64).numpy().copy() if "exp_avg_sq" in s else z(p) for s, p in zip(st, ps)],
            "step": steps.pop() if steps else 0}


def _np(ps):
    return [p.detach().to(torch.float64).numpy().copy() for p in ps]


def _grads(ps):
    return [p.grad.detach().to(torch.float64).numpy().copy() for p in ps]


def _polyak(params, targets, tau):
    """SB3's `polyak_update`: target.mul_(1 - tau); torch.add(target, param, alpha=tau, out=target)."""
    with torch.no_grad():
        for p, t in zip(params, targets):
            t.mul_(1 - tau)
            torch.add(t, p, alpha=tau, out=t)


def explained_variance(y_pred, y_true):
    """SB3's `common.utils.explained_variance`, in the dtype of its arguments."""
    var_y = np.var(y_true)
    return np.nan if var_y == 0 else float(1 - np.var(y_true - y_pred) / var_y)


# ---- PPO.train -------------------------------------------------------------------------------------------------------------------------
def ppo_train(actor, critic, log_std, buffer, epochs, *, activation, dtype=torch.float64, clip_range, clip_range_vf=None,
              normalize_advantage=True, ent_coef, vf_coef, lr, adam_eps=1e-5, max_grad_norm, target_kl=None, reverse_rows=False,
              transposed=False, mutant=None, record_grads=False) -> dict:
    """buffer: {"obs" [n, D], "actions" [n, A], "values", "log_prob", "advantages", "returns" [n]} float32, flat; epochs: per epoch
    the list of its minibatches' row indices.  Returns {"params" (the actor's W, b per layer, the critic's, log_std), "exp_avg",
    "exp_avg_sq", "step", "stats", "kinks", "stop" (epoch, minibatch) or None, "per_minibatch_kl", "grads" (per minibatch, unclipped)}."""
    assert mutant in (None, *MUTANTS["ppo"])
    log = KinkLog()
    ps = _params(actor, dtype) + _params(critic, dtype) + [torch.from_numpy(np.array(log_std, np.float32)).to(dtype).requires_grad_(True)]
    na = 2 * len(actor)
    opt = torch.optim.Adam(ps, lr=lr, eps=adam_eps)
    buf = {k: _tensor(v, dtype) for k, v in buffer.items()}
    pg_losses, value_losses, entropy_losses, clip_fractions, all_kl, grads, pg_terms, kl_terms = [], [], [], [], [], [], [], []
    approx_kl_divs, loss, n_updates, stop, continue_training = [], None, 0, None, True
    for e, minibatches in enumerate(epochs):
        approx_kl_divs = []
        for m, idx in enumerate(minibatches):
            idx = torch.from_numpy(np.array(idx[::-1] if reverse_rows else idx, np.int64))
            obs, actions, old_values, old_log_prob, advantages, returns = (buf[k][idx] for k in ("obs", "actions", "values", "log_prob", "advantages", "returns"))
            if normalize_advantage and len(advantages) > 1:
                over = buf["advantages"] if mutant == "advantage_over_buffer" else advantages
                advantages = (advantages - over.mean()) / (over.std() + 1e-8)
            dist = torch.distributions.Normal(_mlp(ps[:na], obs, activation, log, transposed), torch.ones_like(ps[-1]) * ps[-1].exp())
            log_prob, entropy = dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)
            values = _mlp(ps[na:-1], obs, activation, log, transposed).flatten()
            ratio = torch.exp(log_prob - old_log_prob)
            policy_loss_1 = advantages * ratio
            policy_loss_2 = advantages * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)
            policy_loss = -torch.min(policy_loss_1, policy_loss_2).mean()
            log.add("ratio_clip", torch.cat([ratio - (1 - clip_range), ratio - (1 + clip_range)]))
            outside = ((ratio < 1 - clip_range) | (ratio > 1 + clip_range)).detach()
            log.add("surrogates", (policy_loss_1 - policy_loss_2)[outside])
            pg_losses.append(policy_loss.item())
            with torch.no_grad():  # the operands behind the two means of signed terms: one rounding of a log-probability moves a row's
                carried = torch.maximum(torch.abs(log_prob), torch.abs(old_log_prob)).clamp(min=1.0)  # ratio by |log_prob| * 2^-24 of itself
                pg_terms.append(torch.mean(torch.abs(torch.min(policy_loss_1, policy_loss_2)) * carried).item())
                kl_terms.append(torch.mean(torch.abs(ratio - 1) * carried).item())
            clip_fractions.append(torch.mean((torch.abs(ratio - 1) > clip_range).to(dtype)).item())
            if clip_range_vf is None:
                values_pred = values
            elif mutant == "vclip_around_new":
                values_pred = values + torch.clamp(old_values - values, -clip_range_vf, clip_range_vf)
            else:
                values_pred = old_values + torch.clamp(values - old_values, -clip_range_vf, clip_range_vf)
            if clip_range_vf is not None:
                log.add("value_clip", torch.abs(values - old_values) - clip_range_vf)
            value_loss = F.mse_loss(returns, values_pred)
            value_losses.append(value_loss.item())
            entropy_loss = -torch.mean(entropy)
            entropy_losses.append(entropy_loss.item())
            loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
            with torch.no_grad():
                log_ratio = log_prob - old_log_prob
                approx_kl_div = torch.mean((torch.exp(log_ratio) - 1) - log_ratio).cpu().numpy()
                approx_kl_divs.append(approx_kl_div)
                all_kl.append(float(approx_kl_div))
            stopping = target_kl is not None and approx_kl_div > 1.5 * target_kl
            if target_kl is not None:
                log.add("target_kl", float(approx_kl_div) - 1.5 * target_kl)
            if stopping and mutant != "kl_stop_after_step":
                continue_training, stop = False, (e, m)
                break
            opt.zero_grad()
            loss.backward()
            if record_grads:
                grads.append(_grads(ps))
            log.add("grad_norm", torch.nn.utils.clip_grad_norm_(ps, max_grad_norm) - max_grad_norm)
            opt.step()
            if stopping:
                continue_training, stop = False, (e, m)
                break
        n_updates += 1
        if not continue_training:
            break
    y, v = (buf[k].numpy() for k in ("returns", "values"))
    stats = {"policy_gradient_loss": np.mean(pg_losses), "value_loss": np.mean(value_losses), "entropy_loss": np.mean(entropy_losses),
             "approx_kl": float(np.mean(approx_kl_divs)),  # SB3 clears the list every epoch: the last epoch entered
             "approx_kl_all_epochs": float(np.mean(all_kl)), "clip_fraction": np.mean(clip_fractions), "loss": loss.item(),
             "n_updates": n_updates, "minibatches": len(all_kl), "explained_variance": explained_variance(v, y),
             "std": torch.exp(ps[-1]).mean().item(), "last_approx_kl": all_kl[-1]}
    last = len(approx_kl_divs)
    terms = {"policy_gradient_loss": np.mean(pg_terms), "approx_kl_all_epochs": np.mean(kl_terms), "approx_kl": np.mean(kl_terms[-last:]),
             "last_approx_kl": kl_terms[-1]}
    return {"params": _np(ps), **_adam_state(opt, ps), "stats": {k: float(x) for k, x in stats.items()}, "kinks": log, "stop": stop,
            "per_minibatch_kl": all_kl, "grads": grads, "terms": {k: float(x) for k, x in terms.items()}}


# ---- TD3.train -------------------------------------------------------------------------------------------------------------------------
def _batch(b, dtype, reverse_rows):
    """(obs, actions, next_obs, dones, rewards), the last two [B] or [B, 1] -> tensors of `dtype`, dones and rewards [B, 1]."""
    out = [_tensor(x, dtype) for x in b]
    out[3], out[4] = out[3].reshape(-1, 1), out[4].reshape(-1, 1)
    return [x.flip(0) for x in out] if reverse_rows else out


def normalised(x, mean, var, epsilon, clip) -> np.ndarray:
    """SB3 VecNormalize's `(x - mean) / sqrt(var + epsilon)`, clipped, in float64 from the exported statistics (mean 0 for rewards)."""
    return np.clip((np.asarray(x, F64) - mean) / np.sqrt(np.asarray(var, F64) + epsilon), -clip, clip)


def td3_train(actor, critics, target_actor, target_critics, batches, noise, *, activation, dtype=torch.float64, gamma, tau, policy_delay,
              sigma, noise_clip, lr, adam_eps=1e-8, first_update=0, reverse_rows=False, transposed=False, mutant=None,
              record_grads=False) -> dict:
    """batches: per gradient step (obs, actions, next_obs, dones, rewards) as `replay_buffer.sample` returns them (normalised where a
    normaliser is in use); noise: per step the standard-normal draw [B, A] that SB3 takes from `normal_(0, 1) * target_policy_noise`;
    sigma: target_policy_noise, a float or [A].  The actors end in tanh; actions lie in [-1, 1].  Returns {"actor", "critics" (flat: W, b
    per layer, critic 0 then 1), "target_actor", "target_critics", "actor_opt", "critic_opt", "stats", "kinks", "grads"}."""
    assert mutant in (None, *MUTANTS["td3"])
    log = KinkLog()
    pa, ta = _params(actor, dtype), _params(target_actor, dtype)
    pc, tc = [_params(c, dtype) for c in critics], [_params(c, dtype) for c in target_critics]
    flat = lambda nets: [p for net in nets for p in net]  # noqa: E731
    opt_a, opt_c = torch.optim.Adam(pa, lr=lr, eps=adam_eps), torch.optim.Adam(flat(pc), lr=lr, eps=adam_eps)
    sig = torch.from_numpy(np.broadcast_to(np.asarray(sigma, F64), (actor[-1][0].shape[0],)).copy()).to(dtype)
    pi = lambda ps, x: torch.tanh(_mlp(ps, x, activation, log, transposed))  # noqa: E731
    q = lambda ps, x, a: _mlp(ps, torch.cat([x, a], dim=1), activation, log, transposed)  # noqa: E731
    n_updates, actor_losses, critic_losses, each_losses, grads, q_terms = first_update, [], [], [], [], []
    for b, eps in zip(batches, noise):
        n_updates += 1
        obs, actions, next_obs, dones, rewards = _batch(b, dtype, reverse_rows)
        eps = _tensor(eps, dtype).flip(0) if reverse_rows else _tensor(eps, dtype)
        with torch.no_grad():
            n = eps * sig
            log.add("noise_clip", torch.cat([n + noise_clip, n - noise_clip]))
            n = n.clamp(-noise_clip, noise_clip)
            raw = pi(ta, next_obs) + n
            log.add("action_bounds", torch.cat([raw + 1, raw - 1]))
            next_actions = raw.clamp(-1, 1)
            next_q_values = torch.cat([q(t, next_obs, next_actions) for t in tc], dim=1)
            if len(tc) == 2:
                log.add("q_min", next_q_values[:, 0] - next_q_values[:, 1])
            next_q_values, _ = torch.min(next_q_values, dim=1, keepdim=True)
            target_q_values = rewards + (1 - dones) * gamma * next_q_values
        stale = [p.detach().clone() for p in pc[0]]
        each = [F.mse_loss(q(c, obs, actions), target_q_values) for c in pc]
        critic_loss = sum(each)
        critic_losses.append(critic_loss.item())
        each_losses.append([x.item() for x in each])
        opt_c.zero_grad()
        critic_loss.backward()
        step_grads = {"critic": _grads(flat(pc)), "target_q": target_q_values.to(torch.float64).numpy().reshape(-1).copy()}
        opt_c.step()
        due = (n_updates - 1 if mutant == "u_mod_delay" else n_updates) % policy_delay == 0
        if due:
            q1 = stale if mutant == "stale_critic_in_actor_loss" else pc[0]
            q_pi = q(q1, obs, pi(pa, obs))
            actor_loss = -q_pi.mean()
            actor_losses.append(actor_loss.item())
            q_terms.append(q_pi.detach().abs().mean().item())  # the operands of this mean of signed terms
            opt_a.zero_grad()
            actor_loss.backward()
            step_grads["actor"] = _grads(pa)
            opt_a.step()
        if due or mutant == "polyak_every_step":
            _polyak(flat(pc), flat(tc), tau)
            _polyak(pa, ta, tau)
        if record_grads:
            grads.append(step_grads)
    each_losses = np.asarray(each_losses, F64)
    stats = {"critic_loss": np.mean(critic_losses), "critic_0_loss": each_losses[:, 0].mean(),
             "critic_1_loss": each_losses[:, 1].mean() if len(pc) == 2 else 0.0,
             "actor_loss": np.mean(actor_losses) if actor_losses else np.nan, "last_critic_loss": critic_losses[-1],
             "last_actor_loss": actor_losses[-1] if actor_losses else np.nan, "n_updates": n_updates, "actor_steps": len(actor_losses)}
    return {"actor": _np(pa), "critics": _np(flat(pc)), "target_actor": _np(ta), "target_critics": _np(flat(tc)),
            "actor_opt": _adam_state(opt_a, pa), "critic_opt": _adam_state(opt_c, flat(pc)), "stats": {k: float(x) for k, x in stats.items()},
            "kinks": log, "grads": grads,
            "terms": {"actor_loss": float(np.mean(q_terms)), "last_actor_loss": q_terms[-1]} if q_terms else {}}


# ---- the critic half of SAC.train ----------------------------------------------------------------------------------------------------
LOG_STD_MIN, LOG_STD_MAX = -20, 2


def sac_critic_steps(actor, critics, target_actor, target_critics, batches, noise, *, activation, dtype=torch.float64, gamma, tau,
                     ent_coef, lr, adam_eps=1e-8, reverse_rows=False, transposed=False, mutant=None) -> dict:
    """actor: its last layer [2A, H], the mu rows then the log_std rows (SB3's two heads on one latent).  Per step: the target from the
    ONLINE actor on next_obs (`actor.action_log_prob`), the critic loss 0.5 * sum_c mse, Adam on the critics, Polyak of the target
    critics.  target_actor: the copy of the actor a target handle carries; SB3 has none and nothing may read it, it only follows by
    Polyak.  The actor itself takes no step here.  Returns {"critics", "target_actor", "target_critics", "critic_opt", "stats", "kinks"}."""
    assert mutant in (None, *MUTANTS["sac"])
    log = KinkLog()
    pa, ta = _params(actor, dtype), _params(target_actor, dtype)
    pc, tc = [_params(c, dtype) for c in critics], [_params(c, dtype) for c in target_critics]
    flat = lambda nets: [p for net in nets for p in net]  # noqa: E731
    opt_c = torch.optim.Adam(flat(pc), lr=lr, eps=adam_eps)
    A = actor[-1][0].shape[0] // 2
    q = lambda ps, x, a: _mlp(ps, torch.cat([x, a], dim=1), activation, log, transposed)  # noqa: E731
    critic_losses = []
    for b, eps in zip(batches, noise):
        obs, actions, next_obs, dones, rewards = _batch(b, dtype, reverse_rows)
        eps = _tensor(eps, dtype).flip(0) if reverse_rows else _tensor(eps, dtype)
        with torch.no_grad():
            out = _mlp(ta if mutant == "next_action_from_target_actor" else pa, next_obs, activation, log, transposed)
            mean_actions, log_std = out[:, :A], out[:, A:]
            log.add("log_std_clamp", torch.cat([log_std - LOG_STD_MIN, log_std - LOG_STD_MAX]))
            log_std = torch.clamp(log_std, LOG_STD_MIN, LOG_STD_MAX)
            dist = torch.distributions.Normal(mean_actions, torch.exp(log_std))
            gaussian_actions = mean_actions + torch.exp(log_std) * eps  # rsample() with the given draw
            next_actions = torch.tanh(gaussian_actions)
            next_log_prob = dist.log_prob(gaussian_actions).sum(dim=1) - torch.sum(torch.log(1 - next_actions ** 2 + 1e-6), dim=1)
            next_q_values = torch.cat([q(t, next_obs, next_actions) for t in tc], dim=1)
            if len(tc) == 2:
                log.add("q_min", next_q_values[:, 0] - next_q_values[:, 1])
            next_q_values, _ = torch.min(next_q_values, dim=1, keepdim=True)
            next_q_values = next_q_values - ent_coef * next_log_prob.reshape(-1, 1)
            target_q_values = rewards + (1 - dones) * gamma * next_q_values
        critic_loss = (1.0 if mutant == "no_half" else 0.5) * sum(F.mse_loss(q(c, obs, actions), target_q_values) for c in pc)
        critic_losses.append(critic_loss.item())
        opt_c.zero_grad()
        critic_loss.backward()
        opt_c.step()
        _polyak(flat(pc), flat(tc), tau)
        _polyak(pa, ta, tau)
    stats = {"critic_loss": np.mean(critic_losses), "last_critic_loss": critic_losses[-1], "n_updates": len(critic_losses)}
    return {"critics": _np(flat(pc)), "target_actor": _np(ta), "target_critics": _np(flat(tc)), "critic_opt": _adam_state(opt_c, flat(pc)),
            "stats": {k: float(x) for k, x in stats.items()}, "kinks": log, "terms": {}}
