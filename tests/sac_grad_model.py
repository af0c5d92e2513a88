"""SAC's actor and entropy-coefficient gradients (include/fleet_hip.h "SAC actor and entropy-coefficient gradients on the device") restated
for the tests, three times over.  Nothing here needs a GPU or the library.

What stable-baselines3 2.3.2's `SAC.train` computes in one gradient step:
    actions_pi, log_prob = actor.action_log_prob(obs)          # rsample: u = m + exp(ls) * eps, a = tanh(u)
    ent_coef_loss = -(log_ent_coef * (log_prob + target_entropy).detach()).mean()
    min_qf_pi = min_c critic_c(obs, actions_pi)                # the critics AFTER their optimiser step
    actor_loss = (ent_coef * log_prob - min_qf_pi).mean()      # gradient into the actor only

1. `model64`: the ANALYTIC gradient in NumPy float64, the forward from `sac_model`.  Per row, alpha = ent_coef, k the critic that attains
   the minimum (critic 0 on q_0 <= q_1: `torch.min(dim=1)` returns the first of equal values, and no judged case is near a tie),
   w_j = 1 - a_j^2:
       dL/da_j = -(1/B) dQ_k/da_j + (alpha/B) (2 a_j) / (w_j + 1e-6)
       dL/du_j = dL/da_j w_j;   dL/dm_j = dL/du_j
       dL/dl_j = (dL/du_j exp(ls_j) eps_j - alpha/B) [-20 <= l_j <= 2]     (torch's clamp backward: the bounds INCLUSIVE, a value
                 exactly at a bound passes its gradient; outside them the gradient is zero)
       d ent_coef_loss / d log_ent_coef = -(mean_b(log_prob_b) + target_entropy)
   Under the reparametrisation the Gaussian term of log_prob does not depend on m and depends on ls only through -ls.
2. `autograd`: a second reading that shares no arithmetic with the first -- plain torch on the CPU: `Normal(mean, std).log_prob` of the
   rsample-style u, tanh, SB3's correction, `torch.min(..., dim=1)`, `.mean().backward()` -- parametrised by dtype in the style of
   tests/sb3_update_ref.py: float64 checks the analytic model, float32 gives eps_ref.  `mutant` misreads SB3 on purpose (MUTANTS).
3. `dheads32`: the header's float32 order of the head deltas from STORED values (a, eps, the clamped log_std, da), operation by
   operation, and `da_one_layer32`, the critic's da where it can be restated exactly (critics of one layer).

Then the case table of tests/test_sac_grad_gpu.py and the conditions every judged case meets (`conditions`).
"""
import functools
import zlib

import numpy as np

import policy_bits as pb
import policy_model as pm
import sac_model as sm
import sb3_update_ref as ur
import td3_model as tm

ROOT = pm.ROOT
F32, F64 = np.float32, np.float64
SAC_ACTOR_STATS = ("actor_loss", "ent_coef_loss", "log_prob_mean", "qmin_mean", "ent_coef")
MUTANTS = ("critic0_only", "no_clamp_mask", "no_alpha_in_dl", "no_target_entropy")
KINK_FACTOR = 16.0  # a kink's smallest float64 distance over the largest float32-vs-float64 deviation, at least
W_FLOOR = 2.0 ** -10  # bound-judged cases keep 1 - a^2 above this


# ---- 1. the analytic model, float64 ------------------------------------------------------------------------------------------------
def model64(actor, critics, activation, obs, eps, alpha, log_ent_coef=None, target_entropy=None) -> dict:
    """{"grads": [dW, db per layer of the actor, the last pair [2A, H] / [2A]], "log_ent_coef_grad", "stats": {name: value},
    "dheads" [B, 2A], "da" [B, A], "actions", "log_prob", "q" [B, n_critics], "k" [B], "l" (unclamped), "log_std", "w", "pre": {"actor":
    [...], "critics": [...]} the hidden pre-activations, "terms": the signed terms of the two means}."""
    obs, eps = np.asarray(obs, F64), np.asarray(eps, F64)
    B, D = obs.shape
    A = np.asarray(actor[-1][0]).shape[0] // 2
    alpha = float(alpha)
    te = -float(A) if target_entropy is None else float(target_entropy)
    xa, pre_a, y = tm._forward(actor, obs, activation)
    m, l = y[:, :A], y[:, A:]
    f = sm.act64(m, l, eps)
    ls, a, lp = f["log_std"], f["actions"], f["log_prob"]
    x = np.concatenate([obs, a], axis=1)
    fw = [tm._forward(c, x, activation) for c in critics]
    q = np.stack([o[2][:, 0] for o in fw], 1)
    k = np.zeros(B, np.int64) if len(critics) == 1 else np.where(q[:, 0] <= q[:, 1], 0, 1)
    qmin = q[np.arange(B), k]
    da = np.zeros((B, A))
    for c, (layers, (xc, _, _)) in enumerate(zip(critics, fw)):
        _, dx = tm._backward(layers, xc, np.where(k == c, -1.0 / B, 0.0)[:, None], activation)
        da += dx[:, D:]
    w = 1.0 - a * a
    dla = da + (alpha / B) * (2.0 * a) / (w + sm.EPSILON)
    du = dla * w
    mask = ((l >= sm.LOG_STD_MIN) & (l <= sm.LOG_STD_MAX)).astype(F64)
    dl = (du * np.exp(ls) * eps - alpha / B) * mask
    dheads = np.concatenate([du, dl], 1)
    grads, _ = tm._backward(actor, xa, dheads, activation)
    term = alpha * lp - qmin
    gl = -(lp.mean() + te)
    stats = {"actor_loss": float(term.mean()), "ent_coef_loss": 0.0 if log_ent_coef is None else float(log_ent_coef) * gl,
             "log_prob_mean": float(lp.mean()), "qmin_mean": float(qmin.mean()), "ent_coef": alpha}
    return {"grads": grads, "log_ent_coef_grad": gl, "stats": stats, "dheads": dheads, "da": da, "actions": a, "log_prob": lp, "q": q, "k": k,
            "l": l, "log_std": ls, "w": w, "pre": {"actor": pre_a, "critics": [p for o in fw for p in o[1]]},
            "terms": {"actor_loss": term, "entropy": lp + te}}


# ---- 2. SB3's expressions under torch autograd -------------------------------------------------------------------------------------
def autograd(actor, critics, activation, obs, eps, alpha, log_ent_coef=None, target_entropy=None, dtype="float64", mutant=None) -> dict:
    """SB3's own lines in `dtype` on the CPU: {"grads", "log_ent_coef_grad", "stats", "q", "l", "actions", "log_prob", "dheads", "kinks"}."""
    import torch

    assert mutant in (None, *MUTANTS)
    dt = getattr(torch, dtype)
    log = ur.KinkLog()
    pa, pc = ur._params(actor, dt), [ur._params(c, dt) for c in critics]
    x, e = ur._tensor(obs, dt), ur._tensor(eps, dt)
    A = np.asarray(actor[-1][0]).shape[0] // 2
    te = -float(A) if target_entropy is None else float(target_entropy)
    out = ur._mlp(pa, x, activation, log, False)
    out.retain_grad()  # the heads' deltas: d actor_loss / d (mean, unclamped log_std)
    mean_actions, raw = out[:, :A], out[:, A:]
    log.add("log_std_clamp", torch.cat([raw - ur.LOG_STD_MIN, raw - ur.LOG_STD_MAX]))
    log_std = torch.clamp(raw, ur.LOG_STD_MIN, ur.LOG_STD_MAX)
    if mutant == "no_clamp_mask":  # the clamped value, the gradient of the identity
        log_std = raw + (log_std - raw).detach()
    std = torch.exp(log_std)
    gaussian_actions = mean_actions + std * e  # Normal.rsample() with the given draw
    actions_pi = torch.tanh(gaussian_actions)
    log_prob = torch.distributions.Normal(mean_actions, std).log_prob(gaussian_actions).sum(dim=1)
    log_prob = log_prob - torch.sum(torch.log(1 - actions_pi ** 2 + 1e-6), dim=1)
    if mutant == "no_alpha_in_dl":  # the same value; the Gaussian term's -log_std no longer reaches the actor
        log_prob = log_prob + (log_std - log_std.detach()).sum(dim=1)
    log_prob = log_prob.reshape(-1, 1)
    gl, ent_loss = None, 0.0
    if log_ent_coef is not None:
        lec = torch.tensor([float(log_ent_coef)], dtype=dt, requires_grad=True)
        shift = 0.0 if mutant == "no_target_entropy" else te
        ent_coef_loss = -(lec * (log_prob + shift).detach()).mean()
        ent_coef_loss.backward()
        gl, ent_loss = float(lec.grad[0]), ent_coef_loss.item()
    q_values_pi = torch.cat([ur._mlp(ps, torch.cat([x, actions_pi], dim=1), activation, log, False) for ps in pc], dim=1)
    if len(pc) == 2:
        log.add("q_min", q_values_pi[:, 0] - q_values_pi[:, 1])
    if mutant == "critic0_only":
        min_qf_pi = q_values_pi[:, :1]
    else:
        min_qf_pi, _ = torch.min(q_values_pi, dim=1, keepdim=True)
    actor_loss = (float(alpha) * log_prob - min_qf_pi).mean()
    actor_loss.backward()
    stats = {"actor_loss": actor_loss.item(), "ent_coef_loss": ent_loss, "log_prob_mean": log_prob.mean().item(),
             "qmin_mean": min_qf_pi.mean().item(), "ent_coef": float(alpha)}
    n64 = lambda t: t.detach().to(torch.float64).numpy().copy()  # noqa: E731
    return {"grads": ur._grads(pa), "log_ent_coef_grad": gl, "stats": stats, "q": n64(q_values_pi), "l": n64(raw), "actions": n64(actions_pi),
            "log_prob": n64(log_prob).reshape(-1), "dheads": n64(out.grad), "kinks": log}


def sac_gradient_steps(actor, critics, target_actor, target_critics, batches, noise, target_noise, *, activation, dtype="float64", gamma, tau,
                       lr, log_ent_coef=None, ent_coef=None, target_entropy=None, adam_eps=1e-8) -> dict:
    """SB3's whole `SAC.train` loop under autograd and `torch.optim.Adam`, one gradient step per batch: alpha = exp(log_ent_coef) read
    before its step (or the fixed `ent_coef`), the entropy-coefficient step, the critic step on the soft target (drawn with
    target_noise), the actor step (drawn with noise) on the critics just stepped, the Polyak update (the target handle's copy of the
    actor follows too, and nothing reads it).  batches: (obs, actions, next_obs, dones, rewards) per step."""
    import torch
    import torch.nn.functional as F

    dt = getattr(torch, dtype)
    log = ur.KinkLog()
    pa, ta = ur._params(actor, dt), ur._params(target_actor, dt)
    pc, tc = [ur._params(c, dt) for c in critics], [ur._params(c, dt) for c in target_critics]
    flat = lambda nets: [p for net in nets for p in net]  # noqa: E731
    opt_a, opt_c = torch.optim.Adam(pa, lr=lr, eps=adam_eps), torch.optim.Adam(flat(pc), lr=lr, eps=adam_eps)
    A = np.asarray(actor[-1][0]).shape[0] // 2
    te = -float(A) if target_entropy is None else float(target_entropy)
    lec, opt_e = None, None
    if log_ent_coef is not None:
        lec = torch.tensor([float(log_ent_coef)], dtype=dt, requires_grad=True)
        opt_e = torch.optim.Adam([lec], lr=lr, eps=adam_eps)
    qf = lambda ps, x, a: ur._mlp(ps, torch.cat([x, a], dim=1), activation, log, False)  # noqa: E731

    def action_log_prob(x, e):
        out = ur._mlp(pa, x, activation, log, False)
        mean_actions, raw = out[:, :A], out[:, A:]
        log.add("log_std_clamp", torch.cat([raw - ur.LOG_STD_MIN, raw - ur.LOG_STD_MAX]))
        std = torch.exp(torch.clamp(raw, ur.LOG_STD_MIN, ur.LOG_STD_MAX))
        u = mean_actions + std * e
        a = torch.tanh(u)
        return a, torch.distributions.Normal(mean_actions, std).log_prob(u).sum(dim=1) - torch.sum(torch.log(1 - a ** 2 + 1e-6), dim=1)

    alphas, actor_losses, critic_losses = [], [], []
    for b, e_pi, e_t in zip(batches, noise, target_noise):
        obs, actions, next_obs, dones, rewards = ur._batch(b, dt, False)
        actions_pi, log_prob = action_log_prob(obs, ur._tensor(e_pi, dt))
        log_prob = log_prob.reshape(-1, 1)
        if lec is not None:
            alpha = torch.exp(lec.detach())
            ent_coef_loss = -(lec * (log_prob + te).detach()).mean()
            opt_e.zero_grad()
            ent_coef_loss.backward()
            opt_e.step()
        else:
            alpha = torch.tensor([float(ent_coef)], dtype=torch.float32).to(dt)  # the device keeps alpha in float32
        alphas.append(float(alpha))
        with torch.no_grad():
            next_actions, next_log_prob = action_log_prob(next_obs, ur._tensor(e_t, dt))
            next_q = torch.cat([qf(t, next_obs, next_actions) for t in tc], dim=1)
            if len(tc) == 2:
                log.add("q_min", next_q[:, 0] - next_q[:, 1])
            next_q, _ = torch.min(next_q, dim=1, keepdim=True)
            next_q = next_q - alpha * next_log_prob.reshape(-1, 1)
            target_q = rewards + (1 - dones) * gamma * next_q
        critic_loss = 0.5 * sum(F.mse_loss(qf(c, obs, actions), target_q) for c in pc)
        critic_losses.append(critic_loss.item())
        opt_c.zero_grad()
        critic_loss.backward()
        opt_c.step()
        q_pi = torch.cat([qf(c, obs, actions_pi) for c in pc], dim=1)
        if len(pc) == 2:
            log.add("q_min", q_pi[:, 0] - q_pi[:, 1])
        min_qf_pi, _ = torch.min(q_pi, dim=1, keepdim=True)
        actor_loss = (alpha * log_prob - min_qf_pi).mean()
        actor_losses.append(actor_loss.item())
        opt_a.zero_grad()
        actor_loss.backward()
        opt_a.step()
        ur._polyak(flat(pc), flat(tc), tau)
        ur._polyak(pa, ta, tau)
    out = {"actor": ur._np(pa), "critics": ur._np(flat(pc)), "target_actor": ur._np(ta), "target_critics": ur._np(flat(tc)),
           "actor_opt": ur._adam_state(opt_a, pa), "critic_opt": ur._adam_state(opt_c, flat(pc)), "kinks": log,
           "stats": {"alphas": alphas, "actor_losses": actor_losses, "critic_losses": critic_losses}}
    if lec is not None:
        out["log_ent_coef"], out["ent_opt"] = ur._np([lec]), ur._adam_state(opt_e, [lec])
    return out


# ---- 3. the header's float32 order ---------------------------------------------------------------------------------------------------
def dheads32(actions, eps, log_std, da, alpha, B) -> np.ndarray:
    """[B, 2A] float32: dm, then dl, from the device's stored a, eps, clamped log_std and the critics' da, every operation rounded on
    its own in the header's order.  The mask is read off the clamped value: a column at a bound is a clamped one (condition (a) keeps
    the unclamped l of every judged column away from the bounds)."""
    a, e, ls, da = (np.asarray(v, F32) for v in (actions, eps, log_std, da))
    invB = F32(1.0) / F32(B)
    ab = F32(alpha) * invB
    w = (F32(1.0) - (a * a).astype(F32)).astype(F32)
    g = ((F32(2.0) * a).astype(F32) / (w + F32(1e-6)).astype(F32)).astype(F32)
    dla = (da + (ab * g).astype(F32)).astype(F32)
    du = (dla * w).astype(F32)
    sdb = np.exp(ls.astype(F64)).astype(F32)  # (float)exp((double)ls)
    se = (sdb * e).astype(F32)
    dl = ((du * se).astype(F32) - ab).astype(F32)
    dl = np.where((ls > F32(-20.0)) & (ls < F32(2.0)), dl, F32(0.0)).astype(F32)
    return np.concatenate([du, dl], 1)


def da_one_layer32(critics, D, k, B) -> np.ndarray:
    """da [B, A] float32 of critics WITHOUT a hidden layer: da_c[j] = fmaf(W_c[0][D + j], dq_c, 0), dq_c = -invB in the rows critic c won
    and 0 elsewhere; da = da_0 (+ da_1)."""
    invB = F32(1.0) / F32(B)
    da = None
    for c, layers in enumerate(critics):
        assert len(layers) == 1
        wa = np.asarray(layers[0][0], F32)[0, D:]
        dq = np.where(np.asarray(k) == c, -invB, F32(0.0)).astype(F32)[:, None]
        d = (wa[None, :] * dq).astype(F32)
        da = d if da is None else (da + d).astype(F32)
    return da


def chain_dW32(dheads, x) -> tuple:
    """(dW [out, in], db [out]) float32 of a ONE-layer actor: dW[j][k] = fmaf(d[b][j], x[b][k], acc), db[j] += d[b][j], b ascending."""
    d, x = np.asarray(dheads, F32), np.asarray(x, F32)
    dW, db = np.zeros((d.shape[1], x.shape[1]), F32), np.zeros(d.shape[1], F32)
    for b in range(d.shape[0]):
        dW = pb.fma32(d[b][:, None], x[b][None, :], dW)
        db = (db + d[b]).astype(F32)
    return dW, db


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
def bound(ref64, ref32) -> float:
    """The project's bound of one tensor (DESIGN.md sections 7n, 7v): 8 * max(eps_ref, 2^-24 * max|ref|), eps_ref the float32 second
    reading's distance to float64."""
    r64, r32 = np.asarray(ref64, F64), np.asarray(ref32, F64)
    return 8.0 * max(float(np.abs(r32 - r64).max()), 2.0 ** -24 * float(np.abs(r64).max()))


def ratio(got, ref64, ref32) -> float:
    """worst error / bound of one tensor (<= 1 passes); 0 where both are exactly zero."""
    err = float(np.abs(np.asarray(got, F64) - np.asarray(ref64, F64)).max())
    b = bound(ref64, ref32)
    return 0.0 if err == 0.0 else (np.inf if b == 0.0 else err / b)


def class_ratios(got, m64, r32, learned) -> dict:
    """tensor class -> the worst ratio: got / m64 / r32 are dicts with "grads", "stats" (name -> value) and "log_ent_coef_grad"."""
    out = {"actor_grads": max(ratio(g, a, b) for g, a, b in zip(got["grads"], m64["grads"], r32["grads"])),
           "stats": max(ratio(got["stats"][n], m64["stats"][n], r32["stats"][n]) for n in SAC_ACTOR_STATS
                        if learned or n != "ent_coef_loss")}
    if learned:
        out["log_ent_coef_grad"] = ratio(got["log_ent_coef_grad"], m64["log_ent_coef_grad"], r32["log_ent_coef_grad"])
    return out


# ---- the cases of tests/test_sac_grad_gpu.py ----------------------------------------------------------------------------------------
# The smallest shapes at which the kernel can still go wrong: B around the 16-row tile (1, 16, 17, 33: one row, a full tile, a ragged
# second tile, two tiles and a row), A in {1, 3, 5, 65} (the 4-column Philox block; 2A crossing 128 and A64 crossing 64), D in {7, 131}
# (below the 128-column chunk; the seam inside a critic's first chunk at 7, behind it at 131), trunks without a hidden layer, within
# one column group, with padding both ways and with two column groups; one and two critics; both activations; alpha learned and
# fixed; the noise given and drawn.
# name: D, A, hidden widths (actor and critics), activation, n_critics, B, learned alpha, noise given, log_std bias (None: as initialised);
# eps_scale: the given noise times this per column (a column clamped at log_std = 2 has a standard deviation of 7.4: condition (b)
# needs a small draw there)
CASES = {
    "7x1-one-layer-twin": dict(D=7, A=1, hidden=(), activation="tanh", n_critics=2, B=17, learned=True, given=True, bias=None),
    "7x3-one-layer-single": dict(D=7, A=3, hidden=(), activation="tanh", n_critics=1, B=1, learned=False, given=False, bias=None),
    "7x5-8-8-relu-twin": dict(D=7, A=5, hidden=(8, 8), activation="relu", n_critics=2, B=33, learned=True, given=False, bias=None),
    "7x5-8-8-tanh-clamped": dict(D=7, A=5, hidden=(8, 8), activation="tanh", n_critics=2, B=33, learned=True, given=True,
                                 bias=(-23.0, 4.0, -0.5, 3.5, -0.25), eps_scale=(1.0, 0.125, 1.0, 0.125, 1.0)),
    "131x65-65-63-relu-twin": dict(D=131, A=65, hidden=(65, 63), activation="relu", n_critics=2, B=17, learned=False, given=True, bias=-1.0),
    "131x65-130-70-tanh-single": dict(D=131, A=65, hidden=(130, 70), activation="tanh", n_critics=1, B=16, learned=True, given=True, bias=-1.0),
    "131x3-130-70-relu-twin": dict(D=131, A=3, hidden=(130, 70), activation="relu", n_critics=2, B=33, learned=False, given=False, bias=None),
}
BOTH_WIN = "7x5-8-8-relu-twin"  # condition (d) is asked of this case
CLAMPED = "7x5-8-8-tanh-clamped"  # condition (e)
SATURATED = dict(D=7, A=3, hidden=(), activation="tanh", n_critics=2, B=17, learned=True, given=True, bias=None)  # bits only
ONE_LAYER = ("7x1-one-layer-twin", "7x3-one-layer-single")  # da has an exact float32 restatement
MAX_SALT = 16
ALPHA, LOG_ALPHA = 0.2, float(np.log(np.float32(0.2)))


def seed(name, salt) -> int:
    return zlib.crc32(f"sac-grad/{name}/{salt}".encode())


def make(name, salt, spec=None) -> dict:
    """The networks and inputs of a case under `salt`: torch's default initialisation, observations N(0, 1) clipped to +-3, eps a
    standard-normal stand-in clipped to +-2.5 (the given noise; a drawn case is judged on the device's own draw)."""
    s = dict(CASES[name] if spec is None else spec)
    D, A, hidden, nc = s["D"], s["A"], tuple(s["hidden"]), s["n_critics"]
    rng = np.random.default_rng(seed(name, salt))
    actor = pm.random_layers(rng, (D, *hidden, 2 * A))
    if s["bias"] is not None:
        w, b = actor[-1]
        b = b.copy()
        b[A:] = np.broadcast_to(np.asarray(s["bias"], F32), (A,))
        actor[-1] = (w, b)
    critics = [pm.random_layers(rng, (D + A, *hidden, 1)) for _ in range(nc)]
    B = s["B"]
    obs = np.clip(rng.standard_normal((B, D)), -3, 3).astype(F32)
    eps = np.clip(rng.standard_normal((B, A)), -2.5, 2.5).astype(F32)
    if s.get("eps_scale") is not None:
        eps = (eps * np.asarray(s["eps_scale"], F32)).astype(F32)
    s.update(name=name, salt=salt, actor=actor, critics=critics, obs=obs, eps=eps, alpha=float(F32(ALPHA)),
             log_ent_coef=float(F32(LOG_ALPHA)) if s["learned"] else None, target_entropy=-float(A))
    return s


def saturated_case() -> dict:
    """One-layer networks whose mu bias throws every u past +-12: 1 - a^2 == 0 in float32 in every column."""
    c = make("saturated", 0, SATURATED)
    w, b = c["actor"][-1]
    b = b.copy()
    b[:c["A"]] = np.array([30.0, -30.0, 25.0], F32)
    c["actor"][-1] = (w, b)
    return c


def args_of(c, eps=None) -> tuple:
    return c["actor"], c["critics"], c["activation"], c["obs"], c["eps"] if eps is None else eps, c["alpha"], c["log_ent_coef"], c["target_entropy"]


def conditions(c, eps=None, q_dev=None) -> dict:
    """The conditions of a judged case from the float64 model (and the float32 second reading for the deviations): name -> bool.
    eps: the draw that is judged (default: the case's own); q_dev [B, n_critics]: the device's critic outputs, whose deviation from
    float64 then also counts against the q_0 / q_1 kink."""
    m = model64(*args_of(c, eps))
    r64, r32 = autograd(*args_of(c, eps), dtype="float64"), autograd(*args_of(c, eps), dtype="float32")
    f = {}
    # (a) per kind of kink: the smallest float64 distance >= 16 x the largest float32-vs-float64 deviation
    for kind, (dist, dev) in ur.kink_margins(r64["kinks"], r32["kinks"]).items():
        if kind == "q_min" and q_dev is not None:
            dq = np.asarray(q_dev, F64)
            dev = max(dev, float(np.abs((dq[:, 0] - dq[:, 1]) - (m["q"][:, 0] - m["q"][:, 1])).max()))
        f[f"(a) {kind}: distance {dist:.3g} >= {KINK_FACTOR:g} x deviation {dev:.3g}"] = bool(dist >= KINK_FACTOR * dev)
    # (b) no column near saturation
    f[f"(b) 1 - a^2 >= 2^-10 (min {m['w'].min():.3g})"] = bool(m["w"].min() >= W_FLOOR)
    # (c) the means are no cancelling means
    for n, t in m["terms"].items():
        if n == "entropy" and not c["learned"]:
            continue
        f[f"(c) {n}: 8 |mean| {8 * abs(t.mean()):.3g} >= mean |term| {np.abs(t).mean():.3g}"] = bool(8.0 * abs(t.mean()) >= np.abs(t).mean())
    if c["name"] == BOTH_WIN:  # (d) both critics win rows inside one 16-row tile, the rarer one at least a quarter of all rows
        k = m["k"]
        f["(d) both critics win inside one tile"] = bool(any(0 < k[t:t + 16].sum() < len(k[t:t + 16]) for t in range(0, len(k), 16)))
        f["(d) the rarer critic wins a quarter of the rows"] = bool(min(k.mean(), 1 - k.mean()) >= 0.25)
    if c["name"] == CLAMPED:  # (e) clamped columns on both sides, and columns that are not
        f["(e) log_std clamped on both sides"] = bool((m["l"] < sm.LOG_STD_MIN).any() and (m["l"] > sm.LOG_STD_MAX).any()
                                                      and ((m["l"] > sm.LOG_STD_MIN) & (m["l"] < sm.LOG_STD_MAX)).any())
    return f


@functools.lru_cache(maxsize=None)
def case(name, first_salt=0) -> dict:
    """The case under the first salt from `first_salt` on that meets the conditions (AssertionError when none below MAX_SALT does)."""
    for salt in range(first_salt, MAX_SALT):
        c = make(name, salt)
        if all(conditions(c).values()):
            return c
    raise AssertionError(f"{name}: no salt below {MAX_SALT} meets the conditions")


@functools.lru_cache(maxsize=None)
def references(name, first_salt=0) -> tuple:
    """(model64, autograd float64, autograd float32) of a case on its own eps, computed once."""
    c = case(name, first_salt)
    return model64(*args_of(c)), autograd(*args_of(c), dtype="float64"), autograd(*args_of(c), dtype="float32")
