"""PPO's minibatch loss with stable-baselines3 2.3.2's value-function clipping (clip_range_vf = cv > 0) and its ANALYTIC gradients in
NumPy float64 -- what include/fleet_hip.h states per row under "the same with value-function clipping" --, SB3's own expression under
torch-CPU autograd (float64 to check the analytic gradients, float32 for eps_ref), and the old values of the cases of
tests/test_ppo_vclip_gpu.py.  Builds on tests/ppo_model.py: the networks, inputs and everything but the critic's tail are its own.
Shared with tests/test_ppo_vclip_cpu.py; nothing here needs a GPU or the library."""
import functools
import zlib

import numpy as np

import ppo_model as ppm

ROOT = ppm.ROOT
CLIP_RANGE_VF = 0.2
MAX_SALT = 8
SPREAD = 0.45  # old values lie within +-SPREAD of the model's: about half the rows inside a clip range of +-0.2


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def loss_and_grads(actor, critic, activation, log_std, obs, actions, old_log_prob, advantages, returns, old_values, clip_range_vf=CLIP_RANGE_VF,
                   clip_range=ppm.CLIP_RANGE, vf_coef=ppm.VF_COEF, ent_coef=ppm.ENT_COEF) -> dict:
    """ppo_model.loss_and_grads with the critic's tail of the header: {"grads", "stats", "values" (unclipped), "log_prob", "ratio",
    "alive", "pre", and "dl" = v - old, "inside", "values_pred"}."""
    m = ppm.loss_and_grads(actor, critic, activation, log_std, obs, actions, old_log_prob, advantages, returns, clip_range, vf_coef, ent_coef)
    cv = float(clip_range_vf)
    v, ov, ret = m["values"], np.asarray(old_values, np.float64), np.asarray(returns, np.float64)
    B = v.shape[0]
    dl = v - ov
    vp = ov + np.clip(dl, -cv, cv)
    inside = (dl >= -cv) & (dl <= cv)
    dv = np.where(inside, (2.0 * vf_coef / B) * (vp - ret), 0.0)
    xc = ppm._forward(critic, obs, activation)[0]
    na = 2 * len(actor)
    grads = m["grads"][:na] + ppm._backward(critic, xc, dv[:, None], activation) + m["grads"][-1:]
    stats = dict(m["stats"])
    stats["value_loss"] = float(((ret - vp) ** 2).mean())
    stats["loss"] = stats["policy_loss"] + ent_coef * stats["entropy_loss"] + vf_coef * stats["value_loss"]
    return {**m, "grads": grads, "stats": stats, "dl": dl, "inside": inside, "values_pred": vp}


def torch_loss_and_grads(actor, critic, activation, log_std, obs, actions, old_log_prob, advantages, returns, old_values,
                         clip_range_vf=CLIP_RANGE_VF, clip_range=ppm.CLIP_RANGE, vf_coef=ppm.VF_COEF, ent_coef=ppm.ENT_COEF,
                         dtype="float64") -> dict:
    """SB3's own loss expression, the value clip included, under torch-CPU autograd in `dtype`: {"grads", "stats"}."""
    import torch
    from torch import nn

    dt = getattr(torch, dtype)
    T = lambda v: torch.from_numpy(np.array(v, dtype=np.float32)).to(dt)  # noqa: E731
    params = [T(t).requires_grad_(True) for net in (actor, critic) for w, b in net for t in (w, b)] + [T(log_std).requires_grad_(True)]

    def run(ps, n, x):
        for i in range(n):
            x = nn.functional.linear(x, ps[2 * i], ps[2 * i + 1])
            if i < n - 1:
                x = torch.tanh(x) if activation == "tanh" else torch.relu(x)
        return x

    na = len(actor)
    x, adv = T(obs), T(advantages)
    dist = torch.distributions.Normal(run(params[:2 * na], na, x), torch.ones_like(params[-1]) * params[-1].exp())
    log_prob, entropy = dist.log_prob(T(actions)).sum(dim=1), dist.entropy().sum(dim=1)
    values = run(params[2 * na:-1], len(critic), x).flatten()
    ratio = torch.exp(log_prob - T(old_log_prob))
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    old = T(old_values)
    values_pred = old + torch.clamp(values - old, -clip_range_vf, clip_range_vf)
    value_loss = nn.functional.mse_loss(T(returns), values_pred)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    loss.backward()
    with torch.no_grad():
        lr = log_prob - T(old_log_prob)
        stats = {"policy_loss": policy_loss.item(), "value_loss": value_loss.item(), "entropy_loss": entropy_loss.item(), "loss": loss.item(),
                 "approx_kl": torch.mean((torch.exp(lr) - 1) - lr).item(),
                 "clip_fraction": torch.mean((torch.abs(ratio - 1) > clip_range).to(dt)).item()}
    return {"grads": [p.grad.numpy().astype(np.float64) for p in params], "stats": stats}


# ---- the old values of the cases of tests/test_ppo_vclip_gpu.py ------------------------------------------------------------------------
def seed(name, salt) -> int:
    return zlib.crc32(f"ppo-vclip/{name}/{salt}".encode())


def _old_values(name, salt) -> np.ndarray:
    v = ppm.model(name, ppm.ROWS)["values"]
    rng = np.random.default_rng(seed(name, salt))
    old = (v + rng.uniform(-SPREAD, SPREAD, ppm.ROWS)).astype(np.float32)
    old.setflags(write=False)
    return old


def facts_of(name, old_values, cv=CLIP_RANGE_VF) -> dict:
    """The conditions over a case's ROWS rows.  With them no branch of the clip can differ between float32 and float64."""
    dl = ppm.model(name, ppm.ROWS)["values"] - np.asarray(old_values, np.float64)
    inside = np.abs(dl) <= cv
    return {"a row clipped above among the first 16": bool((dl[:16] > cv).any()),
            "a row clipped below among the first 16": bool((dl[:16] < -cv).any()),
            "rows inside the range": bool(inside.sum() >= ppm.ROWS // 4),
            "no |v - old| within 1e-4 of the range": bool(np.abs(np.abs(dl) - cv).min() > 1e-4)}


@functools.lru_cache(maxsize=None)
def case(name) -> dict:
    """ppo_model.case(name) with "old_values" under the first salt in 0..MAX_SALT-1 for which the conditions hold ("vclip_salt")."""
    c = dict(ppm.case(name))
    for salt in range(MAX_SALT):
        old = _old_values(name, salt)
        if all(facts_of(name, old).values()):
            c["old_values"], c["vclip_salt"] = old, salt
            return c
    raise AssertionError(f"{name}: no salt below {MAX_SALT} meets the conditions")


def batch_args(c, B) -> tuple:
    """The arguments of loss_and_grads for the first B rows of a case."""
    return (*ppm.batch_args(c, B), c["old_values"][:B])


@functools.lru_cache(maxsize=None)
def model(name, B) -> dict:
    return loss_and_grads(*batch_args(case(name), B))


@functools.lru_cache(maxsize=None)
def reference32(name, B) -> dict:
    """torch-CPU float32 autograd of the same batch: eps_ref is its distance from `model`."""
    return torch_loss_and_grads(*batch_args(case(name), B), dtype="float32")


# ---- the tie case ------------------------------------------------------------------------------------------------------------------
TIE_CV, TIE_OLD = 0.25, (0.25, 0.75, 0.0, 1.0)  # v == 0.5: dl = +cv and -cv (ties: the gradient passes), +0.5 and -0.5 (clipped: it does not)


def tie_case(D=5, A=3) -> dict:
    """One-layer heads; the critic's W = 0 and b = 0.5, so v == 0.5 exactly in every arithmetic.  B = 4."""
    rng = np.random.default_rng(zlib.crc32(b"ppo-vclip/tie"))
    f32 = np.float32
    actor = [((rng.standard_normal((A, D)) * 0.3).astype(f32), (rng.standard_normal(A) * 0.1).astype(f32))]
    critic = [(np.zeros((1, D), f32), np.array([0.5], f32))]
    obs = rng.standard_normal((4, D)).astype(f32)
    log_std = np.zeros(A, f32)
    actions = (obs @ actor[0][0].T + actor[0][1] + rng.standard_normal((4, A)).astype(f32)).astype(f32)
    zero = np.zeros(4, f32)
    lp = ppm.loss_and_grads(actor, critic, "tanh", log_std, obs, actions, zero, zero, zero)["log_prob"]
    return {"actor": actor, "critic": critic, "activation": "tanh", "log_std": log_std, "obs": obs, "actions": actions,
            "old_log_prob": lp.astype(f32), "advantages": np.array([1.0, -1.0, 0.5, -0.5], f32),
            "returns": np.array([1.0, -0.5, 2.0, 0.25], f32), "old_values": np.array(TIE_OLD, f32)}
