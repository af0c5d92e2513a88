"""PPO's minibatch loss (stable-baselines3 2.3.2 `PPO.train`, clip_range_vf = None) and its ANALYTIC gradients in NumPy float64 from the
float32 weights and inputs -- what include/fleet_hip.h "PPO minibatch gradients on the device" states per element, nothing rounded on
the way -- the same loss as torch autograd (float64 to check the analytic gradients, CPU float32 for eps_ref), and the networks and
inputs of tests/test_ppo_grad_gpu.py.  Shared with tests/test_ppo_grad_cpu.py; nothing here needs a GPU or the library."""
import functools
import zlib

import numpy as np

import policy_model as pm

ROOT = pm.ROOT
STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")
CLIP_RANGE, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _forward(layers, x, activation):
    """-> (inputs of every layer, hidden pre-activations, the last layer's output), float64."""
    xs, pre, y = [], [], np.asarray(x, np.float64)
    for i, (w, b) in enumerate(layers):
        xs.append(y)
        y = y @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if i < len(layers) - 1:
            pre.append(y)
            y = np.tanh(y) if activation == "tanh" else np.where(y > 0, y, 0.0)
    return xs, pre, y


def _backward(layers, xs, d, activation):
    """d: the loss's gradient at the last layer's output -> [dW, db per layer]."""
    grads = [None] * (2 * len(layers))
    for l in range(len(layers) - 1, -1, -1):
        grads[2 * l], grads[2 * l + 1] = d.T @ xs[l], d.sum(0)
        if l:
            h = xs[l]  # the activation of layer l - 1
            d = (d @ np.asarray(layers[l][0], np.float64)) * ((1.0 - h * h) if activation == "tanh" else (h > 0).astype(np.float64))
    return grads


def loss_and_grads(actor, critic, activation, log_std, obs, actions, old_log_prob, advantages, returns, clip_range=CLIP_RANGE,
                   vf_coef=VF_COEF, ent_coef=ENT_COEF) -> dict:
    """{"grads": [dW, db per layer of the actor, of the critic, then dlog_std], "stats": {name: value}, "values", "log_prob", "ratio",
    "alive", "pre": the hidden pre-activations of both heads}."""
    ls, a = np.asarray(log_std, np.float64), np.asarray(actions, np.float64)
    old, adv, ret = (np.asarray(v, np.float64) for v in (old_log_prob, advantages, returns))
    B, c = a.shape[0], float(clip_range)
    xa, pre_a, mean = _forward(actor, obs, activation)
    xc, pre_c, v = _forward(critic, obs, activation)
    v = v[:, 0]
    sd = np.exp(ls)
    dm = a - mean
    lp = (-(dm * dm) / (2.0 * sd * sd) - ls - 0.5 * np.log(2.0 * np.pi)).sum(1)
    lr = lp - old
    ratio = np.exp(lr)
    lo, hi = 1.0 - c, 1.0 + c
    s1, s2 = adv * ratio, adv * np.clip(ratio, lo, hi)
    alive = ((ratio >= lo) & (ratio <= hi)) | (s1 < s2)
    glp = np.where(alive, -(adv * ratio) / B, 0.0)
    dmean = glp[:, None] * (dm / (sd * sd))
    dls = (glp[:, None] * ((dm * dm) / (sd * sd) - 1.0)).sum(0) - ent_coef
    dv = (2.0 * vf_coef / B) * (v - ret)
    entropy = float((0.5 + 0.5 * np.log(2.0 * np.pi) + ls).sum())
    stats = {"policy_loss": float(-np.minimum(s1, s2).mean()), "value_loss": float(((ret - v) ** 2).mean()), "entropy_loss": -entropy,
             "approx_kl": float(((ratio - 1.0) - lr).mean()), "clip_fraction": float((np.abs(ratio - 1.0) > c).mean())}
    stats["loss"] = stats["policy_loss"] + ent_coef * stats["entropy_loss"] + vf_coef * stats["value_loss"]
    grads = _backward(actor, xa, dmean, activation) + _backward(critic, xc, dv[:, None], activation) + [dls]
    return {"grads": grads, "stats": stats, "values": v, "log_prob": lp, "ratio": ratio, "alive": alive, "pre": pre_a + pre_c}


def torch_loss_and_grads(actor, critic, activation, log_std, obs, actions, old_log_prob, advantages, returns, clip_range=CLIP_RANGE,
                         vf_coef=VF_COEF, ent_coef=ENT_COEF, dtype="float64") -> dict:
    """SB3's own loss expression under torch-CPU autograd in `dtype`: {"grads", "stats"} as loss_and_grads."""
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
    value_loss = nn.functional.mse_loss(T(returns), values)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    loss.backward()
    with torch.no_grad():
        lr = log_prob - T(old_log_prob)
        stats = {"policy_loss": policy_loss.item(), "value_loss": value_loss.item(), "entropy_loss": entropy_loss.item(), "loss": loss.item(),
                 "approx_kl": torch.mean((torch.exp(lr) - 1) - lr).item(),
                 "clip_fraction": torch.mean((torch.abs(ratio - 1) > clip_range).to(dt)).item()}
    return {"grads": [p.grad.numpy().astype(np.float64) for p in params], "stats": stats}


# ---- the cases of tests/test_ppo_grad_gpu.py ----------------------------------------------------------------------------------------
ROWS = 33  # a case's rows; a batch of B takes the first B
BATCHES = (1, 16, 17, 33)  # one row; a full tile; a tile and a ragged row; two tiles and a ragged row
# name: (D, A, the actor's hidden widths, the critic's hidden widths, activation, batches)
CASES = {
    "5x3-one-layer": (5, 3, (), (), "tanh", BATCHES),  # no hidden layer
    "127x2-64-64-tanh": (127, 2, (64, 64), (64, 64), "tanh", BATCHES),
    "129x65-65-63-relu": (129, 65, (65, 63), (65, 63), "relu", BATCHES),  # the staging seam at 128, padding both ways, A over a wavefront
    "45x3-deep-actor": (45, 3, (33, 130, 70), (), "tanh", BATCHES),  # a four-layer actor beside a one-layer critic
    "388x50-400-300-tanh": (388, 50, (400, 300), (400, 300), "tanh", (33,)),  # the 16-row units, a stride above 256
}
MAX_SALT = 8


def seed(name, salt) -> int:
    return zlib.crc32(f"ppo/{name}/{salt}".encode())


def _make(name, salt) -> dict:
    D, A, ha, hc, activation, _ = CASES[name]
    rng = np.random.default_rng(seed(name, salt))
    actor, critic = pm.random_layers(rng, (D, *ha, A)), pm.random_layers(rng, (D, *hc, 1))
    obs = np.clip(rng.standard_normal((ROWS, D)), -5, 5).astype(np.float32)
    log_std = rng.uniform(-0.5, 0.3, A).astype(np.float32)
    eps = rng.standard_normal((ROWS, A)).astype(np.float32)
    mean = _forward(actor, obs, activation)[2]
    actions = (mean + np.exp(log_std.astype(np.float64)) * eps).astype(np.float32)
    adv = rng.standard_normal(ROWS).astype(np.float32)
    ret = rng.standard_normal(ROWS).astype(np.float32)
    zero = np.zeros(ROWS, np.float32)
    lp = loss_and_grads(actor, critic, activation, log_std, obs, actions, zero, adv, ret)["log_prob"]
    # spread: log ratios uniform over +-0.45 against a clip range of +-0.2: about half the rows inside
    old = (lp + rng.uniform(-0.45, 0.45, ROWS)).astype(np.float32)
    out = {"actor": actor, "critic": critic, "activation": activation, "log_std": log_std, "obs": obs, "actions": actions, "eps": eps,
           "old_log_prob": old, "advantages": adv, "returns": ret}
    for v in (obs, log_std, eps, actions, old, adv, ret):
        v.setflags(write=False)
    return out


def batch_args(c, B) -> tuple:
    """The arguments of loss_and_grads for the first B rows of a case."""
    return (c["actor"], c["critic"], c["activation"], c["log_std"], c["obs"][:B], c["actions"][:B], c["old_log_prob"][:B],
            c["advantages"][:B], c["returns"][:B])


def facts_of(c) -> dict:
    """The table's conditions over a case's ROWS rows.  With them no branch can differ between float32 and float64."""
    m = loss_and_grads(*batch_args(c, ROWS))
    ratio, alive, adv = m["ratio"], m["alive"], c["advantages"]
    lo, hi = 1.0 - CLIP_RANGE, 1.0 + CLIP_RANGE
    outside = (ratio < lo) | (ratio > hi)
    f = {"both signs of advantage": bool((adv > 0).any() and (adv < 0).any()),
         "a row clipped to zero gradient": bool((~alive).any()),
         "a row outside the range still alive": bool((outside & alive).any()),
         "rows inside the range": bool((~outside).sum() >= ROWS // 4),
         "no ratio within 1e-4 of a bound": bool(np.minimum(np.abs(ratio - lo), np.abs(ratio - hi)).min() > 1e-4),
         "no zero advantage": bool((adv != 0).all())}
    if c["activation"] == "relu":
        f["no relu pre-activation within 1e-5 of zero"] = bool(all(np.abs(p).min() > 1e-5 for p in m["pre"]))
    return f


@functools.lru_cache(maxsize=None)
def case(name) -> dict:
    """The case under the first salt in 0..MAX_SALT-1 for which the conditions hold (AssertionError when none does)."""
    for salt in range(MAX_SALT):
        c = _make(name, salt)
        if all(facts_of(c).values()):
            c["salt"] = salt
            return c
    raise AssertionError(f"{name}: no salt below {MAX_SALT} meets the conditions")


@functools.lru_cache(maxsize=None)
def model(name, B) -> dict:
    return loss_and_grads(*batch_args(case(name), B))


@functools.lru_cache(maxsize=None)
def reference32(name, B) -> dict:
    """torch-CPU float32 autograd of the same batch: eps_ref is its distance from `model`."""
    return torch_loss_and_grads(*batch_args(case(name), B), dtype="float32")


def tensor_names(name) -> list:
    _, _, ha, hc, _, _ = CASES[name]
    return [f"{net}.{l}.{k}" for net, n in (("actor", len(ha) + 1), ("critic", len(hc) + 1)) for l in range(n) for k in ("W", "b")] + ["log_std"]
