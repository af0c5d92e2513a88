"""TD3's two minibatch losses (stable-baselines3 2.3.2 `TD3.train`: `sum(F.mse_loss(q_c, y))` over the critics, and
`-critic.q1_forward(obs, actor(obs)).mean()`) and their ANALYTIC gradients in NumPy float64 from the float32 weights and inputs -- what
include/fleet_hip.h "TD3 / DDPG minibatch gradients on the device" states per element, nothing rounded on the way -- the same losses
as torch autograd (float64 to check the analytic gradients, CPU float32 for eps_ref), and the networks and inputs of
tests/test_td3_grad_gpu.py.  Shared with tests/test_td3_grad_cpu.py; nothing here needs a GPU or the library."""
import functools
import zlib

import numpy as np

import policy_model as pm

ROOT = pm.ROOT
CRITIC_STATS = ("critic_loss", "critic_0_loss", "critic_1_loss")
ACTOR_STATS = ("actor_loss",)
CLIP = (-0.3, 0.7)  # the bounds of a CLIP actor: not +-1, and inside what its means reach


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
    """d: the loss's gradient at the last layer's output -> ([dW, db per layer], the gradient at the network's input)."""
    grads = [None] * (2 * len(layers))
    for l in range(len(layers) - 1, -1, -1):
        grads[2 * l], grads[2 * l + 1] = d.T @ xs[l], d.sum(0)
        d = d @ np.asarray(layers[l][0], np.float64)
        if l:
            h = xs[l]  # the activation of layer l - 1
            d = d * ((1.0 - h * h) if activation == "tanh" else (h > 0).astype(np.float64))
    return grads, d


def critic_loss_and_grads(critics, activation, obs, actions, target_q) -> dict:
    """{"grads": [dW, db per layer of critic 0, then of critic 1], "stats": {name: value}, "q" [B, n_critics], "e" [B, n_critics],
    "pre": the hidden pre-activations}."""
    x = np.concatenate([np.asarray(obs, np.float64), np.asarray(actions, np.float64)], axis=1)  # the observation, then the action
    y = np.asarray(target_q, np.float64).reshape(-1)
    B = x.shape[0]
    grads, pre, qs, es, losses = [], [], [], [], []
    for layers in critics:
        xs, p, q = _forward(layers, x, activation)
        e = q[:, 0] - y
        g, _ = _backward(layers, xs, ((2.0 / B) * e)[:, None], activation)
        grads += g
        pre += p
        qs.append(q[:, 0])
        es.append(e)
        losses.append(float((e * e).mean()))
    stats = {"critic_loss": float(sum(losses)), "critic_0_loss": losses[0], "critic_1_loss": losses[1] if len(losses) == 2 else 0.0}
    return {"grads": grads, "stats": stats, "q": np.stack(qs, 1), "e": np.stack(es, 1), "pre": pre}


def actor_loss_and_grads(actor, critics, activation, output, low, high, obs) -> dict:
    """{"grads": [dW, db per layer of the actor], "stats": {"actor_loss"}, "actions", "q", "mean", "pre": the hidden pre-activations of
    the actor and of critic 0 over concat(obs, actions)}.  Only critic 0 enters."""
    obs = np.asarray(obs, np.float64)
    B, D = obs.shape
    xa, pre_a, mean = _forward(actor, obs, activation)
    if output == "tanh":
        a = np.tanh(mean)
        g = 1.0 - a * a
    elif output == "clip":
        a = np.clip(mean, low, high)
        g = ((mean >= low) & (mean <= high)).astype(np.float64)  # torch's clamp: the bounds inclusive
    else:
        a, g = mean, np.ones_like(mean)
    xc, pre_c, q = _forward(critics[0], np.concatenate([obs, a], axis=1), activation)
    _, dx = _backward(critics[0], xc, np.full((B, 1), -1.0 / B), activation)
    grads, _ = _backward(actor, xa, dx[:, D:] * g, activation)  # into the action columns only
    return {"grads": grads, "stats": {"actor_loss": float(-q[:, 0].mean())}, "actions": a, "q": q[:, 0], "mean": mean, "pre": pre_a + pre_c}


def _torch_nets(actor, critics, dt):
    import torch

    T = lambda v: torch.from_numpy(np.array(v, dtype=np.float32)).to(dt)  # noqa: E731
    pa = [T(t).requires_grad_(True) for w, b in actor for t in (w, b)]
    pc = [[T(t).requires_grad_(True) for w, b in net for t in (w, b)] for net in critics]
    return T, pa, pc


def _torch_run(ps, x, activation):
    import torch
    from torch import nn

    n = len(ps) // 2
    for i in range(n):
        x = nn.functional.linear(x, ps[2 * i], ps[2 * i + 1])
        if i < n - 1:
            x = torch.tanh(x) if activation == "tanh" else torch.relu(x)
    return x


def torch_critic_loss_and_grads(critics, activation, obs, actions, target_q, dtype="float64") -> dict:
    """SB3's own expression under torch-CPU autograd in `dtype`: {"grads", "stats"} as critic_loss_and_grads."""
    import torch
    from torch import nn

    T, _, pc = _torch_nets([], critics, getattr(torch, dtype))
    y = T(np.asarray(target_q).reshape(-1, 1))
    current = [_torch_run(ps, torch.cat([T(obs), T(actions)], dim=1), activation) for ps in pc]  # ContinuousCritic.forward
    each = [nn.functional.mse_loss(q, y) for q in current]
    loss = sum(each)
    loss.backward()
    stats = {"critic_loss": loss.item(), "critic_0_loss": each[0].item(), "critic_1_loss": each[1].item() if len(each) == 2 else 0.0}
    return {"grads": [p.grad.numpy().astype(np.float64) for ps in pc for p in ps], "stats": stats}


def torch_actor_loss_and_grads(actor, critics, activation, output, low, high, obs, dtype="float64") -> dict:
    """-critic.q1_forward(obs, actor(obs)).mean() under torch-CPU autograd in `dtype`: {"grads" (the actor's), "stats"}."""
    import torch

    T, pa, pc = _torch_nets(actor, critics, getattr(torch, dtype))
    x = T(obs)
    mean = _torch_run(pa, x, activation)
    a = torch.tanh(mean) if output == "tanh" else (torch.clamp(mean, low, high) if output == "clip" else mean)
    loss = -_torch_run(pc[0], torch.cat([x, a], dim=1), activation).mean()
    loss.backward()
    return {"grads": [p.grad.numpy().astype(np.float64) for p in pa], "stats": {"actor_loss": loss.item()}}


# ---- the cases of tests/test_td3_grad_gpu.py ----------------------------------------------------------------------------------------
ROWS = 33  # a case's rows; a batch of B takes the first B
BATCHES = (1, 16, 17, 33)  # one row; a full tile; a tile and a ragged row; two tiles and a ragged row
# name: (D, A, the actor's hidden widths, a critic's hidden widths, activation, the actor's output, n_critics, batches)
CASES = {
    "5x3-one-layer": (5, 3, (), (), "tanh", "tanh", 2, BATCHES),  # no hidden layer anywhere
    "5x3-one-layer-ddpg": (5, 3, (), (), "tanh", "tanh", 1, BATCHES),
    "127x2-64-64-tanh": (127, 2, (64, 64), (64, 64), "tanh", "tanh", 2, BATCHES),  # D + A = 129: the seam one past the staged chunk
    "126x5-64-64-relu": (126, 5, (64, 64), (64, 64), "relu", "tanh", 2, BATCHES),  # the seam inside the first chunk
    "126x5-64-64-relu-ddpg": (126, 5, (64, 64), (64, 64), "relu", "tanh", 1, BATCHES),
    "129x65-65-63-relu-clip": (129, 65, (65, 63), (65, 63), "relu", "clip", 2, BATCHES),  # padding both ways, A over a wavefront, bounds that bite
    "45x3-deep-actor": (45, 3, (33, 130, 70), (), "tanh", "none", 2, BATCHES),  # a four-layer actor beside one-layer critics
    "45x3-deep-critic": (45, 3, (), (33, 130, 70), "tanh", "tanh", 2, BATCHES),  # ... and the reverse
    "388x50-400-300-tanh": (388, 50, (400, 300), (400, 300), "tanh", "tanh", 2, (33,)),  # the 16-row units, a stride above 256
}
MAX_SALT = 8


def seed(name, salt) -> int:
    return zlib.crc32(f"td3/{name}/{salt}".encode())


def _make(name, salt) -> dict:
    D, A, ha, hc, activation, output, nc, _ = CASES[name]
    rng = np.random.default_rng(seed(name, salt))
    actor = pm.random_layers(rng, (D, *ha, A))
    if output == "clip":  # means that reach past the bounds
        actor[-1] = ((actor[-1][0] * np.float32(4.0)).astype(np.float32), actor[-1][1])
    critics = [pm.random_layers(rng, (D + A, *hc, 1)) for _ in range(nc)]
    obs = np.clip(rng.standard_normal((ROWS, D)), -5, 5).astype(np.float32)
    actions = rng.uniform(-1, 1, (ROWS, A)).astype(np.float32)
    target_q = rng.standard_normal(ROWS).astype(np.float32)
    for v in (obs, actions, target_q):
        v.setflags(write=False)
    return {"actor": actor, "critics": critics, "activation": activation, "output": output, "low": CLIP[0], "high": CLIP[1], "obs": obs,
            "actions": actions, "target_q": target_q}


def critic_args(c, B) -> tuple:
    """The arguments of critic_loss_and_grads for the first B rows of a case."""
    return c["critics"], c["activation"], c["obs"][:B], c["actions"][:B], c["target_q"][:B]


def actor_args(c, B) -> tuple:
    return c["actor"], c["critics"], c["activation"], c["output"], c["low"], c["high"], c["obs"][:B]


def facts_of(c) -> dict:
    """The table's conditions over a case's ROWS rows.  With them no branch can differ between float32 and float64."""
    mc, ma = critic_loss_and_grads(*critic_args(c, ROWS)), actor_loss_and_grads(*actor_args(c, ROWS))
    f = {"TD errors of both signs": bool(((mc["e"] > 0).any(0) & (mc["e"] < 0).any(0)).all())}
    # The actor loss is a MEAN of signed terms, and the rule's floor, 8 * 2^-24 * |mean q|, is counted in roundings of the result.  Every
    # q[b] carries at least one float32 rounding of its own magnitude whatever computes it, so where the terms cancel the floor lies
    # below the roundings of the terms and the rule measures the cancellation, not the arithmetic (a scalar's eps_ref, one draw of
    # rounding noise, may lie anywhere below that).  The floor covers one rounding of a typical term where 8 |mean q| >= mean |q|:
    # asked of every batch of the case.
    q = ma["q"]
    f["the actor loss is no cancelling mean"] = bool(all(8.0 * abs(q[:B].mean()) >= np.abs(q[:B]).mean() for B in BATCHES))
    if c["activation"] == "relu":
        f["no relu pre-activation within 1e-5 of zero"] = bool(all(np.abs(p).min() > 1e-5 for p in mc["pre"] + ma["pre"]))
    if c["output"] == "clip":
        mean, lo, hi = ma["mean"], c["low"], c["high"]
        f["no mean within 1e-4 of a bound"] = bool(np.minimum(np.abs(mean - lo), np.abs(mean - hi)).min() > 1e-4)
        f["means clipped at both bounds"] = bool((mean < lo).any() and (mean > hi).any())
        f["means not clipped"] = bool(((mean > lo) & (mean < hi)).any())
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
    """{"critic": ..., "actor": ...} of the float64 model."""
    c = case(name)
    return {"critic": critic_loss_and_grads(*critic_args(c, B)), "actor": actor_loss_and_grads(*actor_args(c, B))}


@functools.lru_cache(maxsize=None)
def reference32(name, B) -> dict:
    """torch-CPU float32 autograd of the same batch: eps_ref is its distance from `model`."""
    c = case(name)
    return {"critic": torch_critic_loss_and_grads(*critic_args(c, B), dtype="float32"),
            "actor": torch_actor_loss_and_grads(*actor_args(c, B), dtype="float32")}


def tensor_names(name) -> dict:
    _, _, ha, hc, _, _, nc, _ = CASES[name]
    names = lambda net, n: [f"{net}.{l}.{k}" for l in range(n) for k in ("W", "b")]  # noqa: E731
    return {"actor": names("actor", len(ha) + 1), "critic": [n for c in range(nc) for n in names(f"critic{c}", len(hc) + 1)]}
