"""The cases of the end-to-end update reference (tests/sb3_update_ref.py): the smallest shapes at which the one-call updates can still
go wrong, each of at most 10 optimiser steps; the conditions a case must meet on the CPU; and the project's bound per tensor.
Shared by tests/test_update_ref_cpu.py (conditions, mutants) and tests/test_update_ref_gpu.py (the device against the reference).

The bound, per tensor and per scalar:  |got - ref64| <= 8 * max(max|ref32 - ref64|, 2^-24 * max|ref64|)   (`ratio`: error / bound).
The conditions (`conditions`):
  (a) per kind of kink the smallest float64 distance is at least KINK_MARGIN = 16 times the largest float32-vs-float64 deviation,
  (b) a second float32 evaluation (rows reversed, matrix products transposed) stays within the bound,
  (c) with target_kl, every minibatch's float64 approx_kl is at least 10 % away from 1.5 * target_kl,
  (d) for every compared statistic that is a MEAN OF SIGNED TERMS (PPO's policy loss and approx_kl, TD3's actor loss) the bound is at
      least one float32 rounding of a typical term: 8 max(eps_ref, 2^-24 |stat|) >= 2^-24 * term, term as the reference reports it
      (mean |q| for the actor loss; for PPO the row's term times max(1, |log_prob|, |old_log_prob|), because one rounding of a
      log-probability moves that row's ratio by so much of itself).  This is tests/td3_model.py's condition "the actor loss is no
      cancelling mean", stated for the bound itself: where the terms cancel, the rule's floor lies below the roundings of the terms,
      and a scalar's eps_ref is ONE draw of rounding noise that may lie anywhere below them -- a float32 reference that happens to
      land within 1e-9 of float64 makes a bound no float32 evaluation can be asked to meet.
A case is drawn under the first salt below MAX_SALT that meets them; the bound and the rows compared never change.  (eps_ref is torch's
on the machine that runs the test, so the salt may differ between machines; the test judges the case that machine chose.)

Two things make the choice hold where it is used.  The smoothing noise of a TD3 or SAC case is the float64 model of the device's own
draw (explore_model.normals under the call's seed, rows and steps; the device is held to it within 1e-5 elsewhere), so the kinks a case
was chosen for are the kinks of the device's run; the GPU tests feed the reference the device's recorded draw and ask (a) of that run
again.  And a salt is taken only with TWICE the kink margin, SELECT_MARGIN: the other torch build or the device's last bits of noise
move a margin by a few per cent, not by half.
With target_kl the stop is put on a minibatch of full rows.  The stopping minibatch's approx_kl is compared on its own, and weighs as
much as a full minibatch in the mean SB3 logs; of ONE row it is one float32 evaluation of (e^x - 1) - x, x the difference of two
log-probabilities some ten times its size, and its eps_ref is one draw of one rounding: for the same case two torch builds gave
4.8e-7 and 7.9e-9, a bound that moves sixty-fold with the machine the reference runs on (condition (d) at its plainest).
"""
import functools

import numpy as np
import torch

import explore_model as em
import offpolicy_model as om
import replay_model as rm
import sb3_update_ref as ref
import train_model as tm

F32, F64 = np.float32, np.float64
KINK_MARGIN, KL_MARGIN, MAX_SALT = 16.0, 0.10, 64
SELECT_MARGIN = 2 * KINK_MARGIN


# ---- the bound -------------------------------------------------------------------------------------------------------------------------
def ratio(got, r64, r32) -> float:
    """|got - ref64| / (8 max(max|ref32 - ref64|, 2^-24 max|ref64|)) of one tensor or scalar; a NaN must meet a NaN."""
    g, a, b = (np.asarray(x, F64) for x in (got, r64, r32))
    assert g.shape == a.shape == b.shape, (g.shape, a.shape, b.shape)
    if np.isnan(a).any() or np.isnan(g).any():
        return 0.0 if np.array_equal(np.isnan(a), np.isnan(g)) and np.array_equal(g[~np.isnan(g)], a[~np.isnan(a)]) else np.inf
    err = float(np.abs(g - a).max()) if g.size else 0.0
    lim = 8.0 * max(float(np.abs(b - a).max()) if a.size else 0.0, 2.0 ** -24 * (float(np.abs(a).max()) if a.size else 0.0))
    return err / lim if lim > 0 else (0.0 if err == 0 else np.inf)


def ratios(got: dict, r64: dict, r32: dict) -> dict:
    """class -> the worst `ratio` over its tensors; the three dicts map a class to a list of tensors (or scalars)."""
    assert set(got) == set(r64) == set(r32)
    out = {}
    for k in got:
        assert len(got[k]) == len(r64[k]) == len(r32[k]), k
        out[k] = max((ratio(g, a, b) for g, a, b in zip(got[k], r64[k], r32[k])), default=0.0)
    return out


def conditions(r64, r32, second: dict, target_kl=None) -> dict:
    """{"kinks": kind -> (distance, deviation), "a": bool, "b": class -> ratio, "c": the smallest relative distance or None, "ok"}."""
    kinks = ref.kink_margins(r64["kinks"], r32["kinks"])
    a = all(dist >= KINK_MARGIN * dev for dist, dev in kinks.values())
    c = None
    if target_kl is not None:
        c = min(abs(kl - 1.5 * target_kl) / (1.5 * target_kl) for kl in r64["per_minibatch_kl"])
    d = {}
    for k, term in r64["terms"].items():
        if target_kl is None and k in ("approx_kl", "last_approx_kl"):
            continue  # compared only with target_kl
        v64, v32 = r64["stats"][k], r32["stats"][k]
        d[k] = 8.0 * max(abs(v32 - v64), 2.0 ** -24 * abs(v64)) / (2.0 ** -24 * term)
    ok = a and all(v <= 1.0 for v in second.values()) and (c is None or c >= KL_MARGIN) and all(v >= 1.0 for v in d.values())
    return {"kinks": kinks, "a": a, "b": second, "c": c, "d": d, "ok": ok,
            "select": ok and all(dist >= SELECT_MARGIN * dev for dist, dev in kinks.values())}


# ---- PPO -------------------------------------------------------------------------------------------------------------------------------
PPO_HYPER = dict(clip_range=0.2, vf_coef=0.5, ent_coef=0.01, lr=3e-3, adam_eps=1e-5, max_grad_norm=0.5)
PPO_SEED = 0x1234567890ABCDEF
# name: D, the actor's hidden widths, the critic's, A, activation, E, K, batch_size, n_epochs, what differs from PPO's defaults
PPO_CASES = {
    "base": (5, (8, 8), (8, 8), 3, "tanh", 3, 5, 4, 2, {}),
    # D crosses the 128-column chunk, the widths cross 64, minibatches of 17 and 16 rows.  SB3's default learning rate here and in the
    # deep actor: Adam moves every weight by about lr per step, a pre-activation over 131 inputs by lr * sum|x| -- at 3e-3 the float64
    # reference itself leaves the trust region within two steps (approx_kl 0.012, 0.031, 1.3, 5.0), the clip kills most rows' gradients
    # (a third to a half of a layer's are exactly zero) and Adam divides what is left, rounding noise, by sqrt(v) + eps.
    "value-clipped": (131, (65, 63), (65, 63), 5, "relu", 3, 11, 17, 2, {"clip_range_vf": 0.2, "lr": 3e-4}),
    "normalisation-off": (8, (8, 8), (8, 8), 4, "tanh", 5, 13, 16, 2, {"normalize_advantage": False}),
    # target_kl is chosen per salt so that the float64 reference stops inside epoch 1 of 3: a whole epoch before it, one never entered
    "target-kl": (8, (8, 8), (8, 8), 4, "tanh", 5, 13, 16, 3, {"target_kl": None}),
    "deep-actor": (45, (33, 130, 70), (), 3, "tanh", 3, 11, 33, 2, {"lr": 3e-4}),  # a one-layer critic, one minibatch of all 33 rows
}


def _layers(rng, sizes):
    return [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), (0.1 * rng.standard_normal(o)).astype(F32)) for i, o in zip(sizes[:-1], sizes[1:])]


def _forward64(layers, x, activation):
    x = np.asarray(x, F64)
    for i, (w, b) in enumerate(layers):
        x = x @ w.astype(F64).T + b.astype(F64)
        if i < len(layers) - 1:
            x = np.tanh(x) if activation == "tanh" else np.maximum(x, 0.0)
    return x


def flat(x, E, K):
    """A rollout array [K, E, ...] in the flat order of the sample indices, i = env * K + t."""
    return np.swapaxes(np.asarray(x), 0, 1).reshape((E * K,) + np.asarray(x).shape[2:])


def _ppo_make(name, salt) -> dict:
    D, ha, hc, A, activation, E, K, batch, n_epochs, extra = PPO_CASES[name]
    rng = np.random.default_rng([salt, len(name), D, A, E, K])
    actor, critic = _layers(rng, (D, *ha, A)), _layers(rng, (D, *hc, 1))
    log_std = (-0.5 + 0.1 * rng.standard_normal(A)).astype(F32)
    obs = rng.standard_normal((K, E, D)).astype(F32)
    mean, sd = _forward64(actor, obs, activation), np.exp(log_std.astype(F64))
    actions = (mean + sd * rng.standard_normal((K, E, A))).astype(F32)
    lp = (-((actions - mean) ** 2) / (2 * sd * sd) - log_std.astype(F64) - 0.5 * np.log(2 * np.pi)).sum(-1)
    # the old policy is a little off today's: log ratios over +-0.25 against a clip range of 0.2, old values +-0.4 against 0.2
    log_probs = (lp + rng.uniform(-0.25, 0.25, (K, E))).astype(F32)
    values = (_forward64(critic, obs, activation)[..., 0] + rng.uniform(-0.4, 0.4, (K, E))).astype(F32)
    adv = (rng.standard_normal((K, E)) * 2.0 + 0.3).astype(F32)
    rollout = {"observations": obs, "actions": actions, "values": values, "log_probs": log_probs, "advantages": adv,
               "returns": (values + adv).astype(F32)}
    n = E * K
    epochs = [[tm.indices(n, PPO_SEED, e)[s:s + B] for s, B in tm.minibatches(n, batch)] for e in range(n_epochs)]
    buffer = {k: flat(rollout[r], E, K) for k, r in (("obs", "observations"), ("actions", "actions"), ("values", "values"),
                                                     ("log_prob", "log_probs"), ("advantages", "advantages"), ("returns", "returns"))}
    c = {"name": name, "actor": actor, "critic": critic, "log_std": log_std, "activation": activation, "E": E, "K": K, "D": D, "A": A,
         "batch_size": batch, "n_epochs": n_epochs, "rollout": rollout, "buffer": buffer, "epochs": epochs, "seed": PPO_SEED,
         "kw": {**PPO_HYPER, **extra, "activation": activation}}
    if "target_kl" in extra:
        # The run up to a stop is the run without target_kl.  The stop is to fall inside epoch 1, behind its first minibatch: at the
        # minibatch i there whose approx_kl stands highest above every earlier one, with the threshold half way (in ratio) between.
        kl = np.asarray(ppo_run(dict(c, kw={**c["kw"], "target_kl": None}), torch.float64)["per_minibatch_kl"])
        first = len(epochs[0])
        gap, i = max((kl[i] / kl[:i].max(), i) for i in range(first + 1, 2 * first) if len(epochs[1][i - first]) == batch)
        c["kw"]["target_kl"] = float(np.sqrt(kl[i] * kl[:i].max()) / 1.5) if gap > 1 else float(kl.max())
        c["stop"] = (1, i - first)
    return c


def ppo_run(c, dtype, **more) -> dict:
    return ref.ppo_train(c["actor"], c["critic"], c["log_std"], c["buffer"], c["epochs"], dtype=dtype, **{**c["kw"], **more})


PPO_STATS = ("policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl_all_epochs", "clip_fraction", "loss", "explained_variance", "std")


def ppo_classes(r) -> dict:
    """What is compared of a PPO update, by class."""
    return {"params": r["params"], "exp_avg": r["exp_avg"], "exp_avg_sq": r["exp_avg_sq"], "stats": [r["stats"][k] for k in PPO_STATS]}


def ppo_exact(r) -> tuple:
    return r["step"], r["stats"]["minibatches"], r["stats"]["n_updates"], r["stop"]


# ---- TD3 / DDPG ------------------------------------------------------------------------------------------------------------------------
TD3_SEED = 0x7A46E7
TD3_HYPER = dict(gamma=0.99, tau=0.005, noise_clip=0.5, lr=1e-3)
NORM = dict(clip_obs=10.0, clip_reward=10.0, epsilon=1e-8)
# name: the arguments of offpolicy_model.Stack, then of its one_call
TD3_CASES = {
    "base": (dict(pos=4, full=True), dict(G=6, B=4, delay=2, first_update=0)),  # two critics, the ring wrapped
    "ddpg": (dict(pos=4, full=True, n_critics=1), dict(G=6, B=4, delay=1, first_update=0)),
    # D + A = 136 crosses the 128-column chunk with the seam inside a tile; B is a tile and a row
    "seam": (dict(D=131, A=5, hidden=(65, 63), activation="tanh", max_batch=32, with_norm=True), dict(G=5, B=17, delay=2, first_update=0)),
    "no-actor-step": (dict(pos=4, full=True), dict(G=2, B=4, delay=3, first_update=0)),
}
STACK_DEFAULTS = dict(E=3, R=7, D=5, A=3, hidden=(8, 8), n_critics=2, activation="relu", seed=1, pos=0, full=True, with_norm=False)


def gather(arrays, rows, envs, stats=None):
    """SB3's `_get_samples` in float64: (obs, actions, next_obs, dones * (1 - timeouts), rewards), normalised with `stats`."""
    o, n, r = (arrays[k][rows, envs].astype(F64) for k in ("observations", "next_observations", "rewards"))
    if stats is not None:
        o, n = (ref.normalised(x, stats["obs_mean"], stats["obs_var"], NORM["epsilon"], NORM["clip_obs"]) for x in (o, n))
        r = ref.normalised(r, 0.0, stats["ret_var"], NORM["epsilon"], NORM["clip_reward"])
    d = arrays["dones"][rows, envs].astype(F64) * (1.0 - arrays["timeouts"][rows, envs].astype(F64))
    return o, arrays["actions"][rows, envs].astype(F64), n, d, r


def drawn_batches(arrays, buffer_seed, first_call, G, B, upper, E, stats=None):
    return [gather(arrays, *rm.draw(buffer_seed, first_call + g, B, upper, E), stats) for g in range(G)]


def _td3_make(name, salt) -> dict:
    make, call = TD3_CASES[name]
    s = {**STACK_DEFAULTS, **make, "seed": 1 + salt}
    actor, critics = om.networks(s["D"], s["A"], s["hidden"], s["n_critics"], s["seed"])
    arrays, rng = om.contents(s["E"], s["R"], s["D"], s["A"], s["seed"])
    stats = None
    if s["with_norm"]:
        stats = {"obs_mean": 0.3 * rng.standard_normal(s["D"]), "obs_var": rng.uniform(0.5, 2.0, s["D"]), "ret_var": 1.7}
    upper = s["R"] if s["full"] else s["pos"]
    batches = drawn_batches(arrays, s["seed"] + 77, 0, call["G"], call["B"], upper, s["E"], stats)
    noise = [em.normals(TD3_SEED, np.arange(call["B"]), s["A"], call["first_update"] + g) for g in range(call["G"])]
    sigma = 0.2 if s["n_critics"] == 2 else 0.0
    kw = {**TD3_HYPER, "activation": s["activation"], "policy_delay": call["delay"], "sigma": sigma, "first_update": call["first_update"]}
    return {"name": name, "stack": {**make, "seed": s["seed"]}, "call": {**call, "seed": TD3_SEED}, "shape": s, "actor": actor, "critics": critics,
            "arrays": arrays, "norm": stats, "upper": upper, "batches": batches, "noise": noise, "kw": kw}


def td3_run(c, dtype, batches=None, noise=None, **more) -> dict:
    return ref.td3_train(c["actor"], c["critics"], c["actor"], c["critics"], batches or c["batches"], noise or c["noise"], dtype=dtype,
                         **{**c["kw"], **more})


TD3_STATS = ("critic_loss", "critic_0_loss", "critic_1_loss", "actor_loss", "last_critic_loss", "last_actor_loss")


def td3_classes(r) -> dict:
    return {"online": r["actor"] + r["critics"], "targets": r["target_actor"] + r["target_critics"],
            "actor_exp_avg": r["actor_opt"]["exp_avg"], "actor_exp_avg_sq": r["actor_opt"]["exp_avg_sq"],
            "critic_exp_avg": r["critic_opt"]["exp_avg"], "critic_exp_avg_sq": r["critic_opt"]["exp_avg_sq"],
            "stats": [r["stats"][k] for k in TD3_STATS]}


def td3_exact(r) -> tuple:
    return r["actor_opt"]["step"], r["critic_opt"]["step"], r["stats"]["n_updates"], r["stats"]["actor_steps"]


# ---- the critic half of SAC ------------------------------------------------------------------------------------------------------------
SAC_HYPER = dict(gamma=0.99, tau=0.005, ent_coef=0.2, lr=1e-3)
SAC_SEED, SAC_E, SAC_R, SAC_B, SAC_STEPS = 0x7A26E70000000001, 3, 7, 17, 4
# name: D, hidden widths, A, activation.  ReLU (SB3's default for SAC) is on the narrow case: at 131-(130, 70) with A = 65 the 80 000
# pre-activations of four steps come within 1e-5 of zero under every salt, against float32 deviations of 1e-6 -- condition (a) cannot
# hold there, so the wide case, which is there for the strides, runs tanh.
SAC_CASES = {"7-64-64-a5": (7, (64, 64), 5, "relu"), "131-130-70-a65": (131, (130, 70), 65, "tanh")}


def _sac_make(name, salt) -> dict:
    D, hidden, A, activation = SAC_CASES[name]
    nets = np.random.default_rng([salt, D, A])
    actor, critics = _layers(nets, (D, *hidden, 2 * A)), [_layers(nets, (D + A, *hidden, 1)) for _ in range(2)]
    # a target handle's own copies, another draw: SB3 starts the target critics at the online ones, but only unequal copies can show
    # which of the two a step read
    target_actor, target_critics = _layers(nets, (D, *hidden, 2 * A)), [_layers(nets, (D + A, *hidden, 1)) for _ in range(2)]
    arrays, rng = om.contents(SAC_E, SAC_R, D, A, 50 + salt)
    batches = drawn_batches(arrays, 9 + salt, 0, SAC_STEPS, SAC_B, SAC_R, SAC_E)
    noise = [em.normals(SAC_SEED, np.arange(SAC_B), A, u) for u in range(SAC_STEPS)]
    return {"name": name, "D": D, "A": A, "actor": actor, "critics": critics, "target_actor": target_actor, "target_critics": target_critics,
            "arrays": arrays, "buffer_seed": 9 + salt, "batches": batches, "noise": noise, "kw": {**SAC_HYPER, "activation": activation}}


def sac_run(c, dtype, batches=None, noise=None, **more) -> dict:
    return ref.sac_critic_steps(c["actor"], c["critics"], c["target_actor"], c["target_critics"], batches or c["batches"],
                                noise or c["noise"], dtype=dtype, **{**c["kw"], **more})


def sac_classes(r) -> dict:
    return {"critics": r["critics"], "targets": r["target_actor"] + r["target_critics"], "critic_exp_avg": r["critic_opt"]["exp_avg"],
            "critic_exp_avg_sq": r["critic_opt"]["exp_avg_sq"], "stats": [r["stats"]["critic_loss"], r["stats"]["last_critic_loss"]]}


# ---- a case under the first salt that meets the conditions ------------------------------------------------------------------------------
FAMILIES = {"ppo": (PPO_CASES, _ppo_make, ppo_run, ppo_classes), "td3": (TD3_CASES, _td3_make, td3_run, td3_classes),
            "sac": (SAC_CASES, _sac_make, sac_run, sac_classes)}


def check(family, c, **inputs) -> dict:
    """The float64 and float32 references of a case, the second float32 evaluation and the conditions: {"ref64", "ref32", "conditions"}."""
    _, _, run, classes = FAMILIES[family]
    r64, r32 = run(c, torch.float64, **inputs), run(c, torch.float32, **inputs)
    second = run(c, torch.float32, reverse_rows=True, transposed=True, **inputs)
    cond = conditions(r64, r32, ratios(classes(second), classes(r64), classes(r32)), c["kw"].get("target_kl"))
    return {"ref64": r64, "ref32": r32, "conditions": cond}


@functools.lru_cache(maxsize=None)
def case(family, name) -> dict:
    """The case, with "salt" and "checked" (`check`'s result), under the first salt for which the conditions hold."""
    _, make, _, _ = FAMILIES[family]
    for salt in range(MAX_SALT):
        c = make(name, salt)
        got = check(family, c)
        stops = "stop" not in c or got["ref64"]["stop"] == got["ref32"]["stop"] == c["stop"]  # the stop falls where the case wants it
        if got["conditions"]["select"] and stops:
            return {**c, "salt": salt, "checked": got}
    raise AssertionError(f"{family}/{name}: no salt below {MAX_SALT} meets the conditions")
