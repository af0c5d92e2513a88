"""SAC's actor and entropy-coefficient gradients on the device (fleet_sac_actor_grad_dev; fleet_td3.hip sac_actor_rows, sac_weights)
against tests/sac_grad_model.py: the forward in bits against `DeviceSACNetworks.act` and `critic_grad`, the head deltas and a one-layer
actor's gradients in bits against the header's float32 order, every gradient tensor and statistic within the project's bound of the
float64 model, what a result may depend on, the refusals that need a handle, `gradient_step` against SB3's loop under autograd, and the
example.  Needs an MI355X.

The critic's da has an exact float32 restatement only where the critics have no hidden layer (a hidden layer's activations are not
exported), so the head deltas are held to bits in the one-layer cases and the saturated case, and to the bound everywhere."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import policy_bits as pb
import sac_grad_model as gm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(gm.ROOT, "profiles", "sac_grad_parity.json")
SEED, STEP, OFFSET = 0x5AC6000000000123, 7, 40
_parity = {}


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def host(t):
    return t.detach().cpu().numpy()


def on_device(a):
    return torch.from_numpy(np.array(a, np.float32)).to(dev())


def write_parity():
    """The figures are printed; they go to profiles/sac_grad_parity.json only when FLEET_WRITE_PARITY=1 asks for it (a test run leaves
    the tree as it found it), merged into the cases the file already holds."""
    if os.environ.get("FLEET_WRITE_PARITY") != "1":
        return
    cases = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as fh:
            cases = json.load(fh).get("cases", {})
    cases.update(_parity)
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as fh:
        json.dump({"bound": "worst |device - float64 model| / (8 * max(eps_ref, 2^-24 * max|ref|)) per tensor class; <= 1 passes",
                   "cases": dict(sorted(cases.items()))}, fh, indent=1)
        fh.write("\n")


def leaves(layers):
    return [on_device(t).requires_grad_(True) for w, b in layers for t in (w, b)]


class Rig:
    """The online networks of a case, the gradient handle on them, and torch leaves for every parameter."""

    def __init__(self, c, max_batch=None):
        from fleetrl_amd import DeviceSACGrad, DeviceSACNetworks

        self.c = c
        self.nets = DeviceSACNetworks(c["actor"], c["critics"], activation=c["activation"])
        self.grad = DeviceSACGrad(self.nets, c["B"] if max_batch is None else max_batch)
        self.actor_params = leaves(c["actor"])
        self.critic_params = [p for net in c["critics"] for p in leaves(net)]
        self.alpha = torch.full((1,), c["alpha"], device=dev())
        self.log_ent_coef = torch.full((1,), c["log_ent_coef"], device=dev(), requires_grad=True) if c["learned"] else None

    def call(self, obs=None, optional=True, given=None, noise=None, **kw):
        """One call of the entry on the case's rows; every output as a tensor (the optional ones only when asked for)."""
        c = self.c
        B, A = c["B"], c["A"]
        obs = on_device(c["obs"]) if obs is None else obs
        given = c["given"] if given is None else given
        out = {}
        if optional:
            out = {"actions": torch.full((B, A), 9.0, device=dev()), "log_prob": torch.full((B,), 9.0, device=dev()),
                   "q": torch.full((B, c["n_critics"]), 9.0, device=dev()), "dheads": torch.full((B, 2 * A), 9.0, device=dev())}
        if noise is None and (given or optional):
            noise = on_device(c["eps"]) if given else torch.full((B, A), 9.0, device=dev())
        out["stats"] = self.grad.actor_grad(obs, ent_coef=self.alpha, seed=SEED, step=STEP, row_offset=OFFSET, into=self.actor_params,
                                            log_ent_coef=self.log_ent_coef, target_entropy=c["target_entropy"], noise=noise, noise_given=given,
                                            actions_out=out.get("actions"), log_prob_out=out.get("log_prob"), q_out=out.get("q"),
                                            dheads_out=out.get("dheads"), **kw)
        out["noise"] = noise
        torch.cuda.synchronize()
        return out

    def results(self, out) -> dict:
        """What the bound judges, in the model's layout."""
        st = host(out["stats"]).astype(np.float64)
        return {"grads": [host(p.grad).astype(np.float64) for p in self.actor_params], "stats": dict(zip(gm.SAC_ACTOR_STATS, st[:5])),
                "log_ent_coef_grad": float(self.log_ent_coef.grad[0]) if self.log_ent_coef is not None else None}

    def result_bits(self, out):
        extra = [bits(self.log_ent_coef.grad)] if self.log_ent_coef is not None else []
        return [bits(p.grad) for p in self.actor_params] + [bits(out["stats"])] + extra

    def close(self):
        self.grad.close(), self.nets.close()


@functools.lru_cache(maxsize=None)
def judged(name) -> dict:
    """The run of a case that is judged: the first salt whose conditions hold on the CPU and again for the device's own run (its drawn
    noise, its critic outputs).  {"c", "out": numpy outputs, "got", "m", "r32", "eps"}; computed once and shared."""
    first = 0
    while True:
        c = gm.case(name, first)
        rig = Rig(c)
        out = rig.call()
        eps = host(out["noise"])
        facts = gm.conditions(c, eps=eps, q_dev=host(out["q"]))
        if all(facts.values()):
            break
        print(f"{name}: salt {c['salt']} misses {[k for k, v in facts.items() if not v]} on the device's run: the next salt")
        first = c["salt"] + 1
        rig.close()
    got = rig.results(out)
    out_np = {k: host(v) for k, v in out.items() if v is not None}
    log_std = torch.empty((c["B"], c["A"]), device=dev())
    rig.nets.act(on_device(c["obs"]), seed=SEED, step=STEP, env_id_offset=OFFSET, noise=on_device(eps), noise_given=True, log_std_out=log_std)
    out_np["log_std"] = host(log_std)
    rig.close()
    m, r32 = gm.model64(*gm.args_of(c, eps)), gm.autograd(*gm.args_of(c, eps), dtype="float32")
    return {"c": c, "out": out_np, "got": got, "m": m, "r32": r32, "eps": eps}


# ---- 1. bits: the forward is the act launch's and the critic launch's ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_actions_noise_log_prob_and_q_are_the_bits_of_act_and_critic_grad(name):
    c = gm.case(name)
    rig = Rig(c)
    out = rig.call()
    B, A = c["B"], c["A"]
    x = on_device(c["obs"])
    rec, lp = torch.full((B, A), 9.0, device=dev()), torch.full((B,), 9.0, device=dev())
    a = rig.nets.act(x, seed=SEED, step=STEP, env_id_offset=OFFSET, noise=on_device(c["eps"]) if c["given"] else rec, noise_given=c["given"],
                     log_prob_out=lp)
    assert np.array_equal(bits(out["actions"]), bits(a)) and np.array_equal(bits(out["log_prob"]), bits(lp))
    if not c["given"]:
        assert np.array_equal(bits(out["noise"]), bits(rec)) and (host(rec) != 9.0).all()
    q = torch.full((B, c["n_critics"]), 9.0, device=dev())
    rig.grad.critic_grad((x, a), torch.zeros(B, device=dev()), into=rig.critic_params, q_out=q)
    assert np.array_equal(bits(out["q"]), bits(q))
    rig.close()


# ---- 2. bits: the head deltas and a one-layer actor's gradients ---------------------------------------------------------------------
def _one_layer_bits(c, out, log_std, grads):
    k = np.zeros(c["B"], np.int64) if c["n_critics"] == 1 else np.where(out["q"][:, 0] <= out["q"][:, 1], 0, 1)
    da = gm.da_one_layer32(c["critics"], c["D"], k, c["B"])
    want = gm.dheads32(out["actions"], out["noise"], log_std, da, c["alpha"], c["B"])
    assert pb.same_bits(out["dheads"], want), np.abs(out["dheads"] - want).max()
    dW, db = gm.chain_dW32(out["dheads"], c["obs"])  # over the device's own deltas
    assert pb.same_bits(grads[0], dW) and pb.same_bits(grads[1], db)
    return k


@pytest.mark.parametrize("name", gm.ONE_LAYER)
def test_one_layer_head_deltas_and_gradients_are_the_headers_float32_order(name):
    j = judged(name)
    k = _one_layer_bits(j["c"], j["out"], j["out"]["log_std"], [g.astype(np.float32) for g in j["got"]["grads"]])
    if j["c"]["n_critics"] == 2:
        assert len(set(k)) == 2  # both critics' da enter


def test_saturated_columns_follow_the_float32_order_in_bits():
    """|u| > 12: 1 - a^2 == 0 in float32 in every column.  One ulp of tanhf moves the float64 answer there, so the case is held to
    the float32 restatement fed the device's stored a, and to nothing else."""
    c = gm.saturated_case()
    rig = Rig(c)
    out = rig.call()
    log_std = torch.empty((c["B"], c["A"]), device=dev())
    rig.nets.act(on_device(c["obs"]), seed=SEED, step=STEP, env_id_offset=OFFSET, noise=out["noise"], noise_given=True, log_std_out=log_std)
    o = {k: host(v) for k, v in out.items()}
    assert (np.abs(o["actions"]) == 1.0).all() and np.isfinite(o["dheads"]).all() and np.isfinite(o["stats"]).all()
    _one_layer_bits(c, o, host(log_std), [host(p.grad) for p in rig.actor_params])
    assert (o["dheads"][:, :c["A"]] == 0).all()  # du = dLa * 0
    rig.close()


# ---- 3. the bound --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_gradients_and_statistics_lie_within_the_bound_of_the_float64_model(name):
    j = judged(name)
    c, m, r32, got = j["c"], j["m"], j["r32"], j["got"]
    ratios = gm.class_ratios(got, m, r32, c["learned"])
    ratios["dheads"] = gm.ratio(j["out"]["dheads"], m["dheads"], r32["dheads"])
    print(f"{name}: salt {c['salt']}, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    _parity[name] = {"salt": c["salt"], **{k: round(float(v), 4) for k, v in ratios.items()}}
    write_parity()
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert c["learned"] or got["stats"]["ent_coef_loss"] == 0.0
    q = j["out"]["q"]
    k_dev = np.zeros(c["B"], np.int64) if c["n_critics"] == 1 else np.where(q[:, 0] <= q[:, 1], 0, 1)
    assert np.array_equal(k_dev, m["k"])  # the device selected the model's critic in every row


def test_the_statistics_behind_slot_four_are_zero_and_alpha_is_as_read():
    j = judged("7x1-one-layer-twin")
    st = j["out"]["stats"]
    assert (st[5:] == 0).all() and st[4] == np.float32(j["c"]["alpha"])


# ---- 4. what a result depends on ---------------------------------------------------------------------------------------------------
def test_results_depend_on_the_inputs_and_B_alone():
    """Two calls, a call on another stream, a larger max_batch, NaN rows behind row B, NaN-filled .grad tensors and a call without the
    optional outputs give identical bits; the critics' .grad is not touched."""
    c = gm.case(gm.BOTH_WIN)
    B, D = c["B"], c["D"]
    rig = Rig(c)
    first = rig.call()
    eps = first["noise"].clone()
    ref = rig.result_bits(first)
    per_row = [bits(first[k]) for k in ("actions", "log_prob", "q", "dheads")]
    again = rig.call()
    assert all(np.array_equal(a, b) for a, b in zip(ref, rig.result_bits(again)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = rig.call()
    assert all(np.array_equal(a, b) for a, b in zip(ref, rig.result_bits(other)))
    rig.close()
    big = Rig(c, max_batch=3 * B + 5)
    padded = torch.full((B + 9, D), float("nan"), device=dev())
    padded[:B] = on_device(c["obs"])
    for p in big.actor_params:
        p.grad = torch.full_like(p, float("nan"))
    sentinel = [torch.full_like(p, 3.0) for p in big.critic_params]
    for p, g in zip(big.critic_params, sentinel):
        p.grad = g.clone()
    out = big.call(obs=padded[:B])
    assert all(np.array_equal(a, b) for a, b in zip(ref, big.result_bits(out)))
    assert all(np.array_equal(a, bits(out[k])) for a, k in zip(per_row, ("actions", "log_prob", "q", "dheads")))
    assert all(torch.equal(p.grad, g) for p, g in zip(big.critic_params, sentinel))
    bare = big.call(optional=False, given=True, noise=eps)  # the draw handed back in: no optional output is written
    assert all(np.array_equal(a, b) for a, b in zip(ref, big.result_bits(bare)))
    drawn = big.call(optional=False, given=False)  # ... and drawn again with nowhere to record it
    assert all(np.array_equal(a, b) for a, b in zip(ref, big.result_bits(drawn)))
    big.close()


def test_ent_coef_is_read_on_the_device_when_the_launch_runs():
    c = gm.case("7x5-8-8-relu-twin")
    rig = Rig(c)
    a = rig.call()
    before, st = rig.result_bits(a), host(a["stats"])
    rig.alpha.mul_(2.0)  # on the device, enqueued: the host never learns the value
    b = rig.call()
    st2 = host(b["stats"])
    assert st2[4] == np.float32(2.0) * st[4] and st2[0] != st[0] and st2[2] == st[2] and st2[3] == st[3]
    assert not np.array_equal(before[0], rig.result_bits(b)[0])
    rig.close()


# ---- 5. refusals that need a handle ------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_handle_launch_nothing():
    from fleetrl_amd import DeviceTD3Grad, DeviceTD3Target, FleetHipError, _capi

    c = gm.case("7x5-8-8-relu-twin")
    rig = Rig(c)
    lib, B, A = rig.grad.lib, c["B"], c["A"]
    x, stats = on_device(c["obs"]), torch.full((8,), 5.0, device=dev())
    ptrs = rig.grad._grad_pointers("actor", rig.actor_params, rig.grad._shapes["actor"], "the actor's")
    n = len(rig.actor_params)
    for p in rig.actor_params:
        p.grad.fill_(7.0)

    def args(**over):
        a = _capi.FleetSacActorArgs()
        a.struct_bytes, a.B, a.obs, a.ent_coef, a.stats = C.sizeof(a), B, x.data_ptr(), rig.alpha.data_ptr(), stats.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    one = torch.zeros(1, device=dev())
    for a, count, reason in ((args(B=B + 1), n, f"B must be at most max_batch = {B}, got {B + 1}"),
                             (args(), n - 2, f"expected {n} gradient tensors (W, b per layer of the actor), got {n - 2}"),
                             (args(struct_bytes=8), n, "FleetSacActorArgs.struct_bytes does not match"), (args(B=0), n, "B must be >= 1"),
                             (args(obs=None), n, "null obs"), (args(ent_coef=None), n, "null ent_coef"), (args(stats=None), n, "null stats"),
                             (args(noise_mode=1), n, "noise_mode GIVEN with a null noise"), (args(noise_mode=3), n, "unknown noise_mode 3"),
                             (args(log_ent_coef=one.data_ptr()), n, "given together"), (args(log_ent_coef_grad=one.data_ptr()), n, "given together"),
                             (args(reserved=2), n, "reserved must be 0"), (args(row_offset=-3), n, "row_offset must be >= 0")):
        assert lib.fleet_sac_actor_grad_dev(rig.grad.h, C.byref(a), ptrs, count) == _capi.ERR_INVALID
        msg = lib.fleet_td3_last_error(rig.grad.h).decode()
        assert msg.startswith("fleet_sac_actor_grad_dev: ") and reason in msg, msg
    with pytest.raises(ValueError, match="noise_given needs the noise tensor"):
        rig.grad.actor_grad(x, ent_coef=rig.alpha, seed=1, step=1, into=rig.actor_params, noise_given=True)
    torch.cuda.synchronize()
    assert (host(stats) == 5.0).all() and all((host(p.grad) == 7.0).all() for p in rig.actor_params)  # nothing was launched
    # networks that are not squashed: the TD3 entry's business, and the message says so
    td3_actor = [(w[:A], b[:A]) if i == len(c["actor"]) - 1 else (w, b) for i, (w, b) in enumerate(c["actor"])]
    plain = DeviceTD3Target(td3_actor, c["critics"], activation=c["activation"], output="tanh")
    g = DeviceTD3Grad(plain, B)
    tp = leaves(td3_actor)
    tptrs = g._grad_pointers("actor", tp, g._shapes["actor"], "the actor's")
    assert lib.fleet_sac_actor_grad_dev(g.h, C.byref(args()), tptrs, len(tp)) == _capi.ERR_INVALID
    msg = lib.fleet_td3_last_error(g.h).decode()
    assert msg.startswith("fleet_sac_actor_grad_dev: ") and "not a squashed Gaussian" in msg and "fleet_td3_actor_grad_dev" in msg
    # ... and the TD3 entry still refuses the squashed networks
    with pytest.raises(FleetHipError, match="its gradient is not this entry's"):
        DeviceTD3Grad.actor_grad(rig.grad, x, into=rig.actor_params)
    g.close(), plain.close(), rig.close()


# ---- 6. the whole gradient step ------------------------------------------------------------------------------------------------------
STEP_SHAPES = {"7-64-64-A5-relu": dict(D=7, A=5, hidden=(64, 64), activation="relu", n_critics=2, B=33, learned=True, given=False, bias=None),
               "131-130-70-A65-tanh": dict(D=131, A=65, hidden=(130, 70), activation="tanh", n_critics=2, B=17, learned=True, given=False, bias=-1.0)}
N_STEPS, GAMMA, TAU, LR, TARGET_SEED = 4, 0.99, 0.005, 3e-4, 0x7A26E70000000777


def _steps_on_the_device(shape, salt):
    """N_STEPS of `gradient_step` under `salt`, and the two references on the device's own draws: (handles, got, ref, margins)."""
    from fleetrl_amd import DeviceAdam, DeviceSACGrad, DeviceSACNetworks
    from fleetrl_amd.sac import gradient_step

    spec = STEP_SHAPES[shape]
    c = gm.make(shape, salt, spec)
    D, A, B = c["D"], c["A"], c["B"]
    rng = np.random.default_rng(gm.seed(shape, 1000 + salt))
    t_critics = [[(w + 0.01 * rng.standard_normal(w.shape).astype(np.float32), b) for w, b in net] for net in c["critics"]]
    batches = [(np.clip(rng.standard_normal((B, D)), -3, 3).astype(np.float32), rng.uniform(-1, 1, (B, A)).astype(np.float32),
                np.clip(rng.standard_normal((B, D)), -3, 3).astype(np.float32), (rng.random(B) < 0.2).astype(np.float32),
                rng.standard_normal(B).astype(np.float32)) for _ in range(N_STEPS)]
    nets = DeviceSACNetworks(c["actor"], c["critics"], activation=c["activation"])
    targets = DeviceSACNetworks(c["actor"], t_critics, activation=c["activation"])
    grad = DeviceSACGrad(nets, B)
    pa, pc = leaves(c["actor"]), [p for net in c["critics"] for p in leaves(net)]
    log_ent_coef = torch.full((1,), c["log_ent_coef"], device=dev(), requires_grad=True)
    opt_a, opt_c = DeviceAdam(nets, pa, nets="actor", lr=LR), DeviceAdam(nets, pc, nets="critic", lr=LR)
    opt_e = DeviceAdam(nets, [log_ent_coef], nets="none", lr=LR)
    alpha = torch.empty(1, device=dev())
    noise, target_noise = [], []
    for u, b in enumerate(batches):
        obs, actions, next_obs, dones, rewards = (on_device(v) for v in b)
        e_pi, e_t = torch.empty((B, A), device=dev()), torch.empty((B, A), device=dev())
        nets.act(obs, seed=SEED, step=u, noise=e_pi)  # the draws of this step: keyed by (seed, row, step, column) alone
        nets.act(next_obs, seed=TARGET_SEED, step=u, noise=e_t)
        noise.append(host(e_pi)), target_noise.append(host(e_t))
        batch = types.SimpleNamespace(observations=obs, actions=actions, next_observations=next_obs, dones=dones, rewards=rewards)
        gradient_step(nets, targets, grad, opt_a, opt_c, batch, pa, pc, gamma=GAMMA, tau=TAU, seed=SEED, target_seed=TARGET_SEED, step=u,
                      log_ent_coef=log_ent_coef, ent_adam=opt_e, alpha_out=alpha)
    torch.cuda.synchronize()
    kw = dict(activation=c["activation"], gamma=GAMMA, tau=TAU, lr=LR, log_ent_coef=c["log_ent_coef"])
    ref = {dt: gm.sac_gradient_steps(c["actor"], c["critics"], c["actor"], t_critics, batches, noise, target_noise, dtype=dt, **kw)
           for dt in ("float64", "float32")}
    margins = gm.ur.kink_margins(ref["float64"]["kinks"], ref["float32"]["kinks"])
    handles = dict(nets=nets, targets=targets, grad=grad, opt_a=opt_a, opt_c=opt_c, opt_e=opt_e)
    return handles, dict(pa=pa, pc=pc, log_ent_coef=log_ent_coef, alpha=alpha), ref, margins


@pytest.mark.parametrize("shape", sorted(STEP_SHAPES))
def test_gradient_step_follows_sb3s_loop_under_autograd_and_torchs_adam(shape):
    """4 steps of `gradient_step` with a learned alpha: every parameter, target and Adam moment within the bound of the autograd
    reference stepping torch.optim.Adam, on the noise the device drew (recorded under the same keys by `act`); step counts exact.
    Condition (a) is asked of the run that is judged -- every ReLU pre-activation, log_std against its bounds and q_0 against q_1 of
    all four steps: a salt that misses it is not judged and the next one is taken."""
    for salt in range(gm.MAX_SALT):
        handles, t, ref, margins = _steps_on_the_device(shape, salt)
        if all(dist >= gm.KINK_FACTOR * devi for dist, devi in margins.values()):
            break
        print(f"{shape}: salt {salt} misses condition (a): {margins}: the next salt")
        for h in ("opt_e", "opt_c", "opt_a", "grad", "targets", "nets"):
            handles[h].close()
    else:
        raise AssertionError(f"{shape}: no salt below {gm.MAX_SALT} meets condition (a)")
    nets, targets, opt_a, opt_c, opt_e = (handles[k] for k in ("nets", "targets", "opt_a", "opt_c", "opt_e"))
    pa, pc, log_ent_coef, alpha = t["pa"], t["pc"], t["log_ent_coef"], t["alpha"]
    shapes = [tuple(s) for pair in nets._shapes for s in pair]
    tgt = targets.export_torch([torch.empty(s, device=dev()) for s in shapes])
    got = {"actor": pa, "critics": pc, "target_actor": tgt[:len(pa)], "target_critics": tgt[len(pa):], "log_ent_coef": [log_ent_coef]}
    states = {"actor_opt": opt_a.state_dict(), "critic_opt": opt_c.state_dict(), "ent_opt": opt_e.state_dict()}
    worst = {}
    for k, tensors in got.items():
        worst[k] = max(gm.ratio(host(t), a, b) for t, a, b in zip(tensors, ref["float64"][k], ref["float32"][k]))
    for k, sd in states.items():
        assert {int(float(s["step"])) for s in sd["state"].values()} == {N_STEPS} == {ref["float64"][k]["step"]}
        for mom in ("exp_avg", "exp_avg_sq"):
            worst[f"{k}.{mom}"] = max(gm.ratio(host(sd["state"][i][mom]), a, b)
                                      for i, (a, b) in enumerate(zip(ref["float64"][k][mom], ref["float32"][k][mom])))
    print(f"{shape}: salt {salt}, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    _parity["gradient_step/" + shape] = {"salt": salt, **{k: round(float(v), 4) for k, v in worst.items()}}
    write_parity()
    assert all(v <= 1.0 for v in worst.values()), worst
    assert abs(float(alpha[0]) - ref["float64"]["stats"]["alphas"][-1]) <= 1e-6 * ref["float64"]["stats"]["alphas"][-1]
    for h in ("opt_e", "opt_c", "opt_a", "grad", "targets", "nets"):
        handles[h].close()


# ---- 7. the example ------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_with_check():
    env = dict(os.environ, PYTHONPATH=gm.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(gm.ROOT, "examples", "sac_device_grad.py"), "--steps", "8", "--batch", "33", "--check"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines and "check" in lines[-1] and lines[-1]["check"]["max_relative_difference"] < 1e-3 and lines[-1]["backward_calls"] == 0
