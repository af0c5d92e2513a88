"""The one-call updates against SB3's loops as plain torch autograd (tests/sb3_update_ref.py) at the cases of tests/update_cases.py:
`DevicePPOTrain.train` (with clip_range_vf and target_kl), `DeviceTD3Train.train` (TD3 and DDPG) and the critic half of a SAC step
through `fleetrl_amd.sac.critic_update` and `polyak`.  Per case the call runs once, everything is read back, and ref64 and ref32 run on
the CPU from the same initial weights and buffer contents, the same rows (train_model.indices, replay_model.draw) and -- for TD3 and
SAC -- the noise the device itself drew, recorded on twin handles under the same seed, step and rows.  Every online and target
parameter, both optimisers' moments and the statistics are held to |device - ref64| <= 8 max(|ref32 - ref64|, 2^-24 max|ref64|) per
tensor; the counts are compared exactly.  The figures go to profiles/update_ref_parity.json (with FLEET_WRITE_PARITY=1)."""
import json
import os

import numpy as np
import pytest

import offpolicy_model as om
import train_model as tm
import update_cases as uc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
PARITY_FILE = os.path.join(tm.ROOT, "profiles", "update_ref_parity.json")
_parity = {}


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy().copy()


def write_parity():
    """The figures are printed; they go to the file only when FLEET_WRITE_PARITY=1 asks for it, merged into the cases it holds."""
    if os.environ.get("FLEET_WRITE_PARITY") != "1":
        return
    cases = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as fh:
            cases = json.load(fh).get("cases", {})
    cases.update(_parity)
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as fh:
        json.dump({"bound": "8 * max(max|ref32 - ref64|, 2^-24 * max|ref64|) per tensor; the figures are error / bound",
                   "cases": dict(sorted(cases.items()))}, fh, indent=1)
        fh.write("\n")


def judge(tag, got, checked, exact_got, exact_want):
    """Print and record every class's error / bound, then assert: the conditions of this very run, the counts, the bound."""
    r = uc.ratios(got, *(checked[k] for k in ("ref64_classes", "ref32_classes")))
    cond = checked["conditions"]
    print(tag, "error / bound", {k: float(f"{v:.3g}") for k, v in r.items()}, "exact", exact_got, "reference", exact_want)
    print(tag, "kinks (distance, deviation)", {k: (float(f"{a:.3g}"), float(f"{b:.3g}")) for k, (a, b) in cond["kinks"].items()})
    _parity[tag] = {k: float(f"{v:.4g}") for k, v in r.items()}
    write_parity()
    for k in (k for k, v in r.items() if v > 1.0):  # what lies outside, tensor by tensor: value, reference, float32 reference's error
        for i, (g, a, b) in enumerate(zip(got[k], checked["ref64_classes"][k], checked["ref32_classes"][k])):
            g, a, b = (np.asarray(x, np.float64) for x in (g, a, b))
            print(f"  {tag} {k}[{i}] shape {g.shape}: error / bound {uc.ratio(g, a, b):.3g}, max|error| {np.abs(g - a).max():.3g}, "
                  f"eps_ref {np.abs(b - a).max():.3g}, max|ref64| {np.abs(a).max():.3g}" + (f", device {g!r}, ref64 {a!r}" if g.ndim == 0 else ""))
    assert cond["ok"], cond  # the conditions hold for the inputs of this run too (the noise is the device's)
    assert tuple(exact_got) == tuple(exact_want)
    assert all(v <= 1.0 for v in r.values()), r
    return r


def with_classes(family, checked):
    classes = uc.FAMILIES[family][3]
    return {**checked, "ref64_classes": classes(checked["ref64"]), "ref32_classes": classes(checked["ref32"])}


# ---- PPO -------------------------------------------------------------------------------------------------------------------------------
class PPORig:
    """The handles of tests/test_ppo_train_gpu.py's Rig on a case's networks, with the case's rollout in the buffer."""

    def __init__(self, c):
        from fleetrl_amd import DeviceAdam, DevicePolicy, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer

        kw = c["kw"]
        self.pol = DevicePolicy(c["actor"], critic_layers=c["critic"], activation=c["activation"], output="clip")
        self.params = [torch.nn.Parameter(on_device(t)) for net in (c["actor"], c["critic"]) for w, b in net for t in (w, b)] + \
                      [torch.nn.Parameter(on_device(c["log_std"]))]
        self.buf = DeviceRolloutBuffer(c["E"], c["K"], c["D"], c["A"])
        for name, a in c["rollout"].items():
            getattr(self.buf, name).copy_(on_device(a))
        self.buf.pos, self.buf.full = c["K"], True
        self.grad = DevicePPOGrad(self.pol, -(-c["batch_size"] // 16) * 16)
        self.adam = DeviceAdam(self.pol, self.params, lr=kw["lr"], eps=kw["adam_eps"], max_grad_norm=kw["max_grad_norm"])
        self.train = DevicePPOTrain(self.buf, self.grad, self.adam)
        torch.cuda.synchronize()

    def close(self):
        for h in (self.train, self.adam, self.grad, self.buf, self.pol):
            h.close()


@pytest.mark.parametrize("name", sorted(uc.PPO_CASES))
def test_ppo_train_against_sb3s_loop_under_autograd(name):
    c = uc.case("ppo", name)
    print(f"ppo/{name}: salt {c['salt']}")
    kw = c["kw"]
    rig = PPORig(c)
    stats = host(rig.train.train(rig.params, n_epochs=c["n_epochs"], batch_size=c["batch_size"], clip_range=kw["clip_range"],
                                 vf_coef=kw["vf_coef"], ent_coef=kw["ent_coef"], lr=kw["lr"], normalize_advantage=kw.get("normalize_advantage", True),
                                 seed=c["seed"], first_epoch=0, clip_range_vf=kw.get("clip_range_vf"), target_kl=kw.get("target_kl")))
    sd = rig.adam.state_dict()["state"]
    s = dict(zip(tm.STATS, stats))
    got = {"params": [host(p) for p in rig.params], "exp_avg": [host(sd[i]["exp_avg"]) for i in range(len(sd))],
           "exp_avg_sq": [host(sd[i]["exp_avg_sq"]) for i in range(len(sd))],
           "stats": [s[k] for k in ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss", "explained_variance", "std")]}
    image = [host(t) for t in rig.adam.export_image()]
    assert all(np.array_equal(p, i) for p, i in zip(got["params"][:-1], image))  # the policy's image holds the parameters
    step, count = rig.adam.describe()["step"], int(s["n_updates"])
    r64 = c["checked"]["ref64"]
    per_epoch = len(c["epochs"][0])
    if kw.get("target_kl") is None:
        # the block's [6] counts minibatches; SB3's `_n_updates` counts epochs: n_epochs here, since nothing stops the update
        exact, want = (step, count, c["n_epochs"], None), uc.ppo_exact(r64)
    else:
        k = dict(zip(("n_steps", "n_epochs", "early_stop", "last_approx_kl", "epoch_approx_kl"), stats[9:14]))
        # the stopping minibatch: the last one counted; no optimiser step was taken at it, and no epoch entered after it
        stopped = ((count - 1) // per_epoch, (count - 1) % per_epoch) if k["early_stop"] == 1.0 else None
        assert k["n_steps"] == step == count - 1
        exact, want = (step, count, int(k["n_epochs"]), stopped), uc.ppo_exact(r64)
    checked = with_classes("ppo", c["checked"])
    if kw.get("target_kl") is not None:  # two more statistics: the approx_kl compared last, and SB3's train/approx_kl (the last epoch's mean)
        got["stats"] = got["stats"] + [k["last_approx_kl"], k["epoch_approx_kl"]]
        for which in ("ref64", "ref32"):
            checked[which + "_classes"]["stats"] = checked[which + "_classes"]["stats"] + [checked[which]["stats"][x] for x in ("last_approx_kl", "approx_kl")]
    judge(f"ppo/{name}", got, checked, exact, want)
    rig.buf.check_errors()
    rig.close()


# ---- TD3 / DDPG ------------------------------------------------------------------------------------------------------------------------
def td3_stack(c):
    """An offpolicy_model.Stack of the case; with a normaliser, the case's statistics in it and what it then exports."""
    from fleetrl_amd.vec_normalize import RunningStats

    s = om.Stack(**c["stack"])
    stats = None
    if c["norm"] is not None:
        s.env.set_state(obs_rms=RunningStats(c["norm"]["obs_mean"], c["norm"]["obs_var"], 100.0),
                        ret_rms=RunningStats(np.float64(0.0), np.float64(c["norm"]["ret_var"]), 100.0))
        st = s.env.get_state()
        stats = {"obs_mean": st.obs_rms.mean, "obs_var": st.obs_rms.var, "ret_var": float(st.ret_rms.var)}
    return s, stats


def td3_noise(twin, c):
    """The target-smoothing draws of the call's steps, recorded on a twin's target handle: the noise is keyed by (seed, row, step =
    first_update + g, column) and by nothing else."""
    call, D = c["call"], c["shape"]["D"]
    zero = lambda *shape: torch.zeros(shape, device=dev())  # noqa: E731
    out = []
    for g in range(call["G"]):
        eps = zero(call["B"], c["shape"]["A"])
        twin.targets.target(zero(call["B"], D), zero(call["B"]), zero(call["B"]), gamma=uc.TD3_HYPER["gamma"], sigma=twin.sigma,
                            noise_clip=uc.TD3_HYPER["noise_clip"], seed=call["seed"], step=call["first_update"] + g, noise=eps)
        out.append(host(eps).astype(np.float64))
    return out


@pytest.mark.parametrize("name", sorted(uc.TD3_CASES))
def test_td3_train_against_sb3s_loop_under_autograd(name):
    c = uc.case("td3", name)
    print(f"td3/{name}: salt {c['salt']}")
    call, h = c["call"], uc.TD3_HYPER
    s, stats = td3_stack(c)
    twin, _ = td3_stack(c)
    assert om.same_state(s.state(), twin.state()) == []
    arrays = {k: host(getattr(s.buf, k)) for k in c["arrays"]}
    assert all(np.array_equal(arrays[k], c["arrays"][k]) for k in arrays)
    assert float(s.sigma[0]) == F32(c["kw"]["sigma"]) and s.opt_c.lr == h["lr"]
    noise = td3_noise(twin, c)
    # the draw is the one the case was chosen under (the model of the device's generator), to the bound of tests/test_explore_gpu.py
    assert c["kw"]["sigma"] == 0.0 or all(np.abs(e).max() > 0 and np.abs(e - m).max() <= 1e-5 for e, m in zip(noise, c["noise"]))
    block = host(s.one_call(G=call["G"], B=call["B"], delay=call["delay"], first_update=call["first_update"], seed=call["seed"],
                            gamma=h["gamma"], tau=h["tau"], noise_clip=h["noise_clip"]))
    st = s.state()
    batches = uc.drawn_batches(arrays, c["shape"]["seed"] + 77, 0, call["G"], call["B"], c["upper"], c["shape"]["E"], stats)
    checked = with_classes("td3", uc.check("td3", c, batches=batches, noise=noise))
    d = dict(zip(om.STATS, block))
    got = {"online": st["params"], "targets": st["target_image"], "actor_exp_avg": st["actor_m"], "actor_exp_avg_sq": st["actor_v"],
           "critic_exp_avg": st["critic_m"], "critic_exp_avg_sq": st["critic_v"], "stats": [d[k] for k in uc.TD3_STATS]}
    if not got["actor_exp_avg"]:  # an optimiser that never stepped holds no state yet: zeros, as the reference counts them
        got["actor_exp_avg"] = got["actor_exp_avg_sq"] = [np.zeros_like(p) for p in st["params"][:len(s.actor_params)]]
    assert all(np.array_equal(a, b) for a, b in zip(st["params"], st["online_image"])) and st["calls"] == call["G"]
    exact = (st["actor_step"], st["critic_step"], int(d["n_updates"]), int(d["actor_steps"]))
    judge(f"td3/{name}", got, checked, exact, uc.td3_exact(checked["ref64"]))
    s.buf.check_errors()
    s.close()
    twin.close()


# ---- the critic half of SAC ------------------------------------------------------------------------------------------------------------
class SACRig:
    def __init__(self, c):
        from fleetrl_amd import DeviceAdam, DeviceReplayBuffer, DeviceSACNetworks, DeviceTD3Grad

        act = c["kw"]["activation"]
        self.nets = DeviceSACNetworks(c["actor"], c["critics"], activation=act)
        self.targets = DeviceSACNetworks(c["target_actor"], c["target_critics"], activation=act)
        self.actor_params = [on_device(t) for w, b in c["actor"] for t in (w, b)]
        self.critic_params = [torch.nn.Parameter(on_device(t)) for net in c["critics"] for w, b in net for t in (w, b)]
        self.grad = DeviceTD3Grad(self.nets, 32)
        self.opt = DeviceAdam(self.nets, self.critic_params, nets="critic", lr=c["kw"]["lr"])
        self.buf = DeviceReplayBuffer(uc.SAC_R * uc.SAC_E, uc.SAC_E, c["D"], c["A"], seed=c["buffer_seed"])
        for k, a in c["arrays"].items():
            getattr(self.buf, k).copy_(on_device(a))
        self.buf.set_position(0, True, 0)
        torch.cuda.synchronize()

    def close(self):
        for h in (self.opt, self.grad, self.targets, self.nets, self.buf):
            h.close()


@pytest.mark.parametrize("name", sorted(uc.SAC_CASES))
def test_the_sac_critic_half_against_sb3s_loop_under_autograd(name):
    from fleetrl_amd.sac import CRITIC_LOSS_SCALE, critic_update

    c = uc.case("sac", name)
    print(f"sac/{name}: salt {c['salt']}")
    kw = c["kw"]
    rig, twin = SACRig(c), SACRig(c)
    zero = lambda *shape: torch.zeros(shape, device=dev())  # noqa: E731
    noise, losses, stats = [], [], zero(8)
    for u in range(uc.SAC_STEPS):
        eps = zero(uc.SAC_B, c["A"])  # the draw of this step, recorded on the twin: keyed by (seed, row, step, column) alone
        twin.nets.target(twin.targets, zero(uc.SAC_B, c["D"]), zero(uc.SAC_B), zero(uc.SAC_B), gamma=kw["gamma"], ent_coef=kw["ent_coef"],
                         seed=uc.SAC_SEED, step=u, noise=eps)
        noise.append(host(eps).astype(np.float64))
        b = rig.buf.sample(uc.SAC_B)
        critic_update(rig.nets, rig.targets, rig.grad, rig.opt, b, rig.critic_params, gamma=kw["gamma"], ent_coef=kw["ent_coef"],
                      seed=uc.SAC_SEED, step=u, stats_out=stats)
        rig.targets.polyak(rig.actor_params + rig.critic_params, kw["tau"])
        losses.append(CRITIC_LOSS_SCALE * float(host(stats)[0]))
    assert all(np.abs(e).max() > 0 and np.abs(e - m).max() <= 1e-5 for e, m in zip(noise, c["noise"]))  # the draw the case was chosen under
    checked = with_classes("sac", uc.check("sac", c, noise=noise))
    sd = rig.opt.state_dict()["state"]
    got = {"critics": [host(p) for p in rig.critic_params], "targets": [host(t) for t in rig.targets.export_torch()],
           "critic_exp_avg": [host(sd[i]["exp_avg"]) for i in range(len(sd))], "critic_exp_avg_sq": [host(sd[i]["exp_avg_sq"]) for i in range(len(sd))],
           "stats": [float(np.mean(losses)), losses[-1]]}
    online = [host(t) for t in rig.nets.export_torch()]
    assert all(np.array_equal(a, b) for a, b in zip(online, [host(p) for p in rig.actor_params] + got["critics"]))
    judge(f"sac/{name}", got, checked, (rig.opt.describe()["step"], rig.buf.calls), (checked["ref64"]["critic_opt"]["step"], uc.SAC_STEPS))
    rig.buf.check_errors()
    rig.close()
    twin.close()
