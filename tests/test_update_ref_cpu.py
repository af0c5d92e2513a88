"""The end-to-end update reference (tests/sb3_update_ref.py) and its cases (tests/update_cases.py) on the CPU: every case meets the
conditions under which the device may be held to it, every deliberate misreading of SB3 lies outside the bound, and the reference's
float64 gradients of one minibatch are those of the expressions the project already trusts."""
import numpy as np
import pytest

import ppo_model as ppm
import td3_model as t3m
import update_cases as uc

torch = pytest.importorskip("torch")

CASES = [(f, n) for f, (table, _, _, _) in uc.FAMILIES.items() for n in table]


@pytest.mark.parametrize("family,name", CASES)
def test_every_case_meets_the_conditions(family, name):
    c = uc.case(family, name)
    cond = c["checked"]["conditions"]
    print(f"{family}/{name}: salt {c['salt']}")
    for kind, (dist, dev) in cond["kinks"].items():
        print(f"  kink {kind}: smallest float64 distance {dist:.3g}, largest float32 deviation {dev:.3g}, margin {dist / dev if dev else np.inf:.3g}")
        assert dist >= uc.KINK_MARGIN * dev, kind  # (a)
    print("  second float32 evaluation, error / bound:", {k: round(v, 3) for k, v in cond["b"].items()})
    assert all(v <= 1.0 for v in cond["b"].values())  # (b)
    print("  means of signed terms, bound / one rounding of a typical term:", {k: float(f"{v:.3g}") for k, v in cond["d"].items()})
    assert all(v >= 1.0 for v in cond["d"].values())  # (d)
    assert set(cond["d"]) == {"ppo": {"policy_gradient_loss", "approx_kl_all_epochs"} | ({"approx_kl", "last_approx_kl"} if name == "target-kl" else set()),
                              "td3": set() if name == "no-actor-step" else {"actor_loss", "last_actor_loss"}, "sac": set()}[family]
    if family == "ppo" and name == "target-kl":
        r64, r32 = c["checked"]["ref64"], c["checked"]["ref32"]
        print(f"  target_kl {c['kw']['target_kl']:.6g}: stop at {r64['stop']}, smallest relative distance {cond['c']:.3g}")
        assert cond["c"] >= uc.KL_MARGIN  # (c)
        assert r64["stop"] == r32["stop"] == c["stop"] and c["stop"][0] == 1 and c["stop"][1] >= 1
        steps = len(c["epochs"][0]) + c["stop"][1]
        assert r64["step"] == r32["step"] == steps and r64["stats"]["n_updates"] == 2 and r64["stats"]["minibatches"] == steps + 1
    else:
        assert cond["c"] is None
    if family == "ppo":
        assert 1 <= c["checked"]["ref64"]["step"] <= 10
        assert set(cond["kinks"]) >= {"ratio_clip", "surrogates", "grad_norm"} and ("relu" in cond["kinks"]) == (c["activation"] == "relu")
        assert ("value_clip" in cond["kinks"]) == (name == "value-clipped")
    elif family == "td3":
        r = c["checked"]["ref64"]
        assert uc.td3_exact(r) == uc.td3_exact(c["checked"]["ref32"])
        assert r["critic_opt"]["step"] == c["call"]["G"] <= 10 and r["actor_opt"]["step"] == len(uc.om.actor_steps(0, c["call"]["G"], c["call"]["delay"]))
        assert (name == "no-actor-step") == (r["actor_opt"]["step"] == 0)
    else:
        assert c["checked"]["ref64"]["critic_opt"]["step"] == uc.SAC_STEPS


MUTANTS = [("ppo", "base", "advantage_over_buffer"), ("ppo", "target-kl", "kl_stop_after_step"), ("ppo", "value-clipped", "vclip_around_new"),
           ("td3", "base", "stale_critic_in_actor_loss"), ("td3", "base", "polyak_every_step"), ("td3", "base", "u_mod_delay"),
           ("td3", "seam", "stale_critic_in_actor_loss"), ("td3", "seam", "polyak_every_step"), ("td3", "seam", "u_mod_delay"),
           ("sac", "7-64-64-a5", "no_half"), ("sac", "7-64-64-a5", "next_action_from_target_actor"),
           ("sac", "131-130-70-a65", "no_half"), ("sac", "131-130-70-a65", "next_action_from_target_actor")]


@pytest.mark.parametrize("family,name,mutant", MUTANTS)
def test_every_mutant_lies_outside_the_bound(family, name, mutant):
    """The mutant in float64 against the case's float64 reference, under the bound the device is held to."""
    _, _, run, classes = uc.FAMILIES[family]
    c = uc.case(family, name)
    got = uc.ratios(classes(run(c, torch.float64, mutant=mutant)), classes(c["checked"]["ref64"]), classes(c["checked"]["ref32"]))
    print(f"{family}/{name} {mutant}: error / bound", {k: float(f"{v:.3g}") for k, v in got.items()})
    assert max(got.values()) > 1.0


def test_the_mutants_are_all_there():
    assert {m for _, _, m in MUTANTS} == {m for ms in uc.ref.MUTANTS.values() for m in ms}


def close64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)


def test_one_ppo_minibatch_has_the_gradients_of_the_projects_restatement():
    """lr = 0 keeps the float32 weights; without normalisation the advantages are the buffer's float32 values: the first minibatch's
    float64 gradients against ppo_model.torch_loss_and_grads on the same rows."""
    c = uc.case("ppo", "normalisation-off")
    r = uc.ppo_run(c, torch.float64, lr=0.0, record_grads=True)
    b, kw = c["buffer"], c["kw"]
    for m, idx in enumerate(c["epochs"][0][:2]):
        want = ppm.torch_loss_and_grads(c["actor"], c["critic"], c["activation"], c["log_std"], b["obs"][idx], b["actions"][idx], b["log_prob"][idx],
                                        b["advantages"][idx], b["returns"][idx], kw["clip_range"], kw["vf_coef"], kw["ent_coef"])
        assert len(want["grads"]) == len(r["grads"][m]) and all(close64(g, w) for g, w in zip(r["grads"][m], want["grads"]))
    assert np.isclose(r["stats"]["loss"], r["stats"]["loss"])


def test_one_td3_step_has_the_gradients_of_the_projects_restatement():
    """lr = 0 keeps the float32 weights and gamma = 0 makes the target the float32 reward: the first step's float64 critic and actor
    gradients against td3_model.torch_critic_loss_and_grads and torch_actor_loss_and_grads."""
    for name in ("base", "ddpg"):
        c = uc.case("td3", name)
        r = uc.td3_run(c, torch.float64, lr=0.0, gamma=0.0, policy_delay=1, record_grads=True)
        obs, actions, _, _, rewards = c["batches"][0]
        g = r["grads"][0]
        assert np.array_equal(g["target_q"], rewards)
        want = t3m.torch_critic_loss_and_grads(c["critics"], c["kw"]["activation"], obs, actions, rewards)
        assert len(want["grads"]) == len(g["critic"]) and all(close64(x, w) for x, w in zip(g["critic"], want["grads"]))
        want = t3m.torch_actor_loss_and_grads(c["actor"], c["critics"], c["kw"]["activation"], "tanh", -1.0, 1.0, obs)
        assert len(want["grads"]) == len(g["actor"]) and all(close64(x, w) for x, w in zip(g["actor"], want["grads"]))
