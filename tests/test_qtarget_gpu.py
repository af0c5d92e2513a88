"""The TD3 / DDPG targets on the device (fleet_qtarget.hip) against the bit model of tests/qtarget_model.py, against the launches this
project already pins (DevicePolicy.explore / act), against torch's own expression, and the Polyak update against its model."""
import json
import os

import numpy as np
import pytest

import explore_model as em
import policy_bits as pb
import policy_model as pm
import qtarget_model as qm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(pm.ROOT, "profiles", "qtarget_parity.json")
f32 = np.float32


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


def make_target(actor, critics, activation="relu", output="clip", low=qm.ACTOR_CLIP[0], high=qm.ACTOR_CLIP[1]):
    from fleetrl_amd import DeviceTD3Target

    return DeviceTD3Target(actor, critics, activation=activation, output=output, low=low, high=high)


def run(tgt, inp, B, *, first=0, noise_given=True, noise=None, outputs=True, sigma=qm.SIGMA, noise_clip=qm.NOISE_CLIP, bounds=qm.ACTION_BOUNDS,
        seed=1, step=0, row_offset=0):
    """One launch on rows first .. first + B of the case's inputs -> {"y", "q", "next_actions", "noise"} as host arrays."""
    sl = slice(first, first + B)
    x, r, d = (on_device(inp[k][sl]) for k in ("next_obs", "rewards", "dones"))
    if noise is None:
        noise = on_device(inp["eps"][sl]) if noise_given else torch.full((B, tgt.act_dim), np.nan, device=dev())
    na = torch.full((B, tgt.act_dim), np.nan, device=dev()) if outputs else None
    q = torch.full((B, tgt.n_critics), np.nan, device=dev()) if outputs else None
    y = tgt.target(x, r, d, gamma=qm.GAMMA, sigma=sigma, noise_clip=noise_clip, low=bounds[0], high=bounds[1], seed=seed, step=step,
                   row_offset=row_offset, next_actions_out=na, q_out=q, noise=noise if (noise_given or outputs) else None,
                   noise_given=noise_given)
    return {"y": host(y), "q": None if q is None else host(q), "next_actions": None if na is None else host(na), "noise": host(noise)}


# ---- 1. the bit model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(qm.CASES))
def test_target_equals_the_model_bit_for_bit(name):
    facts = qm.facts(name)
    assert all(facts.values()), facts  # each critic wins somewhere, both clips bite somewhere and not everywhere, dones 0 and 1
    actor, critics = qm.network(name)
    want, inp = qm.model(name), qm.inputs(name)
    tgt = make_target(actor, critics)
    for B in qm.BATCHES:
        got = run(tgt, inp, B)
        for k in ("next_actions", "q", "y"):
            assert pb.same_bits(got[k], want[k][:B]), (name, B, k)
    tgt.close()


# ---- 2. composition with the launches already pinned ------------------------------------------------------------------------------
@pytest.mark.parametrize("activation,output,name", qm.COMPOSE)
def test_target_is_the_composition_of_explore_act_and_torchs_expression(activation, output, name):
    from fleetrl_amd import DevicePolicy

    actor, critics = qm.network(name)
    inp = qm.inputs(name)
    tgt = make_target(actor, critics, activation, output)
    got = run(tgt, inp, qm.ROWS, noise_clip=float("inf"))
    x, eps = on_device(inp["next_obs"]), on_device(inp["eps"])
    pol = DevicePolicy(actor, activation=activation, output=output, low=qm.ACTOR_CLIP[0], high=qm.ACTOR_CLIP[1])
    a, _, _, _ = pol.explore(x, qm.SIGMA, low=qm.ACTION_BOUNDS[0], high=qm.ACTION_BOUNDS[1], seed=0, step=0, noise=eps, noise_given=True)
    assert pb.same_bits(got["next_actions"], host(a))
    xa = torch.cat([x, a], dim=1).contiguous()
    qs = []
    for c, layers in enumerate(critics):
        cp = DevicePolicy(layers, activation=activation, output="none")
        qs.append(cp.act(xa))
        assert pb.same_bits(got["q"][:, c], host(qs[-1])[:, 0]), c
        cp.close()
    qmin = torch.min(qs[0], qs[1]) if len(qs) == 2 else qs[0]
    r, d = on_device(inp["rewards"]), on_device(inp["dones"])
    y = r + ((1 - d) * f32(qm.GAMMA)) * qmin[:, 0]
    assert y.dtype == torch.float32 and pb.same_bits(got["y"], host(y))
    pol.close()
    tgt.close()


# ---- 3. drawn noise; what a row does not depend on --------------------------------------------------------------------------------
@pytest.mark.parametrize("A,seed,step,offset", [(1, 3, 0, 0), (5, em.SEED, 2 ** 32 + 7, 100), (65, (1 << 63) | 12345, 2 ** 32 - 1, 2 ** 31 - 40)])
def test_recorded_noise_equals_what_explore_records(A, seed, step, offset):
    from fleetrl_amd import DevicePolicy

    rng = np.random.default_rng(A)
    D, B = 9, 37
    actor, critic = pm.random_layers(rng, (D, 20, A)), pm.random_layers(rng, (D + A, 1))
    x = on_device(rng.standard_normal((B, D)).astype(np.float32))
    tgt = make_target(actor, [critic])
    noise = torch.full((B, A), np.nan, device=dev())
    tgt.target(x, torch.zeros(B, device=dev()), torch.zeros(B, device=dev()), gamma=0.99, sigma=0.2, noise_clip=0.5, seed=seed, step=step,
               row_offset=offset, noise=noise)
    pol = DevicePolicy(actor, activation="relu", output="clip")
    rec = torch.full((B, A), np.nan, device=dev())
    pol.explore(x, 0.2, seed=seed, step=step, env_id_offset=offset, noise=rec)
    assert pb.same_bits(host(noise), host(rec)) and np.isfinite(host(noise)).all()
    assert np.abs(host(noise).astype(np.float64) - em.normals(seed, offset + np.arange(B), A, step)).max() < 1e-5
    pol.close()
    tgt.close()


def test_a_rows_outputs_depend_on_the_row_and_on_nothing_else():
    name = qm.INVARIANCE_CASE
    actor, critics = qm.network(name)
    inp = qm.inputs(name)
    tgt = make_target(actor, critics)
    kw = dict(noise_given=False, seed=em.SEED, step=5)
    ref = run(tgt, inp, qm.ROWS, **kw)
    assert np.isfinite(ref["y"]).all() and np.isfinite(ref["noise"]).all()
    # B, and the position in the batch: rows 3 .. 16 as a batch of their own, their global ids kept
    part = run(tgt, inp, qm.ROWS - 3, first=3, row_offset=3, **kw)
    for k in ("y", "q", "next_actions", "noise"):
        assert pb.same_bits(part[k], ref[k][3:]), k
    one = run(tgt, inp, 1, first=16, row_offset=16, **kw)
    assert pb.same_bits(one["y"], ref["y"][16:])
    # the optional outputs
    bare = run(tgt, inp, qm.ROWS, outputs=False, **kw)
    assert pb.same_bits(bare["y"], ref["y"])
    # the stream
    s = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(s):
        other = run(tgt, inp, qm.ROWS, **kw)
    s.synchronize()
    for k in ("y", "q", "next_actions", "noise"):
        assert pb.same_bits(other[k], ref[k]), k
    # n_critics: critic 0 alone sees the same actions and gives the same q_0
    solo = make_target(actor, critics[:1])
    alone = run(solo, inp, qm.ROWS, **kw)
    assert pb.same_bits(alone["next_actions"], ref["next_actions"]) and pb.same_bits(alone["q"][:, 0], ref["q"][:, 0])
    assert pb.same_bits(alone["noise"], ref["noise"])
    solo.close()
    tgt.close()


# ---- 4. Polyak ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", qm.POLYAK_CASES)
def test_polyak_with_tau_one_and_zero(name):
    actor, critics = qm.network(name)
    online = qm.flat_params(*qm.network(name, salt=1))
    inp = qm.inputs(name)
    tgt = make_target(actor, critics)
    before = [host(t) for t in tgt.export_torch()]
    assert all(pb.same_bits(a, b) for a, b in zip(before, qm.flat_params(actor, critics)))  # export is the inverse of the upload
    dev_online = [on_device(a) for a in online]
    tgt.polyak(dev_online, 0.0)
    assert all(pb.same_bits(host(t), b) for t, b in zip(tgt.export_torch(), before))
    tgt.polyak(dev_online, 1.0)
    assert all(pb.same_bits(host(t), b) for t, b in zip(tgt.export_torch(), online))
    after_polyak = run(tgt, inp, qm.ROWS)
    tgt.load_torch([on_device(a) for a in qm.flat_params(actor, critics)])  # away and back again through load_torch
    tgt.load_torch(dev_online)
    after_load = run(tgt, inp, qm.ROWS)
    for k in ("y", "q", "next_actions"):
        assert pb.same_bits(after_polyak[k], after_load[k]), k
    tgt.close()


@pytest.mark.parametrize("tau", [0.005, 0.37])
@pytest.mark.parametrize("name", qm.POLYAK_CASES)
def test_polyak_equals_the_model_once_and_three_times_and_keeps_the_padding_zero(name, tau):
    actor, critics = qm.network(name)
    inp = qm.inputs(name)
    tgt = make_target(actor, critics)
    want = qm.flat_params(actor, critics)
    for n in (1, 2, 3):
        online = qm.flat_params(*qm.network(name, salt=n))
        tgt.polyak([on_device(a) for a in online], tau)
        want = [qm.polyak_bits(t, p, tau) for t, p in zip(want, online)]
        if n in (1, 3):
            got = [host(t) for t in tgt.export_torch()]
            assert all(pb.same_bits(g, w) for g, w in zip(got, want)), n
    # the padded image: a target on the updated weights equals the model on them (in % 4 != 0 and out % 64 != 0 in these cases)
    it = iter(want)
    nets = [[(next(it), next(it)) for _ in net] for net in [actor] + list(critics)]
    assert any(w.shape[1] % 4 and w.shape[0] % 64 for net in nets for w, _ in net)
    m = qm.target_bits(nets[0], nets[1:], inp["next_obs"], inp["rewards"], inp["dones"], inp["eps"], qm.SIGMA, gamma=qm.GAMMA,
                       noise_clip=qm.NOISE_CLIP, low=qm.ACTION_BOUNDS[0], high=qm.ACTION_BOUNDS[1], activation="relu", output="clip",
                       actor_low=qm.ACTOR_CLIP[0], actor_high=qm.ACTOR_CLIP[1])
    got = run(tgt, inp, qm.ROWS)
    for k in ("y", "q", "next_actions"):
        assert pb.same_bits(got[k], m[k]), k
    tgt.close()


def test_polyak_and_target_refuse_with_a_reason_on_a_live_handle():
    from fleetrl_amd import FleetHipError

    name = qm.REFUSAL_CASE
    actor, critics = qm.network(name)
    tgt = make_target(actor, critics)
    params = [on_device(a) for a in qm.flat_params(actor, critics)]
    before = [host(t) for t in tgt.export_torch()]
    for tau in (-0.1, 1.5, float("nan")):
        with pytest.raises(FleetHipError, match="tau must be in"):
            tgt.polyak(params, tau)
    with pytest.raises(ValueError, match="expected 6 tensors"):
        tgt.polyak(params[:-1], 0.5)
    inp = qm.inputs(name)
    for kw, word in ((dict(noise_clip=-1.0), "noise_clip"), (dict(bounds=(0.5, -0.5)), "act_lo <= act_hi"), (dict(row_offset=-1), "row_offset")):
        with pytest.raises(FleetHipError, match=word):
            run(tgt, inp, 4, **kw)
    assert all(pb.same_bits(host(t), b) for t, b in zip(tgt.export_torch(), before))
    tgt.close()


# ---- 5. the tanh TD3 network against float64 ---------------------------------------------------------------------------------------
def _target64(actor, critics, x, r, d, eps, act, f=np.float64):
    a = np.clip(pm.forward64(actor, x, act, "tanh") + np.clip(qm.SIGMA * eps.astype(f), -qm.NOISE_CLIP, qm.NOISE_CLIP), -1.0, 1.0)
    q = np.stack([pm.forward64(c, np.concatenate([x.astype(f), a], axis=1), act, "none")[:, 0] for c in critics], axis=1)
    return a, q, r.astype(f) + (1.0 - d.astype(f)) * qm.GAMMA * q.min(axis=1)


def _target_torch32(actor, critics, x, r, d, eps, act):
    a = pm.forward_torch32(actor, x, act, "tanh")
    a = np.clip(a + np.clip(f32(qm.SIGMA) * eps, -f32(qm.NOISE_CLIP), f32(qm.NOISE_CLIP)), f32(-1), f32(1)).astype(np.float32)
    q = np.stack([pm.forward_torch32(c, np.concatenate([x, a], axis=1), act, "none")[:, 0] for c in critics], axis=1)
    return a, q, (r + ((f32(1) - d) * f32(qm.GAMMA)) * q.min(axis=1)).astype(np.float32)


@pytest.mark.parametrize("activation", ["tanh", "relu"])
def test_td3_network_stays_within_eight_times_the_float32_reference_error(activation):
    """388-400-300-50 (tanh hidden layers, and SB3's ReLU; tanh output) with twin 438-400-300-1 critics against a float64 model: the device's error is at most
    8 * max(eps_ref, 2^-24 * max |out|), eps_ref torch-CPU float32's distance from the same model."""
    rng = np.random.default_rng(388)
    B, D, A = 64, 388, 50
    actor = pm.random_layers(rng, (D, 400, 300, A))
    critics = [pm.random_layers(rng, (D + A, 400, 300, 1)) for _ in range(2)]
    inp = {"next_obs": np.clip(rng.standard_normal((B, D)) * 3, -10, 10).astype(np.float32), "rewards": rng.standard_normal(B).astype(np.float32),
           "dones": (np.arange(B) % 2).astype(np.float32), "eps": rng.standard_normal((B, A)).astype(np.float32)}
    tgt = make_target(actor, critics, activation, "tanh")
    got = run(tgt, inp, B, bounds=(-1.0, 1.0))
    ref = dict(zip(("next_actions", "q", "y"), _target64(actor, critics, *(inp[k] for k in ("next_obs", "rewards", "dones", "eps")), activation)))
    t32 = dict(zip(("next_actions", "q", "y"), _target_torch32(actor, critics, *(inp[k] for k in ("next_obs", "rewards", "dones", "eps")), activation)))
    figures, bad = {}, []
    for k in ("next_actions", "q", "y"):
        eps_ref = float(np.abs(t32[k].astype(np.float64) - ref[k]).max())
        err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        bound = 8 * max(eps_ref, 2.0 ** -24 * float(np.abs(ref[k]).max()))
        figures[f"td3-388-400-300-50-{activation}/{k}/B{B}"] = {"eps_ref": eps_ref, "device_err": err, "bound": bound, "err_over_bound": err / bound}
        print(f"{k}: eps_ref {eps_ref:.3g} device {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
        if not err <= bound:
            bad.append(k)
    if os.environ.get("FLEET_WRITE_PARITY") == "1":  # (a test run leaves the tree as it found it)
        cases = {}
        if os.path.exists(PARITY_FILE):
            with open(PARITY_FILE) as fh:
                cases = json.load(fh).get("cases", {})
        cases.update(figures)
        os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
        with open(PARITY_FILE, "w") as fh:
            json.dump({"bound": "8 * max(eps_ref, 2^-24 * max|out|)", "cases": dict(sorted(cases.items()))}, fh, indent=1)
            fh.write("\n")
    assert not bad, (bad, figures)
    tgt.close()


# ---- 6. a row that is not finite ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_value_that_is_not_finite_stays_in_its_row(value):
    name = qm.HOSTILE_CASE
    actor, critics = qm.network(name)
    inp = {k: np.array(v) for k, v in qm.inputs(name).items()}
    want = qm.model(name)
    inp["next_obs"][7, 100] = value
    tgt = make_target(actor, critics)
    got = run(tgt, inp, qm.ROWS)
    others = np.arange(qm.ROWS) != 7
    for k in ("y", "q", "next_actions"):
        assert pb.same_bits(got[k][others], want[k][others]), k
    assert np.isnan(got["q"][7]).all()  # (a hidden layer's padded columns meet the value: the policy section's words)
    tgt.close()


def test_describe_and_from_state_dict():
    from fleetrl_amd import DeviceTD3Target

    name = qm.DESCRIBE_CASE
    actor, critics = qm.network(name)
    sd = {}
    for prefix, net in [("actor_target.mu", actor)] + [(f"critic_target.qf{c}", n) for c, n in enumerate(critics)]:
        for i, (w, b) in enumerate(net):
            sd[f"{prefix}.{2 * i}.weight"], sd[f"{prefix}.{2 * i}.bias"] = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
    tgt = DeviceTD3Target.from_state_dict(sd, output="clip", low=qm.ACTOR_CLIP[0], high=qm.ACTOR_CLIP[1])
    d = tgt.describe()
    assert (d["obs_dim"], d["act_dim"], d["n_critics"], d["tile_rows"]) == (5, 3, 2, 16)
    assert d["actor"]["widths"] == [70, 3] and d["critics"][1]["widths"] == [65, 63, 1] and d["critics"][0]["output"] == "none"
    got, want = run(tgt, qm.inputs(name), qm.ROWS), qm.model(name)
    assert pb.same_bits(got["y"], want["y"])
    tgt.close()
