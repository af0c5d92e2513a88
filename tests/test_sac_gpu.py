"""SAC's actor and soft targets on the device (fleet_sac_act_dev, fleet_sac_target_dev; fleet_sac.hip) against tests/sac_model.py: stage
by stage, every stage compared with the model fed the device's OWN stored outputs of the stage before; what a row may depend on; the
target against the pieces; the shared fleet_qtarget / fleet_td3 / fleet_adam entries on a squashed handle; the refusals that need
handles; the example.  Needs an MI355X."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import qtarget_model as qm
import sac_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(sm.ROOT, "profiles", "sac_parity.json")
_parity = {}
KINDS = ("one", "tanh", "relu")


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def host(t):
    return t.detach().cpu().numpy()


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def write_parity():
    """The figures are printed; they go to profiles/sac_parity.json only when FLEET_WRITE_PARITY=1 asks for it (a test run leaves the
    tree as it found it), merged into the cases the file already holds."""
    if os.environ.get("FLEET_WRITE_PARITY") != "1":
        return
    cases = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as fh:
            cases = json.load(fh).get("cases", {})
    cases.update(_parity)
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as fh:
        json.dump({"bounds": "tests/sac_model.py: u 4 ulp at max(|u|, |sd eps|); a 2.5 ulp; log_prob_bound", "cases": dict(sorted(cases.items()))},
                  fh, indent=1)
        fh.write("\n")


def case_of(i):
    """The i-th mix of trunk, observation width and batch."""
    return KINDS[i % 3], (sm.D_SMALL, sm.D_CHUNKED)[i % 2], sm.ES[i % len(sm.ES)]


def make(kind, D, A, nc=2, salt=0, log_std_bias=None):
    from fleetrl_amd import DeviceSACNetworks

    actor, critics, activation = sm.networks(kind, D, A, nc, salt, log_std_bias)
    return DeviceSACNetworks(actor, critics, activation=activation), actor, critics, activation


def full_act(nets, x, offset=0, step=11, seed=sm.SEED, normalizer=None, optional=True):
    """Every output of one launch, as tensors."""
    E, A = x.shape[0], nets.act_dim
    out = {k: torch.full((E, A), 9.0, device=dev()) for k in (("noise", "gaussian", "mean", "log_std") if optional else ())}
    lp = torch.full((E,), 9.0, device=dev()) if optional else None
    a = nets.act(x.contiguous(), seed=seed, step=step, env_id_offset=offset, normalizer=normalizer, noise=out.get("noise"),
                 gaussian_actions_out=out.get("gaussian"), log_prob_out=lp, mean_out=out.get("mean"), log_std_out=out.get("log_std"))
    out["actions"] = a
    if optional:
        out["log_prob"] = lp
    torch.cuda.synchronize()
    return out


# ---- 1. the heads, the clamp, the draw ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,A", list(enumerate(sm.ACTS)))
def test_the_heads_are_the_policy_forward_and_the_clamp_is_exact(i, A):
    """mean and the unclamped log_std head bit-equal to DevicePolicy.act over the same 2A-wide chain; the bias of the log_std rows
    pushes l beyond both -20 and 2."""
    from fleetrl_amd import DevicePolicy

    kind, D, E = case_of(i)
    push = np.resize(np.array([-30.0, 5.0, 0.0, -19.5, 1.5], np.float32), A)
    nets, actor, _, activation = make(kind, D, A, log_std_bias=push)
    pol = DevicePolicy(actor, activation=activation, output="none")
    x = on_device(sm.observations(E, D))
    heads = pol.act(x)
    got = full_act(nets, x)
    raw = host(heads)[:, A:]
    assert np.array_equal(bits(got["mean"]), bits(heads[:, :A]))
    assert np.array_equal(bits(got["log_std"]), sm.clamp_log_std32(raw).view(np.int32))
    assert (raw < -20).any() and (host(got["log_std"]) == -20).any()
    if A > 1:
        assert (raw > 2).any() and (host(got["log_std"]) == 2).any()
    nets.close(), pol.close()


@pytest.mark.parametrize("i,A", list(enumerate(sm.ACTS)))
def test_the_recorded_draw_is_the_exploration_draw(i, A):
    """The noise `act` records is the noise DevicePolicy.sample records for the same (seed, step, env ids, A): drawn over A columns,
    not 2A."""
    from fleetrl_amd import DevicePolicy

    kind, D, E = case_of(i + 1)
    nets, _, _, _ = make(kind, D, A)
    pol = DevicePolicy(sm.pm.random_layers(np.random.default_rng(A), (D, A)))
    x = on_device(sm.observations(E, D))
    for seed, step, offset in ((sm.SEED, 0, 0), (3, 2 ** 32, 5), ((1 << 63) | 12345, 2 ** 32 - 1, 2 ** 31 - 40)):
        want = torch.full((E, A), 9.0, device=dev())
        pol.sample(x, 0.0, seed=seed, step=step, env_id_offset=offset, noise=want)
        got = full_act(nets, x, offset=offset, step=step, seed=seed)
        assert np.array_equal(bits(got["noise"]), bits(want)), (seed, step, offset)
    nets.close(), pol.close()


# ---- 2. u, a, log_prob: each against the model fed the device's outputs of the stage before ------------------------------------------
def _stages(tag, nets, x, noise=None):
    E, A = x.shape[0], nets.act_dim
    if noise is None:
        got = full_act(nets, x)
    else:
        out = {k: torch.full((E, A), 9.0, device=dev()) for k in ("gaussian", "mean", "log_std")}
        lp = torch.full((E,), 9.0, device=dev())
        a = nets.act(x, noise=noise, noise_given=True, gaussian_actions_out=out["gaussian"], log_prob_out=lp, mean_out=out["mean"],
                     log_std_out=out["log_std"])
        torch.cuda.synchronize()
        got = dict(out, actions=a, log_prob=lp, noise=noise)
    g = {k: host(v) for k, v in got.items()}
    u64, ub = sm.u_reference(g["mean"], g["log_std"], g["noise"])
    eu = np.abs(g["gaussian"].astype(np.float64) - u64)
    a64, ab = sm.a_reference(g["gaussian"])
    ea = np.abs(g["actions"].astype(np.float64) - a64)
    lp32 = sm.log_prob32(g["log_std"], g["noise"], g["actions"])
    lb = sm.log_prob_bound(g["log_std"], g["noise"], g["actions"])
    el = np.abs(g["log_prob"].astype(np.float64) - lp32.astype(np.float64))
    fig = {"u_err_over_bound": float((eu / ub).max()), "a_err_over_bound": float((ea / ab).max()), "log_prob_max_abs_err": float(el.max()),
           "log_prob_err_over_bound": float((el / lb).max()), "log_prob_bound_max": float(lb.max()), "max_abs_u": float(np.abs(g["gaussian"]).max()),
           "saturated_columns": int((np.abs(g["actions"]) == 1).sum())}
    _parity[tag] = fig
    print(tag, json.dumps(fig))
    write_parity()
    assert (eu <= ub).all() and (ea <= ab).all() and (el <= lb).all(), fig
    assert (np.abs(g["actions"]) <= 1).all()
    return g, fig


@pytest.mark.parametrize("i,A", list(enumerate(sm.ACTS)))
def test_the_stages_stay_within_the_models_bounds(i, A):
    kind, D, E = case_of(i + 2)
    nets, _, _, _ = make(kind, D, A, salt=1)
    _stages(f"stages/{kind}-D{D}-A{A}-E{E}", nets, on_device(sm.observations(E, D)))
    nets.close()


@pytest.mark.parametrize("A", (5, 130))
def test_the_log_probability_holds_its_bound_where_the_action_saturates(A):
    """A wide log_std (sd about 2 and more) under given noise of up to +-5.5: |u| reaches 12 and beyond, a rounds to +-1, c = logf(1e-6f)."""
    nets, _, _, _ = make("one", sm.D_SMALL, A, salt=2, log_std_bias=np.full(A, 0.7, np.float32))
    E = 37
    noise = on_device(np.clip(np.random.default_rng(A).standard_normal((E, A)) * 2, -5.5, 5.5).astype(np.float32))
    g, fig = _stages(f"saturated/A{A}", nets, on_device(sm.observations(E, sm.D_SMALL)), noise=noise)
    assert fig["saturated_columns"] > 0 and fig["max_abs_u"] >= 12
    _, c = sm.terms32(g["log_std"], g["noise"], g["actions"])
    assert (c[np.abs(g["actions"]) == 1] == np.float32(np.log(np.float64(np.float32(1e-6))))).all()
    nets.close()


@pytest.mark.parametrize("i,A", [(0, 3), (1, 50), (2, 65)])
def test_deterministic_is_the_existing_sac_route(i, A):
    """tanh(mean) bit-equal to DevicePolicy over latent_pi + the mu rows with output tanh, what policy.py loads an SB3 SAC archive as."""
    from fleetrl_amd import DevicePolicy

    kind, D, E = case_of(i)
    nets, actor, _, activation = make(kind, D, A)
    mu = actor[:-1] + [(actor[-1][0][:A], actor[-1][1][:A])]
    pol = DevicePolicy(mu, activation=activation, output="tanh")
    x = on_device(sm.observations(E, D))
    mean, ls = torch.full((E, A), 9.0, device=dev()), torch.full((E, A), 9.0, device=dev())
    got = nets.act(x, deterministic=True, mean_out=mean, log_std_out=ls)
    assert np.array_equal(bits(got), bits(pol.act(x)))
    stochastic = full_act(nets, x)
    assert np.array_equal(bits(mean), bits(stochastic["mean"])) and np.array_equal(bits(ls), bits(stochastic["log_std"]))
    nets.close(), pol.close()


# ---- 3. what a row depends on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,A", [(0, 1), (1, 5), (2, 50), (3, 130), (4, 256)])
def test_act_rows_depend_on_their_own_row_only(i, A):
    kind, D, _ = case_of(i)
    nets, _, _, _ = make(kind, D, A)
    E = 37
    x = on_device(sm.observations(E, D))
    whole = {k: bits(v) for k, v in full_act(nets, x, offset=100).items()}
    for r in (0, 15, 16, 36):  # a row alone, and in a batch at another place, under its global id
        alone = full_act(nets, x[r:r + 1], offset=100 + r)
        for k, v in alone.items():
            assert np.array_equal(bits(v)[0], whole[k][r]), (k, r)
    shifted = full_act(nets, x[5:22], offset=105)
    for k, v in shifted.items():
        assert np.array_equal(bits(v), whole[k][5:22]), k
    bare = full_act(nets, x, offset=100, optional=False)  # without every optional output
    assert np.array_equal(bits(bare["actions"]), whole["actions"])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = full_act(nets, x, offset=100)
    assert all(np.array_equal(bits(other[k]), whole[k]) for k in whole)
    nets.close()


def test_act_with_a_normaliser_equals_act_on_normalised_input():
    from fleetrl_amd import DeviceNormalizer

    D, A, E = sm.D_CHUNKED, 5, 17
    nets, _, _, _ = make("relu", D, A)
    norm = DeviceNormalizer(E, D, clip_obs=4.0)
    gen = torch.Generator(device=dev())
    gen.manual_seed(D)
    rew, done = torch.zeros(E, device=dev(), dtype=torch.float64), torch.zeros(E, device=dev(), dtype=torch.uint8)
    for _ in range(3):
        norm.step_torch(torch.randn((E, D), device=dev(), generator=gen) * 3 + 1, rew, done)
    norm.configure(training=False)
    raw = torch.randn((E, D), device=dev(), generator=gen) * 5 + 1
    applied, _, _ = norm.step_torch(raw, rew, done)
    assert not torch.equal(applied, raw)
    want, got = full_act(nets, applied), full_act(nets, raw, normalizer=norm)
    assert all(np.array_equal(bits(got[k]), bits(want[k])) for k in want)
    fewer = full_act(nets, raw[:3], normalizer=norm)
    assert all(np.array_equal(bits(fewer[k]), bits(want[k])[:3]) for k in want)
    norm.close(), nets.close()


# ---- 4. the target -------------------------------------------------------------------------------------------------------------------
def batch(B, D, salt=0):
    rng = np.random.default_rng(991 + salt + B)
    rewards = rng.standard_normal(B).astype(np.float32)
    dones = (rng.random(B) < 0.3).astype(np.float32)
    if B > 1:
        dones[0], dones[1] = 1.0, 0.0
    return on_device(sm.observations(B, D, salt=3)), on_device(rewards), on_device(dones)


def full_target(online, targets, nx, r, d, alpha, offset=0, step=7, optional=True, gamma=0.99):
    B, A = nx.shape[0], online.act_dim
    out = {}
    if optional:
        out = {"noise": torch.full((B, A), 9.0, device=dev()), "next_actions": torch.full((B, A), 9.0, device=dev()),
               "next_log_prob": torch.full((B,), 9.0, device=dev()), "q": torch.full((B, online.n_critics), 9.0, device=dev())}
    y = online.target(targets, nx.contiguous(), r.contiguous(), d.contiguous(), gamma=gamma, ent_coef=alpha, seed=sm.TARGET_SEED, step=step,
                      row_offset=offset, noise=out.get("noise"), next_actions_out=out.get("next_actions"),
                      next_log_prob_out=out.get("next_log_prob"), q_out=out.get("q"))
    out["y"] = y
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("i,A,nc", [(0, 1, 2), (1, 4, 1), (2, 50, 2), (3, 65, 1), (4, 130, 2), (5, 256, 2)])
def test_the_target_is_act_the_critics_and_four_float32_operations(i, A, nc):
    """next_actions / next_log_prob: `act` on the online handle; q: what fleet_td3_critic_grad_dev reports on a plain TD3 handle that
    holds the target critics, for (next_obs, a'); y: the model's four float32 operations from the device's q, lp and alpha."""
    from fleetrl_amd import DeviceTD3Grad, DeviceTD3Target

    kind, D, B = case_of(i)
    online, _, _, activation = make(kind, D, A, nc, salt=3)
    # (the targets differ in their trunks: the LDS stride is the larger of the two)
    targets, _, tcritics, tact = make(KINDS[(i + 1) % 3], D, A, nc, salt=4)
    nx, r, d = batch(B, D)
    alpha = torch.tensor([0.37], device=dev())
    got = full_target(online, targets, nx, r, d, alpha, offset=9)
    acted = full_act(online, nx, offset=9, step=7, seed=sm.TARGET_SEED)
    assert np.array_equal(bits(got["next_actions"]), bits(acted["actions"]))
    assert np.array_equal(bits(got["next_log_prob"]), bits(acted["log_prob"]))
    assert np.array_equal(bits(got["noise"]), bits(acted["noise"]))
    plain = DeviceTD3Target(sm.pm.random_layers(np.random.default_rng(1), (D, A)), tcritics, activation=tact)
    grad = DeviceTD3Grad(plain, B)
    params = [torch.nn.Parameter(on_device(t)) for net in tcritics for w, b in net for t in (w, b)]
    q = torch.full((B, nc), 9.0, device=dev())
    grad.critic_grad((nx, got["next_actions"]), torch.zeros(B, device=dev()), into=params, q_out=q)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got["q"]), bits(q))
    want = sm.target32(host(r), host(d), 0.99, host(got["q"]), np.float32(0.37), host(got["next_log_prob"]))
    assert np.array_equal(bits(got["y"]), want.view(np.int32))
    done = host(d) == 1
    assert np.array_equal(bits(got["y"])[done], bits(r)[done])  # dones = 1 rows give the rewards exactly
    ref = sm.sb3_target64(host(r), host(d), 0.99, host(got["q"]), np.float32(0.37), host(got["next_log_prob"]))
    assert np.allclose(host(got["y"]), ref, rtol=1e-5, atol=1e-5)
    grad.close(), plain.close(), online.close(), targets.close()


def test_alpha_is_read_when_the_launch_runs():
    """alpha changed on the device between two calls, without a host wait, changes y accordingly."""
    D, A, B = sm.D_SMALL, 5, 17
    online, _, _, _ = make("tanh", D, A, salt=5)
    targets, _, _, _ = make("tanh", D, A, salt=6)
    nx, r, d = batch(B, D)
    alpha = torch.tensor([0.2], device=dev())
    q, lp = torch.empty((B, 2), device=dev()), torch.empty(B, device=dev())
    y1 = online.target(targets, nx, r, d, gamma=0.9, ent_coef=alpha, seed=1, step=2, q_out=q, next_log_prob_out=lp)
    alpha.mul_(3.0)  # enqueued on the same stream: no synchronisation
    y2 = online.target(targets, nx, r, d, gamma=0.9, ent_coef=alpha, seed=1, step=2)
    torch.cuda.synchronize()
    a1, a2 = np.float32(0.2), host(alpha)[0]
    assert a2 == np.float32(0.2) * np.float32(3.0)
    assert np.array_equal(bits(y1), sm.target32(host(r), host(d), 0.9, host(q), a1, host(lp)).view(np.int32))
    assert np.array_equal(bits(y2), sm.target32(host(r), host(d), 0.9, host(q), a2, host(lp)).view(np.int32))
    assert not np.array_equal(bits(y1), bits(y2))
    online.close(), targets.close()


@pytest.mark.parametrize("i,A", [(0, 3), (1, 64), (2, 130)])
def test_target_rows_depend_on_their_own_row_only(i, A):
    kind, D, _ = case_of(i)
    online, _, _, _ = make(kind, D, A, salt=7)
    targets, _, _, _ = make(kind, D, A, salt=8)
    B = 37
    nx, r, d = batch(B, D)
    alpha = torch.tensor([0.11], device=dev())
    whole = {k: bits(v) for k, v in full_target(online, targets, nx, r, d, alpha, offset=50).items()}
    for row in (0, 15, 16, 36):
        alone = full_target(online, targets, nx[row:row + 1], r[row:row + 1], d[row:row + 1], alpha, offset=50 + row)
        for k, v in alone.items():
            assert np.array_equal(bits(v)[0], whole[k][row]), (k, row)
    shifted = full_target(online, targets, nx[5:22], r[5:22], d[5:22], alpha, offset=55)
    for k, v in shifted.items():
        assert np.array_equal(bits(v), whole[k][5:22]), k
    bare = full_target(online, targets, nx, r, d, alpha, offset=50, optional=False)
    assert np.array_equal(bits(bare["y"]), whole["y"])
    online.close(), targets.close()


# ---- 5. the shared entries on a squashed handle ----------------------------------------------------------------------------------------
def _params_of(actor, critics):
    return [torch.nn.Parameter(on_device(t)) for net in [actor] + list(critics) for w, b in net for t in (w, b)]


def test_load_export_and_polyak_work_tensor_for_tensor():
    D, A = sm.D_CHUNKED, 5
    nets, actor, critics, _ = make("relu", D, A, salt=9)
    actor2, critics2, _ = sm.networks("relu", D, A, 2, 10)
    new = _params_of(actor2, critics2)
    assert nets.describe()["squashed"] and nets.describe()["actor"]["widths"][-1] == 2 * A and nets.describe()["act_dim"] == A
    start = nets.export_torch()
    for t, (w, b) in zip(zip(start[0::2], start[1::2]), [l for net in [actor] + critics for l in net]):
        assert np.array_equal(host(t[0]), w) and np.array_equal(host(t[1]), b)
    nets.polyak(new, 0.005)
    blended = nets.export_torch()
    for got, t0, p in zip(blended, start, new):
        assert np.array_equal(bits(got), qm.polyak_bits(host(t0), host(p), 0.005).view(np.int32))
    nets.load_torch(new)
    for got, p in zip(nets.export_torch(), new):
        assert np.array_equal(bits(got), bits(p))
    nets.close()


@pytest.mark.parametrize("i,A,nc", [(0, 3, 2), (1, 50, 1), (2, 65, 2)])
def test_the_critic_gradient_is_the_plain_td3_handles(i, A, nc):
    """Gradients, q and stats of fleet_td3_critic_grad_dev on the squashed handle bit-equal to a plain TD3 handle with the same critics."""
    from fleetrl_amd import DeviceTD3Grad, DeviceTD3Target

    kind, D, _ = case_of(i)
    B = 33
    nets, _, critics, activation = make(kind, D, A, nc, salt=11)
    plain = DeviceTD3Target(sm.pm.random_layers(np.random.default_rng(2), (D, A)), critics, activation=activation)
    obs, r, _ = batch(B, D, salt=1)
    actions = on_device(np.tanh(np.random.default_rng(A).standard_normal((B, A))).astype(np.float32))
    outs = []
    for handle in (nets, plain):
        grad = DeviceTD3Grad(handle, B)
        params = [torch.nn.Parameter(on_device(t)) for net in critics for w, b in net for t in (w, b)]
        q = torch.full((B, nc), 9.0, device=dev())
        stats = grad.critic_grad((obs, actions), r, into=params, q_out=q)
        torch.cuda.synchronize()
        outs.append([bits(p.grad) for p in params] + [bits(q), bits(stats)])
        grad.close()
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert any(g.any() for g in outs[0][:-2])
    nets.close(), plain.close()


def test_adam_steps_the_critics_and_the_next_target_sees_them_without_a_host_wait():
    from fleetrl_amd import DeviceAdam, DeviceTD3Grad

    D, A, B = sm.D_SMALL, 5, 17
    online, _, _, _ = make("tanh", D, A, salt=12)
    nets, actor, critics, _ = make("tanh", D, A, salt=13)  # the handle whose critics are trained and then read as targets
    params = [torch.nn.Parameter(on_device(t)) for net in critics for w, b in net for t in (w, b)]
    grad, adam = DeviceTD3Grad(nets, B), DeviceAdam(nets, params, nets="critic", lr=1e-2)
    nx, r, d = batch(B, D)
    alpha = torch.tensor([0.2], device=dev())
    actions = on_device(np.zeros((B, A), np.float32))
    q0, q1 = torch.empty((B, 2), device=dev()), torch.empty((B, 2), device=dev())
    y0 = online.target(nets, nx, r, d, gamma=0.99, ent_coef=alpha, seed=1, step=1, q_out=q0)
    grad.critic_grad((nx, actions), y0, into=params)
    adam.step()
    y1 = online.target(nets, nx, r, d, gamma=0.99, ent_coef=alpha, seed=1, step=1, q_out=q1)  # enqueued behind the step
    torch.cuda.synchronize()
    assert not np.array_equal(bits(q0), bits(q1)) and not np.array_equal(bits(y0), bits(y1))
    exported = nets.export_torch()
    for got, p in zip(exported[2 * len(actor):], params):  # the image moved with the parameters
        assert np.array_equal(bits(got), bits(p))
    fresh, _, _, _ = make("tanh", D, A, salt=13)
    fresh.load_torch(list(exported))
    q2 = torch.empty((B, 2), device=dev())
    online.target(fresh, nx, r, d, gamma=0.99, ent_coef=alpha, seed=1, step=1, q_out=q2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(q1), bits(q2))
    adam.close(), grad.close(), fresh.close(), nets.close(), online.close()


# ---- 6. the refusals that need handles -------------------------------------------------------------------------------------------------
def test_the_new_entries_refuse_plain_handles_and_mismatched_pairs():
    from fleetrl_amd import DeviceNormalizer, DeviceTD3Target, FleetHipError, _capi

    D, A, B = sm.D_SMALL, 3, 4
    sac, actor, critics, _ = make("tanh", D, A, 2)
    plain = DeviceTD3Target(sm.pm.random_layers(np.random.default_rng(1), (D, A)), critics, activation="tanh")
    nx, r, d = batch(B, D)
    alpha = torch.tensor([0.2], device=dev())
    acts = torch.full((B, A), 9.0, device=dev())
    y = torch.full((B,), 9.0, device=dev())
    # a plain TD3 handle given to either new entry (through the C ABI: a DeviceTD3Target has no method that would call them)
    aa, ta = _capi.FleetSacActArgs(), _capi.FleetSacTargetArgs()
    aa.struct_bytes, aa.actions = C.sizeof(aa), acts.data_ptr()
    ta.struct_bytes, ta.gamma, ta.ent_coef, ta.target_q = C.sizeof(ta), 0.9, alpha.data_ptr(), y.data_ptr()
    plain.use_torch_stream(), sac.use_torch_stream()
    with pytest.raises(FleetHipError, match="fleet_sac_act_dev: the handle's actor is not a squashed Gaussian"):
        plain._check(plain.lib.fleet_sac_act_dev(plain.h, nx.data_ptr(), B, None, C.byref(aa)))
    with pytest.raises(FleetHipError, match="fleet_sac_target_dev: the online handle's actor is not a squashed Gaussian"):
        plain._check(plain.lib.fleet_sac_target_dev(plain.h, sac.h, nx.data_ptr(), r.data_ptr(), d.data_ptr(), B, C.byref(ta)))
    with pytest.raises(FleetHipError, match="fleet_sac_target_dev: the target networks' handle is not one fleet_sac_create made"):
        sac.target(plain, nx, r, d, gamma=0.9, ent_coef=alpha, seed=1, step=1, out=y)
    with pytest.raises(FleetHipError, match="fleet_sac_target_dev: null target networks handle"):
        sac.target(None, nx, r, d, gamma=0.9, ent_coef=alpha, seed=1, step=1, out=y)
    for other in (make("tanh", D + 1, A, 2)[0], make("tanh", D, A + 1, 2)[0], make("tanh", D, A, 1)[0]):
        with pytest.raises(FleetHipError, match=r"fleet_sac_target_dev: the online networks have \(obs_dim, act_dim, n_critics\) = \(7, 3, 2\)"):
            sac.target(other, nx, r, d, gamma=0.9, ent_coef=alpha, seed=1, step=1, out=y)
        other.close()
    twin = make("tanh", D, A, 2, salt=1)[0]
    side = torch.cuda.Stream(device=dev())
    sac.use_torch_stream()
    twin.set_stream(side.cuda_stream)
    a = _capi.FleetSacTargetArgs()
    a.gamma, a.ent_coef, a.target_q = 0.9, alpha.data_ptr(), y.data_ptr()
    with pytest.raises(FleetHipError, match="fleet_sac_target_dev: .*handles that do not launch on one stream"):
        sac.soft_target_dev(twin, nx.data_ptr(), r.data_ptr(), d.data_ptr(), B, a)
    wrong = DeviceNormalizer(B, D + 1)
    with pytest.raises(FleetHipError, match=f"fleet_sac_act_dev: the normaliser has obs_dim {D + 1} on device 0, the networks {D} on device 0"):
        sac.act(nx, seed=1, step=1, normalizer=wrong, actions_out=acts)
    torch.cuda.synchronize()
    assert bool((acts == 9.0).all()) and bool((y == 9.0).all())  # nothing was launched
    sac.target(twin, nx, r, d, gamma=0.9, ent_coef=alpha, seed=1, step=1, out=y)  # (the Python call puts both on torch's stream)
    torch.cuda.synchronize()
    assert bool((y != 9.0).all())
    wrong.close(), twin.close(), plain.close(), sac.close()


def test_the_td3_entries_refuse_a_squashed_handle_and_the_handle_goes_on_working():
    from fleetrl_amd import DeviceAdam, DeviceReplayBuffer, DeviceTD3Grad, DeviceTD3Train, FleetHipError, _capi

    D, A, B = sm.D_SMALL, 3, 4
    sac, actor, critics, _ = make("tanh", D, A, 2)
    twin = make("tanh", D, A, 2, salt=1)[0]
    nx, r, d = batch(B, D)
    y = torch.full((B,), 9.0, device=dev())
    ta = _capi.FleetQTargetArgs()
    sigma = torch.full((A,), 0.2, device=dev())
    ta.gamma, ta.noise_clip, ta.act_lo, ta.act_hi, ta.sigma, ta.target_q = 0.9, 0.5, -1.0, 1.0, sigma.data_ptr(), y.data_ptr()
    with pytest.raises(FleetHipError, match="fleet_qtarget_target_dev: the handle's actor is a squashed Gaussian"):
        sac.target_dev(nx.data_ptr(), r.data_ptr(), d.data_ptr(), B, ta)
    grad = DeviceTD3Grad(sac, B)
    aparams = [torch.nn.Parameter(on_device(t)) for w, b in actor for t in (w, b)]
    cparams = [torch.nn.Parameter(on_device(t)) for net in critics for w, b in net for t in (w, b)]
    acts = torch.full((B, A), 9.0, device=dev())
    with pytest.raises(FleetHipError, match="fleet_td3_actor_grad_dev: the networks' actor is a squashed Gaussian"):
        grad.actor_grad(nx, into=aparams, actions_out=acts)
    replay = DeviceReplayBuffer(64, 4, D, A)
    adam_a, adam_c = DeviceAdam(sac, aparams, nets="actor"), DeviceAdam(sac, cparams, nets="critic")
    with pytest.raises(FleetHipError, match="fleet_offpolicy_create: the networks' actor is a squashed Gaussian"):
        DeviceTD3Train(replay, twin, grad, adam_a, adam_c, max_steps=4)
    torch.cuda.synchronize()
    assert bool((y == 9.0).all()) and bool((acts == 9.0).all())  # nothing was launched
    alpha = torch.tensor([0.2], device=dev())
    sac.target(twin, nx, r, d, gamma=0.9, ent_coef=alpha, seed=1, step=1, out=y)  # the handles go on working
    stats = grad.critic_grad((nx, acts * 0), y, into=cparams)
    torch.cuda.synchronize()
    assert bool((y != 9.0).all()) and np.isfinite(host(stats)).all()
    for h in (adam_a, adam_c, replay, grad, twin, sac):
        h.close()


# ---- 7. the example ------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_as_a_child_process():
    env = dict(os.environ, PYTHONPATH=sm.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(sm.ROOT, "examples", "sac_device_targets.py"), "--envs", "8", "--steps", "24",
                          "--batch", "32"], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines and lines[-1]["gradient_steps"] > 0 and np.isfinite(lines[-1]["critic_loss"]) and np.isfinite(lines[-1]["ent_coef"])
