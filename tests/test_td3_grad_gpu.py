"""TD3's minibatch gradients on the device (fleet_td3.hip) against the launch this project already pins (DeviceTD3Target.target, bit for
bit), against fma32 chains where the arithmetic is exact, against the float64 model of tests/td3_model.py under the project's rule,
and what a result may not depend on."""
import json
import os

import numpy as np
import pytest

import policy_bits as pb
import td3_model as tm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(tm.ROOT, "profiles", "td3_grad_parity.json")
f32 = np.float32
INF = float("inf")
_parity = {}


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


def make_nets(c, actor=None, critics=None):
    from fleetrl_amd import DeviceTD3Target

    return DeviceTD3Target(actor or c["actor"], critics or c["critics"], activation=c["activation"], output=c["output"], low=c["low"],
                           high=c["high"])


def make_params(c):
    """torch's parameters in load_torch's order: (the actor's, the critics')."""
    P = lambda nets: [torch.nn.Parameter(on_device(t)) for net in nets for w, b in net for t in (w, b)]  # noqa: E731
    return P([c["actor"]]), P(c["critics"])


def open_case(name, max_batch=tm.ROWS):
    from fleetrl_amd import DeviceTD3Grad

    c = tm.case(name)
    assert all(tm.facts_of(c).values()), tm.facts_of(c)  # the table's conditions, enforced in every case
    nets = make_nets(c)
    return c, nets, DeviceTD3Grad(nets, max_batch), make_params(c)


def padded(a, B, rows):
    """The first B rows of `a` on the device; rows > B: a buffer of that many rows whose tail is NaN, and a view of its head."""
    a = np.array(a[:B])
    if rows and rows > B:
        a = np.concatenate([a, np.full((rows - B, *a.shape[1:]), np.nan, a.dtype)])
    return on_device(a)[:B]


def run_critic(g, c, B, params, *, rows=None, fill=None, outputs=True, obs=None, actions=None, target_q=None):
    """One call of the critic entry -> {"grads": [...], "stats", "q"} as host arrays."""
    obs = padded(c["obs"], B, rows) if obs is None else obs
    actions = padded(c["actions"], B, rows) if actions is None else actions
    target_q = padded(c["target_q"], B, rows) if target_q is None else target_q
    q = torch.full((B, g.n_critics), np.nan, device=dev()) if outputs else None
    if fill is not None:
        for p in params:
            p.grad = torch.full_like(p, fill)
    stats = g.critic_grad((obs, actions), target_q, into=params, q_out=q)
    return {"grads": [host(p.grad).copy() for p in params], "stats": host(stats), "q": None if q is None else host(q)}


def run_actor(g, c, B, params, *, rows=None, fill=None, outputs=True, obs=None):
    """One call of the actor entry -> {"grads": [...], "stats", "q", "actions"} as host arrays."""
    obs = padded(c["obs"], B, rows) if obs is None else obs
    q = torch.full((B,), np.nan, device=dev()) if outputs else None
    a = torch.full((B, g.act_dim), np.nan, device=dev()) if outputs else None
    if fill is not None:
        for p in params:
            p.grad = torch.full_like(p, fill)
    stats = g.actor_grad(obs, into=params, actions_out=a, q_out=q)
    return {"grads": [host(p.grad).copy() for p in params], "stats": host(stats), "q": None if q is None else host(q),
            "actions": None if a is None else host(a)}


def same(a, b, keys=("stats", "q", "actions")):
    return all(pb.same_bits(x, y) for x, y in zip(a["grads"], b["grads"])) and \
        all(pb.same_bits(a[k], b[k]) for k in keys if k in a and a[k] is not None and b[k] is not None)


def target_launch(nets, obs):
    """The pinned launch on the same image with sigma = 0 and no action clip: pi(obs) and every critic's q over (obs, pi(obs))."""
    B = obs.shape[0]
    na, q = torch.full((B, nets.act_dim), np.nan, device=dev()), torch.full((B, nets.n_critics), np.nan, device=dev())
    zero = torch.zeros(B, device=dev())
    nets.target(obs, zero, zero, gamma=0.99, sigma=0.0, noise_clip=0.5, low=-INF, high=INF, seed=1, step=0, next_actions_out=na, q_out=q)
    return na, q


# ---- 1, 2. the launch already pinned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_actor_entry_equals_the_target_launch_bit_for_bit(name):
    c, nets, g, (pa, pc) = open_case(name)
    for B in tm.CASES[name][7]:
        obs = on_device(c["obs"][:B])
        na, q = target_launch(nets, obs)
        got = run_actor(g, c, B, pa, obs=obs)
        assert np.isfinite(got["actions"]).all() and np.isfinite(got["q"]).all()
        assert pb.same_bits(got["actions"], host(na)) and pb.same_bits(got["q"], host(q)[:, 0]), (name, B)
    g.close()
    nets.close()


@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_critic_entry_equals_the_target_launch_bit_for_bit(name):
    """The critic entry on (obs, the target launch's actions) computes that launch's q, for every critic."""
    c, nets, g, (pa, pc) = open_case(name)
    for B in tm.CASES[name][7]:
        obs = on_device(c["obs"][:B])
        na, q = target_launch(nets, obs)
        got = run_critic(g, c, B, pc, obs=obs, actions=na)
        assert np.isfinite(got["q"]).all() and pb.same_bits(got["q"], host(q)), (name, B)
    g.close()
    nets.close()


# ---- 3. where the arithmetic is exact ---------------------------------------------------------------------------------------------------
def neumaier32(terms):
    s, c = f32(0.0), f32(0.0)
    for x in terms:
        x = f32(x)
        t = f32(s + x)
        c = f32(c + (f32(f32(s - t) + x) if abs(s) >= abs(x) else f32(f32(x - t) + s)))
        s = t
    return f32(s + c)


@pytest.mark.parametrize("name", ["5x3-one-layer", "5x3-one-layer-ddpg"])
@pytest.mark.parametrize("B", [1, 3, 17])
def test_a_one_layer_critics_gradients_and_loss_equal_fma_chains_bit_for_bit(name, B):
    """e = q - y; dq = (2.0f * (1.0f / B)) * e; dW[0][k] = fmaf(dq[b], x[b][k], acc) over ascending b with x = (obs, actions): the seam
    included; db = the ascending sum; the loss from the tiles' compensated partials."""
    c, nets, g, (pa, pc) = open_case(name)
    got = run_critic(g, c, B, pc)
    x = np.concatenate([c["obs"][:B], c["actions"][:B]], axis=1)
    invB = f32(1.0) / f32(B)
    losses = []
    for ci, layers in enumerate(c["critics"]):
        q = pb.forward_bits(layers, x, "tanh", "none")[:, 0]
        assert pb.same_bits(got["q"][:, ci], q)
        e = (q - c["target_q"][:B]).astype(f32)
        dq = (f32(f32(2.0) * invB) * e).astype(f32)
        dW, db = np.zeros(x.shape[1], f32), f32(0.0)
        for b in range(B):
            dW = pb.fma32(dq[b], x[b], dW)
            db = f32(db + dq[b])
        assert pb.same_bits(got["grads"][2 * ci], dW[None, :]) and pb.same_bits(got["grads"][2 * ci + 1], np.array([db])), ci
        sq = (e * e).astype(f32)
        losses.append(f32(neumaier32([neumaier32(sq[t:t + 16]) for t in range(0, B, 16)]) * invB))
    if len(losses) == 1:
        losses.append(f32(0.0))
    assert pb.same_bits(got["stats"], np.array([f32(losses[0] + losses[1]), losses[0], losses[1], 0, 0, 0, 0, 0], f32))
    g.close()
    nets.close()


# ---- 4. the float64 model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_gradients_and_statistics_stay_within_eight_times_the_float32_reference_error(name):
    """The project's rule: within 8 * max(eps_ref, 2^-24 * max |ref|) of the float64 model, per gradient tensor and per statistic;
    eps_ref = |torch-CPU float32 autograd - the model|.  Every error / bound ratio goes to profiles/td3_grad_parity.json."""
    c, nets, g, (pa, pc) = open_case(name)
    names = tm.tensor_names(name)
    worst, bad = 0.0, []
    for B in tm.CASES[name][7]:
        m, r = tm.model(name, B), tm.reference32(name, B)
        gc, ga = run_critic(g, c, B, pc), run_actor(g, c, B, pa)
        items = []
        for entry, got, stat_names in (("critic", gc, tm.CRITIC_STATS), ("actor", ga, tm.ACTOR_STATS)):
            assert len(got["grads"]) == len(m[entry]["grads"]) == len(names[entry])
            items += list(zip(names[entry], got["grads"], m[entry]["grads"], r[entry]["grads"]))
            items += [(k, got["stats"][i], m[entry]["stats"][k], r[entry]["stats"][k]) for i, k in enumerate(stat_names)]
            assert not got["stats"][len(stat_names):].any()  # the rest are 0
        for n, gg, mm, rr in items:
            gg, mm = np.asarray(gg, np.float64), np.asarray(mm, np.float64)
            assert gg.shape == mm.shape and np.isfinite(gg).all(), (name, B, n)
            eps_ref = float(np.abs(np.asarray(rr, np.float64) - mm).max())
            err, mag = float(np.abs(gg - mm).max()), float(np.abs(mm).max())
            bound = 8 * max(eps_ref, 2.0 ** -24 * mag)
            ratio = err / bound if bound else (0.0 if err == 0 else np.inf)
            print(f"{name} B={B} {n}: eps_ref {eps_ref:.3g} device {err:.3g} bound {bound:.3g} ratio {ratio:.3g}")
            _parity[f"{name}/B{B}/{n}"] = {"eps_ref": eps_ref, "device_err": err, "bound": bound, "err_over_bound": ratio}
            worst = max(worst, ratio)
            if not err <= bound:
                bad.append((name, B, n, err, bound))
    print(f"{name}: worst error / bound {worst:.3g}")
    g.close()
    nets.close()
    with open(PARITY_FILE, "w") as fh:
        json.dump({"bound": "8 * max(eps_ref, 2^-24 * max|ref|)", "worst": max(v["err_over_bound"] for v in _parity.values()),
                   "cases": dict(sorted(_parity.items()))}, fh, indent=1)
    assert not bad, bad


# ---- 5. what a result does not depend on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["129x65-65-63-relu-clip", "45x3-deep-critic"])
def test_a_result_depends_on_the_inputs_and_b_and_on_nothing_else(name):
    from fleetrl_amd import DeviceTD3Grad

    c, nets, g, (pa, pc) = open_case(name)
    B = 17

    def both(h=g, **kw):
        return run_critic(h, c, B, pc, **kw), run_actor(h, c, B, pa, **kw)

    ref = both(fill=np.nan)  # the gradient tensors come in full of NaN and are overwritten
    for r in ref:
        assert all(np.isfinite(x).all() for x in r["grads"]) and np.isfinite(r["stats"]).all()
    agree = lambda got: same(got[0], ref[0]) and same(got[1], ref[1])  # noqa: E731
    assert agree(both())  # the run
    assert agree(both(fill=1e30))  # what the tensors held
    assert agree(both(outputs=False))  # which optional outputs are asked for
    s = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # the stream: the networks handle's, moved by fleet_qtarget_set_stream
        other = both()
    torch.cuda.synchronize()
    assert agree(other)
    big = DeviceTD3Grad(nets, 4 * tm.ROWS + 5)  # the capacity of the scratch
    assert big.describe()["scratch_bytes"] > g.describe()["scratch_bytes"] and agree(both(big))
    big.close()
    assert agree(both(rows=tm.ROWS))  # NaN rows behind row 17 in every buffer
    run_critic(g, c, tm.ROWS, pc), run_actor(g, c, tm.ROWS, pa)  # a larger batch in between leaves the scratch's rows 17.. filled
    assert agree(both())
    g.close()
    nets.close()


# ---- 6. the image follows load_torch without a host wait ------------------------------------------------------------------------------------
def test_entries_enqueued_behind_load_torch_use_the_new_weights():
    from fleetrl_amd import DeviceTD3Grad

    name = "127x2-64-64-tanh"
    c, nets, g, (pa, pc) = open_case(name)
    B = 33
    before = run_critic(g, c, B, pc), run_actor(g, c, B, pa)
    rng = np.random.default_rng(11)
    new = [[((w + rng.standard_normal(w.shape).astype(f32) * f32(0.05)).astype(f32), (b + rng.standard_normal(b.shape).astype(f32) * f32(0.05)).astype(f32))
            for w, b in net] for net in (c["actor"], *c["critics"])]
    new_t = [on_device(t) for net in new for pair in net for t in pair]
    torch.cuda.synchronize()
    nets.load_torch(new_t)
    after = run_critic(g, c, B, pc), run_actor(g, c, B, pa)  # (nothing between them but the enqueue)
    fresh_nets = make_nets(c, new[0], new[1:])
    fresh = DeviceTD3Grad(fresh_nets, B)
    want = run_critic(fresh, c, B, pc), run_actor(fresh, c, B, pa)
    for a, w, b in zip(after, want, before):
        assert same(a, w) and not pb.same_bits(a["grads"][0], b["grads"][0])
    fresh.close()
    fresh_nets.close()
    g.close()
    nets.close()


# ---- 7. a row that is not finite -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["129x65-65-63-relu-clip", "127x2-64-64-tanh"])
def test_a_nan_observation_stays_in_its_row_for_q_and_actions_and_reaches_the_gradients(name):
    """The critic entry's e of that row is NaN, and with it every delta, gradient tensor and loss.  In the actor entry the row's q and
    the loss are NaN, and dq = -1 / B is not: under tanh every delta of the row is NaN (tanh' of a NaN), under ReLU the header's
    rules -- relu' = h > 0 ? 1 : 0 and the CLIP mask, both false for a NaN, as torch's backward has them -- make the row's deltas
    0, and the NaN reaches the first layer's dW through fmaf(0, NaN, acc) alone."""
    c, nets, g, (pa, pc) = open_case(name)
    B, D = 33, tm.CASES[name][0]
    ref = run_critic(g, c, B, pc), run_actor(g, c, B, pa)
    obs = on_device(c["obs"][:B]).clone()
    obs[20, D - 1] = float("nan")
    got = run_critic(g, c, B, pc, obs=obs), run_actor(g, c, B, pa, obs=obs)
    keep = np.arange(B) != 20
    assert np.isnan(got[0]["q"][20]).all() and pb.same_bits(got[0]["q"][keep], ref[0]["q"][keep])
    assert np.isnan(got[1]["q"][20]) and pb.same_bits(got[1]["q"][keep], ref[1]["q"][keep])
    assert np.isnan(got[1]["actions"][20]).all() and pb.same_bits(got[1]["actions"][keep], ref[1]["actions"][keep])
    assert all(np.isnan(x).any() for x in got[0]["grads"]) and np.isnan(got[0]["stats"][:3]).all()
    assert np.isnan(got[1]["stats"][0]) and np.isnan(got[1]["grads"][0][:, D - 1]).all()
    if c["activation"] == "tanh":
        assert all(np.isnan(x).any() for x in got[1]["grads"])
    g.close()
    nets.close()


# ---- refusals that need a handle -----------------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle():
    import ctypes as C

    from fleetrl_amd import FleetHipError, _capi

    c, nets, g, (pa, pc) = open_case("5x3-one-layer", max_batch=16)
    assert g.describe() == {"max_batch": 16, "scratch_bytes": g.describe()["scratch_bytes"], "tile_rows": 16} and g.tile_rows == nets.tile_rows
    # one tile of: delta [16][64] per network, part [1][8]
    assert g.describe()["scratch_bytes"] == 4 * (3 * 16 * 64 + 8)
    with pytest.raises(FleetHipError, match="fleet_td3_critic_grad_dev: B must be at most max_batch = 16, got 17"):
        run_critic(g, c, 17, pc)
    with pytest.raises(FleetHipError, match="fleet_td3_actor_grad_dev: B must be at most max_batch = 16, got 17"):
        run_actor(g, c, 17, pa)
    with pytest.raises(ValueError, match="expected 4 parameters"):
        g.critic_grad((on_device(c["obs"][:4]), on_device(c["actions"][:4])), on_device(c["target_q"][:4]), into=pc[:-1])
    with pytest.raises(ValueError, match="expected 2 parameters"):
        g.actor_grad(on_device(c["obs"][:4]), into=pc)
    ptr = pc[0].data_ptr()
    a = _capi.FleetTd3CriticArgs()
    a.B = 4
    a.obs = a.actions = a.target_q = a.stats = ptr
    with pytest.raises(FleetHipError, match="fleet_td3_critic_grad_dev: expected 4 gradient tensors"):
        g.critic_grad_dev(a, (C.c_void_p * 2)(ptr, ptr), 2)
    b = _capi.FleetTd3ActorArgs()
    b.B = 4
    b.obs = b.stats = ptr
    with pytest.raises(FleetHipError, match="fleet_td3_actor_grad_dev: expected 2 gradient tensors"):
        g.actor_grad_dev(b, (C.c_void_p * 4)(ptr, ptr, ptr, ptr), 4)
    g.close()
    nets.close()
