"""PPO's minibatch gradients on the device (fleet_ppo.hip) against the launches this project already pins (DevicePolicy.act / sample, bit
for bit), against the float64 model of tests/ppo_model.py under the project's rule, against fma32 chains where the arithmetic is
exact, and what a result may not depend on."""
import json
import os

import numpy as np
import pytest

import policy_bits as pb
import ppo_model as ppm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(ppm.ROOT, "profiles", "ppo_grad_parity.json")
f32 = np.float32
_parity = {}


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


def make_policy(c):
    from fleetrl_amd import DevicePolicy

    return DevicePolicy(c["actor"], critic_layers=c["critic"], activation=c["activation"], output="clip")


def make_params(c):
    """torch's parameters in load_torch's order, then log_std."""
    flat = [t for net in (c["actor"], c["critic"]) for w, b in net for t in (w, b)] + [c["log_std"]]
    return [torch.nn.Parameter(on_device(t)) for t in flat]


class Batch:
    def __init__(self, c, B, rows=None):
        """The first B rows of a case on the device; rows > B: buffers of that many rows whose tail is NaN."""
        for k, name in (("obs", "observations"), ("actions", "actions"), ("old_log_prob", "old_log_prob"), ("advantages", "advantages"),
                        ("returns", "returns")):
            a = np.array(c[k][:B])
            if rows and rows > B:
                a = np.concatenate([a, np.full((rows - B, *a.shape[1:]), np.nan, a.dtype)])
            setattr(self, name, on_device(a)[:B])  # (a view of the first B rows: the NaN rows lie behind it in memory)


def run(g, c, B, params, *, rows=None, batch=None, fill=None):
    """One call -> {"grads": [...], "stats", "values", "log_prob"} as host arrays."""
    b = batch or Batch(c, B, rows)
    values, log_prob = (torch.full((B,), np.nan, device=dev()) for _ in range(2))
    if fill is not None:
        for p in params:
            p.grad = torch.full_like(p, fill)
    stats = g.grad(b, params[-1], ppm.CLIP_RANGE, ppm.VF_COEF, ppm.ENT_COEF, into=params, values_out=values, log_prob_out=log_prob)
    return {"grads": [host(p.grad).copy() for p in params], "stats": host(stats), "values": host(values), "log_prob": host(log_prob)}


def same(a, b):
    return all(pb.same_bits(x, y) for x, y in zip(a["grads"], b["grads"])) and all(pb.same_bits(a[k], b[k]) for k in ("stats", "values", "log_prob"))


def open_case(name, max_batch=ppm.ROWS):
    from fleetrl_amd import DevicePPOGrad

    c = ppm.case(name)
    assert all(ppm.facts_of(c).values()), ppm.facts_of(c)  # the table's conditions, enforced in every case
    pol = make_policy(c)
    return c, pol, DevicePPOGrad(pol, max_batch), make_params(c)


# ---- 1, 2. the launches already pinned ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_values_equal_the_policy_forwards_bit_for_bit(name):
    c, pol, g, params = open_case(name)
    for B in ppm.CASES[name][5]:
        got = run(g, c, B, params)
        v = torch.full((B, 1), np.nan, device=dev())
        pol.act(on_device(c["obs"][:B]), values_out=v)
        assert np.isfinite(got["values"]).all() and pb.same_bits(got["values"], host(v)[:, 0]), (name, B)
    g.close()
    pol.close()


@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_log_prob_equals_what_sample_stored_bit_for_bit(name):
    """Under the weights and the log_std the rollout sampled with, ratio is exactly 1: approx_kl and clip_fraction are exactly 0."""
    c, pol, g, params = open_case(name)
    for B in ppm.CASES[name][5]:
        obs = on_device(c["obs"][:B])
        actions, _, stored, _ = pol.sample(obs, params[-1], seed=7, step=B, noise=on_device(c["eps"][:B]), noise_given=True)
        b = Batch(c, B)
        b.actions, b.old_log_prob = actions, stored
        got = run(g, c, B, params, batch=b)
        assert np.isfinite(got["log_prob"]).all() and pb.same_bits(got["log_prob"], host(stored)), (name, B)
        assert got["stats"][4] == 0.0 and got["stats"][5] == 0.0 and got["stats"][6] == 0.0 and got["stats"][7] == 0.0
    g.close()
    pol.close()


# ---- 3. the float64 model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_gradients_and_statistics_stay_within_eight_times_the_float32_reference_error(name):
    """The project's rule: within 8 * max(eps_ref, 2^-24 * max |ref|) of the float64 model, per gradient tensor and per statistic;
    eps_ref = |torch-CPU float32 autograd - the model|.  Every error / bound ratio goes to profiles/ppo_grad_parity.json."""
    c, pol, g, params = open_case(name)
    worst, bad = 0.0, []
    for B in ppm.CASES[name][5]:
        got, m, r = run(g, c, B, params), ppm.model(name, B), ppm.reference32(name, B)
        items = [(n, gg, mm, rr) for n, gg, mm, rr in zip(ppm.tensor_names(name), got["grads"], m["grads"], r["grads"])]
        items += [(k, got["stats"][i], m["stats"][k], r["stats"][k]) for i, k in enumerate(ppm.STATS)]
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
    pol.close()
    with open(PARITY_FILE, "w") as fh:
        json.dump({"bound": "8 * max(eps_ref, 2^-24 * max|ref|)", "worst": max(v["err_over_bound"] for v in _parity.values()),
                   "cases": dict(sorted(_parity.items()))}, fh, indent=1)
    assert not bad, bad


# ---- 4. where the arithmetic is exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_a_one_layer_critics_gradients_equal_fma_chains_bit_for_bit(B):
    """dv = ((2.0f * vf_coef) * (1.0f / B)) * (v - ret); dW[0][k] = fmaf(dv[b], x[b][k], acc) over ascending b; db = the ascending sum."""
    name = "5x3-one-layer"
    c, pol, g, params = open_case(name)
    got = run(g, c, B, params)
    x = c["obs"][:B]
    v = pb.forward_bits(c["critic"], x, "tanh", "none")[:, 0]
    assert pb.same_bits(got["values"], v)
    k = f32(f32(2.0) * f32(ppm.VF_COEF)) * (f32(1.0) / f32(B))
    dv = (k * (v - c["returns"][:B])).astype(f32)
    dW, db = np.zeros(x.shape[1], f32), f32(0.0)
    for b in range(B):
        dW = pb.fma32(dv[b], x[b], dW)
        db = f32(db + dv[b])
    assert pb.same_bits(got["grads"][2], dW[None, :]) and pb.same_bits(got["grads"][3], np.array([db]))
    vs, vc = f32(0.0), f32(0.0)  # the header's compensated sum, then the total over one tile: 0 + partial
    for b in range(B):
        e = f32(c["returns"][b] - v[b])
        x = f32(e * e)
        t = f32(vs + x)
        vc = f32(vc + (f32(f32(vs - t) + x) if abs(vs) >= abs(x) else f32(f32(x - t) + vs)))
        vs = t
    assert pb.same_bits(got["stats"][1:2], np.array([f32(f32(vs + vc) * (f32(1.0) / f32(B)))]))
    g.close()
    pol.close()


# ---- 5, 6. what a result does not depend on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["129x65-65-63-relu", "45x3-deep-actor"])
def test_a_result_depends_on_the_inputs_and_b_and_on_nothing_else(name):
    from fleetrl_amd import DevicePPOGrad

    c, pol, g, params = open_case(name)
    B = 17
    ref = run(g, c, B, params, fill=np.nan)  # (6: the gradient tensors come in full of NaN and are overwritten)
    assert all(np.isfinite(x).all() for x in ref["grads"]) and np.isfinite(ref["stats"]).all()
    assert same(run(g, c, B, params), ref)  # the run
    assert same(run(g, c, B, params, fill=1e30), ref)  # what the tensors held
    s = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # the stream: the policy's, moved by fleet_policy_set_stream
        other = run(g, c, B, params)
    torch.cuda.synchronize()
    assert same(other, ref)
    big = DevicePPOGrad(pol, 4 * ppm.ROWS + 5)  # the capacity of the scratch
    assert big.describe()["scratch_bytes"] > g.describe()["scratch_bytes"] and same(run(big, c, B, params), ref)
    big.close()
    assert same(run(g, c, B, params, rows=ppm.ROWS), ref)  # NaN rows behind row 17 in every buffer
    run(g, c, ppm.ROWS, params)  # a larger batch in between leaves the scratch's rows 17.. filled
    assert same(run(g, c, B, params), ref)
    g.close()
    pol.close()


# ---- 7. the image follows load_torch without a host wait ------------------------------------------------------------------------------------
def test_grad_enqueued_behind_load_torch_uses_the_new_weights():
    from fleetrl_amd import DevicePPOGrad, DevicePolicy

    name = "127x2-64-64-tanh"
    c, pol, g, params = open_case(name)
    B = 33
    before = run(g, c, B, params)
    rng = np.random.default_rng(11)
    new = [(w + rng.standard_normal(w.shape).astype(f32) * f32(0.05)).astype(f32) for net in (c["actor"], c["critic"]) for pair in net for w in pair]
    new_t = [on_device(w) for w in new]
    torch.cuda.synchronize()
    pol.load_torch(new_t)
    after = run(g, c, B, params)  # (nothing between the two but the enqueue)
    layers = lambda ws: [(ws[i], ws[i + 1]) for i in range(0, len(ws), 2)]  # noqa: E731
    na = 2 * len(c["actor"])
    fresh_pol = DevicePolicy(layers(new[:na]), critic_layers=layers(new[na:]), activation=c["activation"], output="clip")
    fresh = DevicePPOGrad(fresh_pol, B)
    want = run(fresh, c, B, params)
    assert same(after, want) and not pb.same_bits(after["grads"][0], before["grads"][0])
    fresh.close()
    fresh_pol.close()
    g.close()
    pol.close()


# ---- 8. a row that is not finite -----------------------------------------------------------------------------------------------------------
def test_a_nan_observation_stays_in_its_row_for_values_and_log_prob_and_reaches_the_gradients():
    name = "129x65-65-63-relu"
    c, pol, g, params = open_case(name)
    B = 33
    ref = run(g, c, B, params)
    b = Batch(c, B)
    b.observations = b.observations.clone()
    b.observations[20, 128] = float("nan")
    got = run(g, c, B, params, batch=b)
    keep = np.arange(B) != 20
    for k in ("values", "log_prob"):
        assert np.isnan(got[k][20]) and pb.same_bits(got[k][keep], ref[k][keep]), k
    assert all(np.isnan(x).any() for x in got["grads"][:-1]) and np.isnan(got["stats"][3])
    g.close()
    pol.close()


# ---- refusals that need a handle -----------------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle_or_the_policy():
    from fleetrl_amd import DevicePPOGrad, DevicePolicy, FleetHipError

    c, pol, g, params = open_case("5x3-one-layer", max_batch=16)
    assert g.describe() == {"max_batch": 16, "scratch_bytes": g.describe()["scratch_bytes"], "tile_rows": 16} and g.tile_rows == pol.tile_rows
    # one tile of: delta [16][64] per head, ls [16][64], part [1][8]
    assert g.describe()["scratch_bytes"] == 4 * (3 * 16 * 64 + 8)
    with pytest.raises(FleetHipError, match="B must be at most max_batch = 16, got 17"):
        run(g, c, 17, params)
    with pytest.raises(ValueError, match="expected 5 parameters"):
        g.grad(Batch(c, 4), params[-1], 0.2, 0.5, 0.0, into=params[:-1])
    import ctypes as C

    from fleetrl_amd import _capi

    a = _capi.FleetPpoGradArgs()
    a.B, a.clip_range = 4, 0.2
    a.obs = a.actions = a.old_log_prob = a.advantages = a.returns = a.log_std = a.stats = params[0].data_ptr()
    with pytest.raises(FleetHipError, match="expected 5 gradient tensors"):
        g.grad_dev(a, (C.c_void_p * 4)(*[params[0].data_ptr()] * 4), 4)
    one_head = DevicePolicy(c["actor"], activation="tanh", output="clip")
    with pytest.raises(FleetHipError, match="fleet_ppo_create: the policy has one head"):
        DevicePPOGrad(one_head, 16)
    wide = DevicePolicy(c["actor"], critic_layers=c["actor"], activation="tanh", output="clip")
    with pytest.raises(FleetHipError, match="the critic's last width must be 1, got 3"):
        DevicePPOGrad(wide, 16)
    for h in (one_head, wide, g, pol):
        h.close()
