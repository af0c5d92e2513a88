"""PPO's value-function clipping in the gradient launches (fleet_ppo_grad_vclip_dev): against the float64 model of
tests/ppo_vclip_model.py under the project's rule, bit for bit against fleet_ppo_grad_dev wherever the clip may not reach, the tie
rule where the arithmetic is exact, and what a result may not depend on."""
import json
import os

import numpy as np
import pytest

import policy_bits as pb
import ppo_model as ppm
import ppo_vclip_model as vcm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(vcm.ROOT, "profiles", "ppo_vclip_parity.json")
CV = vcm.CLIP_RANGE_VF
_parity = {}


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


class Batch:
    def __init__(self, c, B, rows=None):
        """The first B rows of a case on the device; rows > B: buffers of that many rows whose tail is NaN."""
        for k, name in (("obs", "observations"), ("actions", "actions"), ("old_log_prob", "old_log_prob"), ("advantages", "advantages"),
                        ("returns", "returns"), ("old_values", "old_values")):
            a = np.array(c[k][:B])
            if rows and rows > B:
                a = np.concatenate([a, np.full((rows - B, *a.shape[1:]), np.nan, a.dtype)])
            setattr(self, name, on_device(a)[:B])  # (a view of the first B rows: the NaN rows lie behind it in memory)


def open_case(c, max_batch):
    from fleetrl_amd import DevicePolicy, DevicePPOGrad

    pol = DevicePolicy(c["actor"], critic_layers=c["critic"], activation=c["activation"], output="clip")
    flat = [t for net in (c["actor"], c["critic"]) for w, b in net for t in (w, b)] + [c["log_std"]]
    return pol, DevicePPOGrad(pol, max_batch), [torch.nn.Parameter(on_device(t)) for t in flat]


def run(g, c, B, params, cv, *, rows=None, vf_coef=ppm.VF_COEF):
    """One call -> {"grads": [...], "stats", "values", "log_prob"} as host arrays; cv None: the unclipped entry."""
    values, log_prob = (torch.full((B,), np.nan, device=dev()) for _ in range(2))
    for p in params:
        p.grad = torch.full_like(p, np.nan)
    stats = g.grad(Batch(c, B, rows), params[-1], ppm.CLIP_RANGE, vf_coef, ppm.ENT_COEF, into=params, values_out=values,
                   log_prob_out=log_prob, clip_range_vf=cv)
    return {"grads": [host(p.grad).copy() for p in params], "stats": host(stats).copy(), "values": host(values), "log_prob": host(log_prob)}


def same(a, b):
    return all(pb.same_bits(x, y) for x, y in zip(a["grads"], b["grads"])) and all(pb.same_bits(a[k], b[k]) for k in ("stats", "values", "log_prob"))


# ---- the float64 model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_gradients_and_statistics_stay_within_eight_times_the_float32_reference_error(name):
    """The project's rule: within 8 * max(eps_ref, 2^-24 * max |ref|) of the float64 model, per gradient tensor and per statistic;
    eps_ref = |torch-CPU float32 autograd of SB3's clipped expression - the model|.  Every error / bound ratio goes to
    profiles/ppo_vclip_parity.json."""
    c = vcm.case(name)
    assert all(vcm.facts_of(name, c["old_values"]).values())
    pol, g, params = open_case(c, ppm.ROWS)
    worst, bad = 0.0, []
    for B in ppm.CASES[name][5]:
        got, m, r = run(g, c, B, params, CV), vcm.model(name, B), vcm.reference32(name, B)
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
        json.dump({"bound": "8 * max(eps_ref, 2^-24 * max|ref|)", "clip_range_vf": CV,
                   "worst": max(v["err_over_bound"] for v in _parity.values()), "cases": dict(sorted(_parity.items()))}, fh, indent=1)
    assert not bad, bad


# ---- against the unclipped entry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_everything_the_clip_may_not_reach_equals_the_unclipped_entry_bit_for_bit_and_the_critic_differs(name):
    c = vcm.case(name)
    pol, g, params = open_case(c, ppm.ROWS)
    na = 2 * len(c["actor"])
    for B in ppm.CASES[name][5]:
        plain, clipped = run(g, c, B, params, None), run(g, c, B, params, CV)
        for i in list(range(na)) + [len(params) - 1]:  # every actor tensor, the log_std gradient
            assert pb.same_bits(clipped["grads"][i], plain["grads"][i]), (name, B, ppm.tensor_names(name)[i])
        assert pb.same_bits(clipped["stats"][[0, 2, 4, 5, 6, 7]], plain["stats"][[0, 2, 4, 5, 6, 7]]), (name, B)
        assert pb.same_bits(clipped["values"], plain["values"]) and pb.same_bits(clipped["log_prob"], plain["log_prob"]), (name, B)
        m = vcm.model(name, B)
        if not m["inside"].all():  # (B = 1 may hold an inside row alone; from B = 16 on the table's conditions put a clipped row in)
            for i in range(na, len(params) - 1):
                assert not pb.same_bits(clipped["grads"][i], plain["grads"][i]), (name, B, ppm.tensor_names(name)[i])
            assert clipped["stats"][1] != plain["stats"][1] and clipped["stats"][3] != plain["stats"][3], (name, B)
        assert B < 16 or not m["inside"].all()
    g.close()
    pol.close()


# ---- where the arithmetic is exact ---------------------------------------------------------------------------------------------------
def test_the_two_ties_pass_their_gradient_bit_for_bit_with_torch_float32():
    """v == 0.5 exactly, cv = 0.25, old = 0.25, 0.75, 0.0, 1.0, vf_coef = 0.5, B = 4: the critic-bias gradient is a sum of four exactly
    representable terms (two of them zero), so the device, torch-CPU float32 and the float64 model hold the same number."""
    c = vcm.tie_case()
    pol, g, params = open_case(c, 4)
    got = run(g, c, 4, params, vcm.TIE_CV, vf_coef=0.5)
    args = (c["actor"], c["critic"], "tanh", c["log_std"], c["obs"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"],
            c["old_values"])
    t = vcm.torch_loss_and_grads(*args, clip_range_vf=vcm.TIE_CV, vf_coef=0.5, dtype="float32")
    assert pb.same_bits(got["values"], np.full(4, 0.5, np.float32))
    assert pb.same_bits(got["grads"][3], t["grads"][3].astype(np.float32)) and got["grads"][3].tolist() == [0.125]
    # dW = fmaf chain of dv[b] * obs[b]: dv = -0.125, 0.25, 0, 0 -- products by powers of two, one rounding in the sum, as torch's
    assert pb.same_bits(got["grads"][2], t["grads"][2].astype(np.float32))
    m = vcm.loss_and_grads(*args, clip_range_vf=vcm.TIE_CV, vf_coef=0.5)
    assert got["stats"][1] == np.float32(m["stats"]["value_loss"])  # (0.25 + 1.0 + 3.0625 + 0.25) / 4, exact
    g.close()
    pol.close()


# ---- what a result does not depend on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["129x65-65-63-relu", "45x3-deep-actor"])
def test_a_result_depends_on_the_inputs_and_b_and_on_nothing_else(name):
    from fleetrl_amd import DevicePPOGrad

    c = vcm.case(name)
    pol, g, params = open_case(c, 16)
    B = 16
    ref = run(g, c, B, params, CV)
    assert all(np.isfinite(x).all() for x in ref["grads"]) and np.isfinite(ref["stats"]).all()
    assert same(run(g, c, B, params, CV), ref)  # the run
    big = DevicePPOGrad(pol, 64)  # the capacity of the scratch
    assert same(run(big, c, B, params, CV), ref)
    assert same(run(big, c, B, params, CV, rows=ppm.ROWS), ref)  # NaN rows behind row 16 in every buffer, old values included
    run(big, c, ppm.ROWS, params, CV)  # a larger batch in between leaves the scratch's rows 16.. filled
    assert same(run(big, c, B, params, CV), ref)
    big.close()
    g.close()
    pol.close()


# ---- refusals that need the handle ---------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle():
    import ctypes as C

    from fleetrl_amd import FleetHipError, _capi

    c = vcm.case("5x3-one-layer")
    pol, g, params = open_case(c, 16)
    with pytest.raises(FleetHipError, match="fleet_ppo_grad_vclip_dev: B must be at most max_batch = 16, got 17"):
        run(g, c, 17, params, CV)
    a = _capi.FleetPpoGradVclipArgs()
    a.clip_range_vf, a.old_values = CV, params[0].data_ptr()
    b = a.base
    b.B, b.clip_range = 4, 0.2
    b.obs = b.actions = b.old_log_prob = b.advantages = b.returns = b.log_std = b.stats = params[0].data_ptr()
    with pytest.raises(FleetHipError, match="fleet_ppo_grad_vclip_dev: expected 5 gradient tensors"):
        g.grad_vclip_dev(a, (C.c_void_p * 4)(*[params[0].data_ptr()] * 4), 4)
    with pytest.raises(ValueError, match="`clip_range_vf` must be positive"):
        run(g, c, 4, params, 0.0)
    assert same(run(g, c, 16, params, CV), run(g, c, 16, params, CV))  # and the handle works on after the refusals
    g.close()
    pol.close()
