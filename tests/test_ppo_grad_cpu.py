"""PPO's minibatch gradients without a GPU: the C ABI's section, bindings and struct layouts against a compiled probe, every refusal
that needs no device, the float64 model of tests/ppo_model.py against torch float64 autograd of SB3's own loss expression, known
answers for the clip rule, and the conditions every case of the GPU table must meet."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ppo_model as ppm

torch = pytest.importorskip("torch")

ROOT = ppm.ROOT
ENTRIES = ("fleet_ppo_create", "fleet_ppo_destroy", "fleet_ppo_last_error", "fleet_ppo_describe", "fleet_ppo_grad_dev")
ARG_FIELDS = ["struct_bytes", "B", "obs", "actions", "old_log_prob", "advantages", "returns", "log_std", "clip_range", "vf_coef", "ent_coef",
              "reserved", "values", "log_prob", "stats"]
PARAM_FIELDS = ["struct_bytes", "max_batch"]
TITLE = "PPO minibatch gradients on the device"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_is_the_last_one_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_ppo_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.PPO_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    assert hdr.index("TD3 / DDPG learning targets on the device") < hdr.index("int fleet_qtarget_describe(") < hdr.index(TITLE)
    section = hdr[hdr.index(TITLE):]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    assert "} FleetPpoParams;" in section and "} FleetPpoGradArgs;" in section
    assert not re.search(r"^/\* ---- ", section[len(TITLE):], flags=re.M)  # no section behind it
    for said in ("alive = (ratio >= lo && ratio <= hi) || s1 < s2", "fmaf(d[b][j], x[b][k], acc)", "OVERWRITTEN", "0.9189385332f",
                 "must outlive", "POLICY's stream", "it does reach the gradients"):
        assert said in section, said
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_ppo_grad_dev.argtypes) == 4 and len(lib.fleet_ppo_create.argtypes) == 3 and len(lib.fleet_ppo_describe.argtypes) == 4


def test_no_entry_carries_another_familys_prefix_and_the_class_is_exported():
    import fleetrl_amd
    from fleetrl_amd import _capi, build

    for other in (_capi.POLICY_SYMBOLS, _capi.EXPLORE_SYMBOLS, _capi.ROLLOUT_SYMBOLS, _capi.QTARGET_SYMBOLS):
        assert not set(other) & set(_capi.PPO_SYMBOLS)
    assert all(n.startswith("fleet_ppo_") for n in _capi.PPO_SYMBOLS)
    assert "fleet_ppo.hip" in build.SOURCES
    assert fleetrl_amd.DevicePPOGrad.__name__ == "DevicePPOGrad" and fleetrl_amd.DevicePPOGrad._prefix == "ppo"


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetPpoGradArgs", _capi.FleetPpoGradArgs, ARG_FIELDS), ("FleetPpoParams", _capi.FleetPpoParams, PARAM_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert C.sizeof(_capi.FleetPpoParams) == 8 and C.sizeof(_capi.FleetPpoGradArgs) == 96 and _capi.FleetPpoGradArgs.clip_range.offset == 56


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetPpoGradArgs()
    a.struct_bytes, a.B, a.clip_range, a.vf_coef, a.ent_coef = C.sizeof(a), 4, 0.2, 0.5, 0.0
    a.obs = a.actions = a.old_log_prob = a.advantages = a.returns = a.log_std = a.stats = 256  # (never dereferenced: nothing is launched)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grads(n=5, null_at=None):
    return (C.c_void_p * n)(*[None if i == null_at else 256 for i in range(n)])


GRAD_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=8), "struct_bytes"),
    "B-0": (dict(B=0), "B must be >= 1, got 0"),
    "B-negative": (dict(B=-3), "B must be >= 1, got -3"),
    "null-obs": (dict(obs=None), "null obs"),
    "null-actions": (dict(actions=None), "null actions"),
    "null-old_log_prob": (dict(old_log_prob=None), "null old_log_prob"),
    "null-advantages": (dict(advantages=None), "null advantages"),
    "null-returns": (dict(returns=None), "null returns"),
    "null-log_std": (dict(log_std=None), "null log_std"),
    "null-stats": (dict(stats=None), "null stats"),
    "clip-0": (dict(clip_range=0.0), "clip_range must be in (0, 1)"),
    "clip-1": (dict(clip_range=1.0), "clip_range must be in (0, 1)"),
    "clip-negative": (dict(clip_range=-0.2), "clip_range must be in (0, 1)"),
    "clip-nan": (dict(clip_range=float("nan")), "clip_range must be in (0, 1)"),
    "vf-nan": (dict(vf_coef=float("nan")), "vf_coef is NaN"),
    "ent-nan": (dict(ent_coef=float("nan")), "ent_coef is NaN"),
}


@pytest.mark.parametrize("case", sorted(GRAD_REFUSALS))
def test_grad_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_ppo_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = GRAD_REFUSALS[case]
    assert lib.fleet_ppo_grad_dev(None, C.byref(_args(**fields)), _grads(), 5) == _capi.ERR_INVALID
    why = lib.fleet_ppo_last_error(None).decode()
    assert why.startswith("fleet_ppo_grad_dev: ") and word in why, why


def test_grad_refuses_null_structs_arrays_and_counts_and_names_the_null_handle():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_ppo_last_error(None).decode()  # noqa: E731
    assert lib.fleet_ppo_grad_dev(None, None, _grads(), 5) == _capi.ERR_INVALID and "null FleetPpoGradArgs" in last()
    assert lib.fleet_ppo_grad_dev(None, C.byref(_args()), None, 5) == _capi.ERR_INVALID and "null grads" in last()
    assert lib.fleet_ppo_grad_dev(None, C.byref(_args()), _grads(), 0) == _capi.ERR_INVALID and "count" in last()
    assert lib.fleet_ppo_grad_dev(None, C.byref(_args()), _grads(18), 18) == _capi.ERR_INVALID and "count" in last()  # above 2 * 2 * 4 + 1
    assert lib.fleet_ppo_grad_dev(None, C.byref(_args()), _grads(null_at=3), 5) == _capi.ERR_INVALID and "gradient tensor 3 is null" in last()
    assert lib.fleet_ppo_grad_dev(None, C.byref(_args()), _grads(), 5) == _capi.ERR_INVALID
    assert last() == "fleet_ppo_grad_dev: null handle"
    # the optional outputs may be given, and every coefficient that is a number passes
    ok = _args(values=256, log_prob=256, vf_coef=0.0, ent_coef=-1.0, clip_range=0.999)
    assert lib.fleet_ppo_grad_dev(None, C.byref(ok), _grads(), 5) == _capi.ERR_INVALID and last() == "fleet_ppo_grad_dev: null handle"


def test_create_refuses_bad_parameters_before_it_looks_at_the_policy():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_ppo_last_error(None).decode()  # noqa: E731
    h = C.c_void_p()
    good = _capi.FleetPpoParams(C.sizeof(_capi.FleetPpoParams), 64)
    for p, word in ((None, "null FleetPpoParams"), (_capi.FleetPpoParams(4, 64), "struct_bytes"), (_capi.FleetPpoParams(8, 0), "max_batch"),
                    (_capi.FleetPpoParams(8, (1 << 24) + 1), "max_batch"), (good, "null policy")):
        assert lib.fleet_ppo_create(None, C.byref(p) if p is not None else None, C.byref(h)) == _capi.ERR_INVALID and not h
        assert last().startswith("fleet_ppo_create: ") and word in last(), last()
    assert lib.fleet_ppo_create(None, C.byref(good), None) == _capi.ERR_INVALID and "null output handle" in last()
    assert lib.fleet_ppo_destroy(None) == _capi.OK
    assert lib.fleet_ppo_describe(None, None, None, None) == _capi.ERR_INVALID


# ---- the model against autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_analytic_gradients_equal_float64_autograd_of_sb3s_loss(name):
    """Both sides are float64 and the operations are the same: rounding noise separates them, 1e-12 relative."""
    for B in ppm.CASES[name][5]:
        m, t = ppm.model(name, B), ppm.torch_loss_and_grads(*ppm.batch_args(ppm.case(name), B))
        assert len(m["grads"]) == len(t["grads"]) == len(ppm.tensor_names(name))
        for n, g, r in zip(ppm.tensor_names(name), m["grads"], t["grads"]):
            assert g.shape == r.shape and g.dtype == np.float64
            assert np.abs(g - r).max() <= 1e-12 * max(np.abs(r).max(), 1e-300), (name, B, n)
        for k in ppm.STATS:
            assert abs(m["stats"][k] - t["stats"][k]) <= 1e-12 * max(abs(t["stats"][k]), 1.0), (name, B, k)


# ---- known answers for the clip rule ---------------------------------------------------------------------------------------------------
def _one_row(ratio, adv, c=0.25):
    """D = A = 1, one-layer heads: mean = x, v = 0; a = mean, log_std = 0, so lp = -0.9189..., and old sets the ratio.  The
    gradient of the loss in the actor's BIAS is then -(adv * ratio) * d lp / d mean = 0 at a = mean -- so the action sits one
    standard deviation off: d lp / d mean = 1 and dL/db = glp."""
    one = lambda w, b: [(np.array([[w]], np.float32), np.array([b], np.float32))]  # noqa: E731
    lp = -0.5 - 0.5 * np.log(2 * np.pi)
    m = ppm.loss_and_grads(one(1.0, 0.0), one(0.0, 0.0), "tanh", [0.0], [[0.5]], [[1.5]], [lp - np.log(ratio)], [adv], [0.0], clip_range=c,
                           vf_coef=0.0, ent_coef=0.0)
    assert abs(m["ratio"][0] - ratio) < 1e-12
    return m["grads"][1][0], bool(m["alive"][0]), m["stats"]["policy_loss"]


def test_known_answers_inside_the_range_give_the_full_gradient_through_the_tie():
    for adv in (2.0, -2.0):
        g, alive, pl = _one_row(1.125, adv)
        assert alive and g == pytest.approx(-adv * 1.125, rel=1e-12) and pl == pytest.approx(-adv * 1.125, rel=1e-12)


@pytest.mark.parametrize("ratio,adv,alive", [(1.5, 2.0, False), (1.5, -2.0, True), (0.5, 2.0, True), (0.5, -2.0, False)])
def test_known_answers_outside_the_range(ratio, adv, alive):
    """adv > 0 above the range and adv < 0 below it are clipped to zero gradient; the other two keep the unclipped branch."""
    g, is_alive, pl = _one_row(ratio, adv)
    assert is_alive is alive
    cl = min(max(ratio, 0.75), 1.25)
    assert pl == pytest.approx(-min(adv * ratio, adv * cl), rel=1e-12)
    assert g == (pytest.approx(-adv * ratio, rel=1e-12) if alive else 0.0)


def test_known_answers_on_a_bound_keep_the_gradient_as_torch_does():
    """clamp passes its gradient ON a bound and min splits a tie evenly: the full gradient, for either sign -- and autograd agrees."""
    for bound, adv in ((1.25, 2.0), (1.25, -2.0), (0.75, 2.0), (0.75, -2.0)):
        r = torch.tensor([bound], dtype=torch.float64, requires_grad=True)
        a = torch.tensor([adv], dtype=torch.float64)
        (-torch.min(a * r, a * torch.clamp(r, 0.75, 1.25)).mean()).backward()
        assert r.grad.item() == -adv
        lo, hi = 0.75, 1.25
        s1, s2 = adv * bound, adv * min(max(bound, lo), hi)
        assert (lo <= bound <= hi) or s1 < s2  # the header's `alive`


def test_the_alive_rule_equals_autograd_on_a_grid_of_ratios_and_advantages():
    ratios = np.array([0.3, 0.75, 0.75 + 1e-9, 0.9, 1.0, 1.2, 1.25 - 1e-9, 1.25, 1.7])
    for adv in (-3.0, -1e-3, 0.0, 1e-3, 3.0):
        r = torch.tensor(ratios, requires_grad=True)
        a = torch.full_like(r, adv)
        (-torch.min(a * r, a * torch.clamp(r, 0.75, 1.25)).sum()).backward()
        s1, s2 = adv * ratios, adv * np.clip(ratios, 0.75, 1.25)
        alive = ((ratios >= 0.75) & (ratios <= 1.25)) | (s1 < s2)
        assert np.array_equal(r.grad.numpy(), np.where(alive, -adv, 0.0) + 0.0), adv


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------
def test_the_case_table_covers_what_it_must():
    assert {(c[0], c[1]) for c in ppm.CASES.values()} == {(5, 3), (127, 2), (129, 65), (45, 3), (388, 50)}
    assert ppm.BATCHES == (1, 16, 17, 33) and ppm.ROWS == 33
    assert ppm.CASES["388x50-400-300-tanh"][5] == (33,) and all(c[5] == ppm.BATCHES for n, c in ppm.CASES.items() if not n.startswith("388"))
    assert ppm.CASES["129x65-65-63-relu"][2:5] == ((65, 63), (65, 63), "relu")
    assert ppm.CASES["45x3-deep-actor"][2:4] == ((33, 130, 70), ()) and ppm.CASES["5x3-one-layer"][2:4] == ((), ())
    assert (ppm.CLIP_RANGE, ppm.VF_COEF) == (0.2, 0.5) and ppm.ENT_COEF != 0


@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_every_case_meets_the_tables_conditions(name):
    c = ppm.case(name)
    facts = ppm.facts_of(c)
    assert all(facts.values()) and 0 <= c["salt"] < ppm.MAX_SALT, facts
    assert ("no relu pre-activation within 1e-5 of zero" in facts) == (c["activation"] == "relu")
    m = ppm.model(name, ppm.ROWS)
    inside = np.abs(m["ratio"] - 1.0) <= ppm.CLIP_RANGE
    print(f"{name}: salt {c['salt']}, {int(inside.sum())} of {ppm.ROWS} rows inside the range, {int((~m['alive']).sum())} dead")
    assert all(np.isfinite(g).all() for g in m["grads"])


# ---- the entries that look at their arguments before their handle, across the families ---------------------------------------------
NULL_HANDLE_REFUSALS = {
    "fleet_ppo_grad_dev": ("ppo", (None, None, 0), "null FleetPpoGradArgs"),
    "fleet_td3_critic_grad_dev": ("td3", (None, None, 0), "null FleetTd3CriticArgs"),
    "fleet_td3_actor_grad_dev": ("td3", (None, None, 0), "null FleetTd3ActorArgs"),
    "fleet_adam_step_dev": ("adam", (None, None, None, 0), "null FleetAdamStepArgs"),
    "fleet_adam_state_dev": ("adam", (7, None, None, 0, None), "unknown mode 7"),
    "fleet_adam_export_image_dev": ("adam", (None, 0), "null handle"),
    "fleet_qtarget_target_dev": ("qtarget", (None, None, None, 0, None), "null FleetQTargetArgs"),
}


def test_a_null_handles_refusal_lands_in_its_own_familys_string_and_in_no_other():
    """The seven entries share one opening (fleet_handle.h); the thread-local strings stay one per family."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    families = sorted({f for f, _, _ in NULL_HANDLE_REFUSALS.values()})
    last = lambda: {f: getattr(lib, f"fleet_{f}_last_error")(None).decode() for f in families}  # noqa: E731
    for entry, (family, args, why) in sorted(NULL_HANDLE_REFUSALS.items()):
        before = last()
        assert before[family] != f"{entry}: {why}"  # (the entry before this one left another message)
        assert getattr(lib, entry)(None, *args) == _capi.ERR_INVALID
        after = last()
        assert after.pop(family) == f"{entry}: {why}", entry
        before.pop(family)
        assert after == before, entry
