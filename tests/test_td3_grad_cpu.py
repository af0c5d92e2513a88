"""TD3's minibatch gradients without a GPU: the C ABI's section, bindings and struct layouts against a compiled probe, every refusal
that needs no device, the float64 model of tests/td3_model.py against torch float64 autograd of SB3's own loss expressions, known
answers that tell the likely mistakes apart, and the conditions every case of the GPU table must meet."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import td3_model as tm

torch = pytest.importorskip("torch")

ROOT = tm.ROOT
ENTRIES = ("fleet_td3_create", "fleet_td3_destroy", "fleet_td3_last_error", "fleet_td3_describe", "fleet_td3_critic_grad_dev",
           "fleet_td3_actor_grad_dev")
CRITIC_FIELDS = ["struct_bytes", "B", "obs", "actions", "target_q", "q", "stats", "reserved"]
ACTOR_FIELDS = ["struct_bytes", "B", "obs", "actions_out", "q", "stats", "reserved"]
PARAM_FIELDS = ["struct_bytes", "max_batch"]
TITLE = "TD3 / DDPG minibatch gradients on the device"
PPO_TITLE = "PPO minibatch gradients on the device"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_lies_between_the_targets_and_ppo_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_td3_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.TD3_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    assert hdr.count(TITLE) == 1 and hdr.count(PPO_TITLE) == 1
    assert hdr.index("int fleet_qtarget_describe(") < hdr.index(TITLE) < hdr.index(PPO_TITLE)
    section = hdr[hdr.index(TITLE):hdr.index(PPO_TITLE)]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    for struct in ("} FleetTd3Params;", "} FleetTd3CriticArgs;", "} FleetTd3ActorArgs;"):
        assert struct in section
    assert not re.search(r"^(?:int|const char\*)\s+fleet_(?:qtarget|ppo)_", section, flags=re.M)  # no entry of a neighbour in it
    assert len(re.findall(r"^/\* ---- ", section[len(TITLE):], flags=re.M)) == 1  # the next section's opening, and none between
    for said in ("e_c  = q_c - y[b];  dq_c = (2.0f * invB) * e_c", "dq = -invB", "fmaf(Wt0[D + j][i], d0[i], acc)", "fmaf(-a, a, 1.0f)",
                 "(mean >= lo && mean <= hi) ? 1 : 0", "obs[b][k] for k < D and actions[b][k - D] behind it", "fmaf(d[b][j], x[b][k], acc)",
                 "[0] = [1] + [2]", "[0] = -(total(q) * invB)", "OVERWRITTEN", "must outlive", "ONLINE", "NETWORKS handle's stream",
                 "it does reach the", "No critic gradient is produced"):
        assert said in section, said
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_td3_critic_grad_dev.argtypes) == 4 and len(lib.fleet_td3_actor_grad_dev.argtypes) == 4
    assert len(lib.fleet_td3_create.argtypes) == 3 and len(lib.fleet_td3_describe.argtypes) == 4


def test_no_entry_carries_another_familys_prefix_and_the_class_is_exported():
    import fleetrl_amd
    from fleetrl_amd import _capi, build

    for other in (_capi.POLICY_SYMBOLS, _capi.EXPLORE_SYMBOLS, _capi.ROLLOUT_SYMBOLS, _capi.QTARGET_SYMBOLS, _capi.PPO_SYMBOLS):
        assert not set(other) & set(_capi.TD3_SYMBOLS)
    assert all(n.startswith("fleet_td3_") for n in _capi.TD3_SYMBOLS)
    assert "fleet_td3.hip" in build.SOURCES and "fleet_grad_dev.h" in build.HEADERS and "fleet_qtarget.h" in build.HEADERS
    assert fleetrl_amd.DeviceTD3Grad.__name__ == "DeviceTD3Grad" and fleetrl_amd.DeviceTD3Grad._prefix == "td3"


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetTd3CriticArgs", _capi.FleetTd3CriticArgs, CRITIC_FIELDS),
                               ("FleetTd3ActorArgs", _capi.FleetTd3ActorArgs, ACTOR_FIELDS), ("FleetTd3Params", _capi.FleetTd3Params, PARAM_FIELDS)):
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
    assert C.sizeof(_capi.FleetTd3Params) == 8 and C.sizeof(_capi.FleetTd3CriticArgs) == 56 and C.sizeof(_capi.FleetTd3ActorArgs) == 48


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _critic(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetTd3CriticArgs()
    a.struct_bytes, a.B = C.sizeof(a), 4
    a.obs = a.actions = a.target_q = a.stats = 256  # (never dereferenced: nothing is launched)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _actor(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetTd3ActorArgs()
    a.struct_bytes, a.B = C.sizeof(a), 4
    a.obs = a.stats = 256
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _grads(n=4, null_at=None):
    return (C.c_void_p * n)(*[None if i == null_at else 256 for i in range(n)])


CRITIC_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=8), "struct_bytes"),
    "B-0": (dict(B=0), "B must be >= 1, got 0"),
    "B-negative": (dict(B=-3), "B must be >= 1, got -3"),
    "null-obs": (dict(obs=None), "null obs"),
    "null-actions": (dict(actions=None), "null actions"),
    "null-target_q": (dict(target_q=None), "null target_q"),
    "null-stats": (dict(stats=None), "null stats"),
    "reserved": (dict(reserved=1), "reserved must be 0"),
}
ACTOR_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=56), "struct_bytes"),
    "B-0": (dict(B=0), "B must be >= 1, got 0"),
    "B-negative": (dict(B=-1), "B must be >= 1, got -1"),
    "null-obs": (dict(obs=None), "null obs"),
    "null-stats": (dict(stats=None), "null stats"),
    "reserved": (dict(reserved=1 << 40), "reserved must be 0"),
}


@pytest.mark.parametrize("case", sorted(CRITIC_REFUSALS))
def test_critic_entry_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_td3_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = CRITIC_REFUSALS[case]
    assert lib.fleet_td3_critic_grad_dev(None, C.byref(_critic(**fields)), _grads(), 4) == _capi.ERR_INVALID
    why = lib.fleet_td3_last_error(None).decode()
    assert why.startswith("fleet_td3_critic_grad_dev: ") and word in why, why


@pytest.mark.parametrize("case", sorted(ACTOR_REFUSALS))
def test_actor_entry_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = ACTOR_REFUSALS[case]
    assert lib.fleet_td3_actor_grad_dev(None, C.byref(_actor(**fields)), _grads(), 4) == _capi.ERR_INVALID
    why = lib.fleet_td3_last_error(None).decode()
    assert why.startswith("fleet_td3_actor_grad_dev: ") and word in why, why


@pytest.mark.parametrize("entry", ["critic", "actor"])
def test_entries_refuse_null_structs_and_arrays_and_name_the_null_handle(entry):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fn = getattr(lib, f"fleet_td3_{entry}_grad_dev")
    make = _critic if entry == "critic" else _actor
    struct = "FleetTd3CriticArgs" if entry == "critic" else "FleetTd3ActorArgs"
    last = lambda: lib.fleet_td3_last_error(None).decode()  # noqa: E731
    assert fn(None, None, _grads(), 4) == _capi.ERR_INVALID and f"null {struct}" in last()
    assert fn(None, C.byref(make()), None, 4) == _capi.ERR_INVALID and "null grads" in last()
    assert fn(None, C.byref(make()), _grads(), 0) == _capi.ERR_INVALID and "count" in last()
    assert fn(None, C.byref(make()), _grads(25), 25) == _capi.ERR_INVALID and "count" in last()  # above 2 * 3 * 4
    assert fn(None, C.byref(make()), _grads(null_at=3), 4) == _capi.ERR_INVALID and "gradient tensor 3 is null" in last()
    assert fn(None, C.byref(make()), _grads(), 4) == _capi.ERR_INVALID and last() == f"fleet_td3_{entry}_grad_dev: null handle"
    ok = make(q=256) if entry == "critic" else make(q=256, actions_out=256)  # the optional outputs may be given
    assert fn(None, C.byref(ok), _grads(), 4) == _capi.ERR_INVALID and last() == f"fleet_td3_{entry}_grad_dev: null handle"


def test_create_refuses_bad_parameters_before_it_looks_at_the_networks():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_td3_last_error(None).decode()  # noqa: E731
    h = C.c_void_p()
    good = _capi.FleetTd3Params(C.sizeof(_capi.FleetTd3Params), 64)
    for p, word in ((None, "null FleetTd3Params"), (_capi.FleetTd3Params(4, 64), "struct_bytes"), (_capi.FleetTd3Params(8, 0), "max_batch"),
                    (_capi.FleetTd3Params(8, (1 << 24) + 1), "max_batch"), (good, "null networks handle")):
        assert lib.fleet_td3_create(None, C.byref(p) if p is not None else None, C.byref(h)) == _capi.ERR_INVALID and not h
        assert last().startswith("fleet_td3_create: ") and word in last(), last()
    assert lib.fleet_td3_create(None, C.byref(good), None) == _capi.ERR_INVALID and "null output handle" in last()
    assert lib.fleet_td3_destroy(None) == _capi.OK
    assert lib.fleet_td3_describe(None, None, None, None) == _capi.ERR_INVALID


# ---- the model against autograd ------------------------------------------------------------------------------------------------------
def _close(names, got, want, where):
    assert len(got) == len(want) == len(names), where
    for n, g, r in zip(names, got, want):
        assert g.shape == r.shape and g.dtype == np.float64
        assert np.abs(g - r).max() <= 1e-12 * max(np.abs(r).max(), 1e-300), (*where, n)


@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_analytic_gradients_equal_float64_autograd_of_sb3s_losses(name):
    """Both sides are float64 and the operations are the same: rounding noise separates them, 1e-12 relative."""
    c, names = tm.case(name), tm.tensor_names(name)
    for B in tm.CASES[name][7]:
        m = tm.model(name, B)
        tc, ta = tm.torch_critic_loss_and_grads(*tm.critic_args(c, B)), tm.torch_actor_loss_and_grads(*tm.actor_args(c, B))
        _close(names["critic"], m["critic"]["grads"], tc["grads"], (name, B))
        _close(names["actor"], m["actor"]["grads"], ta["grads"], (name, B))
        for k in tm.CRITIC_STATS:
            assert abs(m["critic"]["stats"][k] - tc["stats"][k]) <= 1e-12 * max(abs(tc["stats"][k]), 1.0), (name, B, k)
        assert abs(m["actor"]["stats"]["actor_loss"] - ta["stats"]["actor_loss"]) <= 1e-12 * max(abs(ta["stats"]["actor_loss"]), 1.0)


# ---- known answers -------------------------------------------------------------------------------------------------------------------
def _one(w, b):
    return [(np.array(w, np.float32), np.array(b, np.float32))]


def test_known_answer_the_critic_gradient_carries_two_over_b_and_the_loss_sums_over_the_critics():
    """One-layer critics over D = A = 1 with zero weights: q = b.  Three equal rows, y = 0: e_0 = 1, e_1 = 2.  dL/db_c = (2 / B) *
    sum_b e_c = 2 e_c (1 / B would give e_c); the loss is 1 + 4 = 5 (the mean over the critics would be 2.5)."""
    critics = [_one([[0.0, 0.0]], [1.0]), _one([[0.0, 0.0]], [2.0])]
    obs, act, y = np.full((3, 1), 3.0, np.float32), np.full((3, 1), 7.0, np.float32), np.zeros(3, np.float32)
    m = tm.critic_loss_and_grads(critics, "relu", obs, act, y)
    assert m["grads"][1][0] == pytest.approx(2.0, rel=1e-12) and m["grads"][3][0] == pytest.approx(4.0, rel=1e-12)
    assert m["stats"] == {"critic_loss": pytest.approx(5.0), "critic_0_loss": pytest.approx(1.0), "critic_1_loss": pytest.approx(4.0)}
    t = tm.torch_critic_loss_and_grads(critics, "relu", obs, act, y)
    assert t["stats"]["critic_loss"] == pytest.approx(5.0) and t["grads"][1][0] == pytest.approx(2.0)
    one = tm.critic_loss_and_grads(critics[:1], "relu", obs, act, y)["stats"]
    assert one["critic_loss"] == one["critic_0_loss"] == pytest.approx(1.0) and one["critic_1_loss"] == 0.0


def test_known_answer_the_first_layers_columns_are_the_observation_then_the_action():
    """B = 1, q = 1, y = 0: dq = 2; dW[0] = 2 * (obs, action) = (6, 14) -- (14, 6) had the action come first."""
    m = tm.critic_loss_and_grads([_one([[0.0, 0.0]], [1.0])], "relu", [[3.0]], [[7.0]], [0.0])
    assert np.array_equal(m["grads"][0], np.array([[6.0, 14.0]]))


@pytest.mark.parametrize("mean,g", [(0.7, 1.0), (-0.3, 1.0), (0.2, 1.0), (np.nextafter(np.float32(0.7), np.float32(1)), 0.0),
                                    (np.nextafter(np.float32(-0.3), np.float32(-1)), 0.0)])
def test_known_answer_the_clip_mask_has_inclusive_bounds_as_torchs_clamp(mean, g):
    """A one-layer actor W = 1, b = 0 over D = 1: mean = obs.  Critic 0: q = 5 a.  The actor's db = -5 g: on a bound the gradient
    passes (torch's clamp), a float32 step outside it is zero."""
    lo, hi = np.float64(np.float32(-0.3)), np.float64(np.float32(0.7))
    actor, critics = _one([[1.0]], [0.0]), [_one([[0.0, 5.0]], [0.0])]
    obs = np.array([[mean]], np.float32)
    m = tm.actor_loss_and_grads(actor, critics, "relu", "clip", lo, hi, obs)
    t = tm.torch_actor_loss_and_grads(actor, critics, "relu", "clip", float(lo), float(hi), obs)
    assert m["grads"][1][0] == -5.0 * g and t["grads"][1][0] == -5.0 * g
    assert m["stats"]["actor_loss"] == pytest.approx(-5.0 * min(max(float(obs[0, 0]), lo), hi), rel=1e-12)


def test_known_answer_the_actor_loss_runs_critic_0_and_not_critic_1():
    actor, c0, c1 = _one([[1.0]], [0.0]), _one([[0.0, 5.0]], [0.0]), _one([[0.0, -11.0]], [0.0])
    obs = np.array([[0.25], [0.5]], np.float32)
    m = tm.actor_loss_and_grads(actor, [c0, c1], "relu", "none", 0.0, 0.0, obs)
    assert m["grads"][1][0] == pytest.approx(-5.0) and m["stats"]["actor_loss"] == pytest.approx(-5.0 * 0.375)
    assert m["grads"][0][0, 0] == pytest.approx(-5.0 * 0.375)  # dW = sum_b dmean[b] * obs[b] = -(5 / 2) * (0.25 + 0.5)
    swapped = tm.actor_loss_and_grads(actor, [c1, c0], "relu", "none", 0.0, 0.0, obs)
    assert swapped["grads"][1][0] == pytest.approx(11.0)
    # the tanh output's factor: 1 - a^2
    th = tm.actor_loss_and_grads(actor, [c0], "relu", "tanh", 0.0, 0.0, obs[:1])
    assert th["grads"][1][0] == pytest.approx(-5.0 * (1.0 - np.tanh(0.25) ** 2), rel=1e-12)


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------
def test_the_case_table_covers_what_it_must():
    assert {(c[0], c[1]) for c in tm.CASES.values()} == {(5, 3), (127, 2), (126, 5), (129, 65), (45, 3), (388, 50)}
    assert tm.BATCHES == (1, 16, 17, 33) and tm.ROWS == 33
    assert tm.CASES["388x50-400-300-tanh"][7] == (33,) and all(c[7] == tm.BATCHES for n, c in tm.CASES.items() if not n.startswith("388"))
    assert tm.CASES["129x65-65-63-relu-clip"][2:6] == ((65, 63), (65, 63), "relu", "clip")
    assert tm.CASES["126x5-64-64-relu"][2:5] == ((64, 64), (64, 64), "relu") and tm.CASES["127x2-64-64-tanh"][2:5] == ((64, 64), (64, 64), "tanh")
    assert tm.CASES["45x3-deep-actor"][2:4] == ((33, 130, 70), ()) and tm.CASES["45x3-deep-critic"][2:4] == ((), (33, 130, 70))
    assert tm.CASES["5x3-one-layer"][2:4] == ((), ())
    assert {c[6] for c in tm.CASES.values()} == {1, 2} and {c[5] for c in tm.CASES.values()} == {"tanh", "clip", "none"}
    assert 127 + 2 == 129 and 126 + 5 > 128 > 126  # the seam one past the 128-column chunk, and inside the first chunk


@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_every_case_meets_the_tables_conditions(name):
    c = tm.case(name)
    facts = tm.facts_of(c)
    assert all(facts.values()) and 0 <= c["salt"] < tm.MAX_SALT, facts
    assert ("no relu pre-activation within 1e-5 of zero" in facts) == (c["activation"] == "relu")
    assert ("no mean within 1e-4 of a bound" in facts) == (c["output"] == "clip")
    m = tm.model(name, tm.ROWS)
    print(f"{name}: salt {c['salt']}, {sorted(facts)}")
    assert all(np.isfinite(g).all() for g in m["critic"]["grads"] + m["actor"]["grads"])
