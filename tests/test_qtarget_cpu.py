"""The TD3 / DDPG targets without a GPU: the C ABI's declarations and bindings, the structs' layout against a compiled probe, every
refusal that needs no device, the state-dict parser, and the model of tests/qtarget_model.py -- known answers that tell the stated
arithmetic from its near misses, the Polyak update against exact rational arithmetic, and the facts every GPU case must exercise."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import policy_bits as pb
import policy_model as pm
import qtarget_model as qm

ROOT = pm.ROOT
ENTRIES = ("fleet_qtarget_create", "fleet_qtarget_destroy", "fleet_qtarget_last_error", "fleet_qtarget_set_stream",
           "fleet_qtarget_load_host", "fleet_qtarget_load_dev", "fleet_qtarget_polyak_dev", "fleet_qtarget_export_dev",
           "fleet_qtarget_target_dev", "fleet_qtarget_describe")
ARG_FIELDS = ["struct_bytes", "noise_mode", "seed", "step", "row_offset", "reserved", "gamma", "noise_clip", "act_lo", "act_hi", "sigma",
              "noise", "target_q", "next_actions", "q"]
PARAM_FIELDS = ["struct_bytes", "obs_dim", "n_critics", "tile_rows", "actor", "critic"]
f32 = np.float32


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_is_placed_after_the_noise_section_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_qtarget_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.QTARGET_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    title = "TD3 / DDPG learning targets on the device"
    assert hdr.index("correlated action noise on the device") < hdr.index("int fleet_noise_describe(") < hdr.index(title)
    section = hdr[hdr.index(title):]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    assert "} FleetQTargetParams;" in section and "} FleetQTargetArgs;" in section
    assert "SEED OF ITS OWN" in section and "fmaf(tau32, p, t * omt32)" in section  # the two things the header must say
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_qtarget_target_dev.argtypes) == 6 and len(lib.fleet_qtarget_polyak_dev.argtypes) == 4


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetQTargetArgs", _capi.FleetQTargetArgs, ARG_FIELDS), ("FleetQTargetParams", _capi.FleetQTargetParams, PARAM_FIELDS)):
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
    assert _capi.FleetQTargetArgs.seed.offset == 8 and C.sizeof(_capi.FleetQTargetParams) == 16 + 3 * C.sizeof(_capi.FleetPolicyHead)


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _params(D=5, actor=(7, 3), critics=((8, 1), (8, 1))):
    from fleetrl_amd import _capi

    p = _capi.FleetQTargetParams()
    p.struct_bytes, p.obs_dim, p.n_critics = C.sizeof(p), D, len(critics)
    for H, widths, out in [(p.actor, actor, _capi.POLICY_OUT_TANH)] + [(p.critic[c], w, _capi.POLICY_OUT_NONE) for c, w in enumerate(critics)]:
        H.n_layers = len(widths)
        for l, w in enumerate(widths[:4]):
            H.width[l] = w
        H.activation, H.output = _capi.POLICY_ACT_RELU, out
    return p


def _create(p, weights=True):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    w = np.zeros(1 << 16, np.float32)
    h = C.c_void_p()
    rc = lib.fleet_qtarget_create(0, C.byref(p) if p is not None else None, w.ctypes.data if weights else None, C.byref(h))
    assert not h
    return rc, lib.fleet_qtarget_last_error(None).decode()


def _changed(**kw):
    p = _params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _with(fn):
    p = _params()
    fn(p)
    return p


CREATE_REFUSALS = {
    "struct_bytes": (lambda: _changed(struct_bytes=8), "struct_bytes"),
    "obs_dim-0": (lambda: _changed(obs_dim=0), "obs_dim"),
    "n_critics-0": (lambda: _changed(n_critics=0), "n_critics"),
    "n_critics-3": (lambda: _changed(n_critics=3), "n_critics"),
    "actor-layers-5": (lambda: _with(lambda p: setattr(p.actor, "n_layers", 5)), "actor: n_layers"),
    "actor-width-513": (lambda: _params(actor=(513, 3)), "actor: width of layer 0"),
    "act-dim-513": (lambda: _params(actor=(7, 513)), "width of layer 1"),
    "D+A": (lambda: _params(D=8190, actor=(3,)), "obs_dim + act_dim"),
    "critic-last-width": (lambda: _params(critics=((8, 2), (8, 1))), "critic 0: the last width must be 1"),
    "critic-1-width-0": (lambda: _params(critics=((8, 1), (0, 1))), "critic 1: width of layer 0"),
    "critic-output": (lambda: _with(lambda p: setattr(p.critic[1], "output", 2)), "critic 1: the output transform must be NONE"),
    "activation": (lambda: _with(lambda p: setattr(p.actor, "activation", 7)), "unknown activation"),
    "actor-clip-lo>hi": (lambda: _with(lambda p: (setattr(p.actor, "output", 1), setattr(p.actor, "lo", 1.0), setattr(p.actor, "hi", -1.0))), "lo <= hi"),
    "actor-clip-nan": (lambda: _with(lambda p: (setattr(p.actor, "output", 1), setattr(p.actor, "lo", float("nan")))), "lo <= hi"),
}


@pytest.mark.parametrize("case", sorted(CREATE_REFUSALS))
def test_create_refuses_bad_parameters_before_it_touches_a_device(case):
    from fleetrl_amd import _capi

    make, word = CREATE_REFUSALS[case]
    rc, why = _create(make())
    assert rc == _capi.ERR_INVALID and why.startswith("fleet_qtarget_create: ") and word in why, why


def test_create_refuses_null_pointers_and_weights_that_are_not_finite():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    assert _create(None) == (_capi.ERR_INVALID, "fleet_qtarget_create: null FleetQTargetParams")
    assert _create(_params(), weights=False) == (_capi.ERR_INVALID, "fleet_qtarget_create: null host_weights")
    w = np.zeros(1 << 12, np.float32)
    assert lib.fleet_qtarget_create(0, C.byref(_params()), w.ctypes.data, None) == _capi.ERR_INVALID
    # D = 5, actor 7-3: 35 + 7 + 21 + 3 = 66 floats; critic 0 over 8 inputs: 8-1 is 64 + 8 + 8 + 1; bias 2 of critic 0's first layer
    w[66 + 64 + 2] = np.inf
    h = C.c_void_p()
    assert lib.fleet_qtarget_create(0, C.byref(_params()), w.ctypes.data, C.byref(h)) == _capi.ERR_INVALID and not h
    assert lib.fleet_qtarget_last_error(None).decode() == "fleet_qtarget_create: critic 0, layer 0: bias 2 is not finite"
    # a null handle
    assert lib.fleet_qtarget_destroy(None) == _capi.OK
    for rc in (lib.fleet_qtarget_set_stream(None, None), lib.fleet_qtarget_load_host(None, w.ctypes.data), lib.fleet_qtarget_load_dev(None, None, 0),
               lib.fleet_qtarget_polyak_dev(None, None, 0, 0.5), lib.fleet_qtarget_export_dev(None, None, 0), lib.fleet_qtarget_describe(None, None)):
        assert rc == _capi.ERR_INVALID


def _target_args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetQTargetArgs()
    a.struct_bytes, a.noise_mode, a.gamma, a.noise_clip, a.act_lo, a.act_hi = C.sizeof(a), _capi.EXPLORE_NOISE_DRAW, 0.99, 0.5, -1.0, 1.0
    a.sigma = a.target_q = 256  # (never dereferenced: nothing is launched)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


TARGET_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=4), {}, "struct_bytes"),
    "noise_mode": (dict(noise_mode=2), {}, "unknown noise_mode 2"),
    "B-0": ({}, dict(B=0), "B must be >= 1, got 0"),
    "null-next_obs": ({}, dict(next_obs=None), "null next_obs"),
    "null-rewards": ({}, dict(rewards=None), "null rewards"),
    "null-dones": ({}, dict(dones=None), "null dones"),
    "null-sigma": (dict(sigma=None), {}, "null sigma"),
    "null-target_q": (dict(target_q=None), {}, "null target_q"),
    "nan-act_lo": (dict(act_lo=float("nan")), {}, "act_lo <= act_hi"),
    "nan-act_hi": (dict(act_hi=float("nan")), {}, "act_lo <= act_hi"),
    "lo>hi": (dict(act_lo=0.5, act_hi=0.25), {}, "act_lo <= act_hi"),
    "noise_clip<0": (dict(noise_clip=-0.125), {}, "noise_clip must be >= 0"),
    "noise_clip-nan": (dict(noise_clip=float("nan")), {}, "noise_clip must be >= 0"),
    "given-null-noise": (dict(noise_mode=1), {}, "GIVEN with a null noise"),
    "row_offset<0": (dict(row_offset=-1), {}, "row_offset must be >= 0, got -1"),
}


@pytest.mark.parametrize("case", sorted(TARGET_REFUSALS))
def test_target_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_qtarget_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, call, word = TARGET_REFUSALS[case]
    c = {"next_obs": 256, "rewards": 256, "dones": 256, "B": 4, **call}
    assert lib.fleet_qtarget_target_dev(None, c["next_obs"], c["rewards"], c["dones"], c["B"], C.byref(_target_args(**fields))) == _capi.ERR_INVALID
    why = lib.fleet_qtarget_last_error(None).decode()
    assert why.startswith("fleet_qtarget_target_dev: ") and word in why, why


def test_target_with_good_arguments_and_no_handle_names_the_handle():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    assert lib.fleet_qtarget_target_dev(None, 256, 256, 256, 4, C.byref(_target_args())) == _capi.ERR_INVALID
    assert lib.fleet_qtarget_last_error(None).decode() == "fleet_qtarget_target_dev: null handle"
    assert lib.fleet_qtarget_target_dev(None, 256, 256, 256, 4, None) == _capi.ERR_INVALID
    assert "null FleetQTargetArgs" in lib.fleet_qtarget_last_error(None).decode()
    # +inf is a noise_clip (no clip), and GIVEN with a noise pointer passes the checks
    ok = _target_args(noise_clip=float("inf"), noise_mode=_capi.EXPLORE_NOISE_GIVEN, noise=256)
    assert lib.fleet_qtarget_target_dev(None, 256, 256, 256, 4, C.byref(ok)) == _capi.ERR_INVALID
    assert lib.fleet_qtarget_last_error(None).decode() == "fleet_qtarget_target_dev: null handle"


# ---- the state-dict parser ---------------------------------------------------------------------------------------------------------
def _sb3_dict(n_critics, with_online=True):
    rng = np.random.default_rng(3)
    actor = pm.random_layers(rng, (6, 8, 2))
    qfs = [pm.random_layers(rng, (8, 9, 1)) for _ in range(n_critics)]
    sd = {}
    for prefix in (("actor", "actor_target") if with_online else ("actor_target",)):
        for i, (w, b) in enumerate(actor):
            sd[f"{prefix}.mu.{2 * i}.weight"], sd[f"{prefix}.mu.{2 * i}.bias"] = w, b
    for prefix in (("critic", "critic_target") if with_online else ("critic_target",)):
        for c, qf in enumerate(qfs):
            for i, (w, b) in enumerate(qf):
                sd[f"{prefix}.qf{c}.{2 * i}.weight"], sd[f"{prefix}.qf{c}.{2 * i}.bias"] = w, b
    return sd, actor, qfs


@pytest.mark.parametrize("n_critics,with_online", [(2, True), (1, True), (1, False)])
def test_parser_accepts_td3_ddpg_and_one_critic_dicts(n_critics, with_online):
    from fleetrl_amd.qtarget import parse_target_state_dict

    sd, actor, qfs = _sb3_dict(n_critics, with_online)
    got = parse_target_state_dict(sd)
    assert len(got["critics_layers"]) == n_critics and len(got["actor_layers"]) == 2
    for (w, b), (gw, gb) in zip(actor, got["actor_layers"]):
        assert gw is w and gb is b
    for qf, g in zip(qfs, got["critics_layers"]):
        assert all(gw is w and gb is b for (w, b), (gw, gb) in zip(qf, g))


@pytest.mark.parametrize("key", ["actor.latent_pi.0.weight", "log_std", "features_extractor.cnn.0.weight", "critic_target.qf2.0.weight",
                                 "actor_target.mu.weight", "mlp_extractor.policy_net.0.weight"])
def test_parser_refuses_strangers_by_key(key):
    from fleetrl_amd.qtarget import parse_target_state_dict

    sd, _, _ = _sb3_dict(2)
    sd[key] = np.zeros((2, 2), np.float32)
    with pytest.raises(ValueError, match=re.escape(repr(key))):
        parse_target_state_dict(sd)


def test_parser_needs_the_target_actor_and_the_first_critic():
    from fleetrl_amd.qtarget import parse_target_state_dict

    sd, _, _ = _sb3_dict(2)
    with pytest.raises(ValueError, match="actor_target.mu"):
        parse_target_state_dict({k: v for k, v in sd.items() if not k.startswith("actor_target.")})
    with pytest.raises(ValueError, match="critic_target.qf0"):
        parse_target_state_dict({k: v for k, v in sd.items() if not k.startswith("critic_target.qf0")})
    with pytest.raises(ValueError, match="bias"):
        parse_target_state_dict({k: v for k, v in sd.items() if k != "critic_target.qf1.0.bias"})


# ---- the model: known answers ------------------------------------------------------------------------------------------------------
def _one(w, b=0.0):
    return [(np.array(w, np.float32), np.array(np.broadcast_to(b, (len(w),)), np.float32))]


def _known(variant=None, **kw):
    """D = 1, A = 1.  The actor: d = clip(x) to +-1.  Critic 0: q = 1 * x + 3 * a'; critic 1: q = 2 * x + 1 * a'."""
    args = dict(next_obs=[[0.25]], rewards=[1.0], dones=[0.0], eps=[[1.0]], sigma=0.5, gamma=0.5, noise_clip=0.25, low=-1.0, high=1.0)
    args.update(kw)
    return qm.target_bits(_one([[1.0]]), [_one([[1.0, 3.0]]), _one([[2.0, 1.0]])], variant=variant, **args)


def test_known_answer_of_the_stated_arithmetic():
    # d = 0.25; n = clip(0.5, +-0.25) = 0.25; a' = 0.5; q0 = 0.25 + 1.5 = 1.75; q1 = 0.5 + 0.5 = 1; y = 1 + 0.5 * 1 = 1.5
    m = _known()
    assert m["next_actions"].tolist() == [[0.5]] and m["q"].tolist() == [[1.75, 1.0]] and m["y"].tolist() == [1.5]
    assert all(v.dtype == np.float32 for v in m.values())
    assert _known(dones=[1.0])["y"].tolist() == [1.0]  # a terminal row keeps its reward
    one = qm.target_bits(_one([[1.0]]), [_one([[1.0, 3.0]])], [[0.25]], [1.0], [0.0], [[1.0]], 0.5, gamma=0.5, noise_clip=0.25)
    assert one["q"].tolist() == [[1.75]] and one["y"].tolist() == [1.875]  # one critic: no min


def test_known_answers_tell_min_from_max():
    assert _known("max")["y"].tolist() == [1.875] != _known()["y"].tolist()
    # ... with critic 0 the smaller one as well: x = -1 gives q0 = -1 - 2.25, q1 = -2 - 0.75
    lo, hi = _known(next_obs=[[-1.0]]), _known("max", next_obs=[[-1.0]])
    assert lo["q"].tolist() == [[-3.25, -2.75]] and lo["y"].tolist() == [1 - 0.5 * 3.25] and hi["y"].tolist() == [1 - 0.5 * 2.75]


def test_known_answers_tell_two_roundings_from_a_fused_multiply_add():
    # t = 1 + 2^-12 (gamma, done = 0), qmin = 1 + 2^-12: t * qmin = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11; r = -1
    g = 1.0 + 2.0 ** -12
    kw = dict(next_obs=[[g]], rewards=[-1.0], gamma=g, eps=[[0.0]], low=0.0, high=0.0)
    # a' = 0: q0 = x = g, q1 = 2 g: the min is q0
    two, fused = _known(**kw), _known("fma", **kw)
    assert two["q"][0, 0] == f32(g) and two["y"].tolist() == [2.0 ** -11] and fused["y"].tolist() == [2.0 ** -11 + 2.0 ** -24]


def test_known_answers_tell_where_the_noise_clip_sits():
    # d = 0.25, n = 0.5: clip(n) then the sum gives 0.5; the clip of the sum gives 0.25
    assert _known()["next_actions"].tolist() == [[0.5]] and _known("clip_after_sum")["next_actions"].tolist() == [[0.25]]
    # the action bounds come last: d = 1, n = 0.25 -> 1.25 -> 1
    assert _known(next_obs=[[3.0]])["next_actions"].tolist() == [[1.0]]
    assert _known(next_obs=[[3.0]], low=-0.5, high=0.75)["next_actions"].tolist() == [[0.75]]


def test_known_answers_tell_obs_then_action_from_action_then_obs():
    # x = 0.25, a' = 0.5: q0 = 1 * x + 3 * a' = 1.75 against 1 * a' + 3 * x = 1.25
    assert _known()["q"][0].tolist() == [1.75, 1.0] and _known("action_first")["q"][0].tolist() == [1.25, 1.25]


# ---- the model: Polyak ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.0, 0.005, 0.37, 1.0])
def test_polyak_model_equals_exact_rational_arithmetic(tau):
    rng = np.random.default_rng(int(tau * 1000) + 1)
    t = (rng.standard_normal(400) * np.exp(rng.uniform(-6, 3, 400))).astype(np.float32)
    p = (rng.standard_normal(400) * np.exp(rng.uniform(-6, 3, 400))).astype(np.float32)
    got = qm.polyak_bits(t, p, tau)
    want = np.array([qm.polyak_exact(a, b, tau) for a, b in zip(t, p)], np.float32)
    assert got.dtype == np.float32 and pb.same_bits(got, want)
    if tau == 0.0:
        assert pb.same_bits(got, t)
    if tau == 1.0:
        assert pb.same_bits(got, p)


def test_polyak_constants_and_the_rounding_helper():
    tau32, omt32 = qm.polyak_constants(0.005)
    assert tau32 == f32(0.005) and omt32 == f32(0.995) and float(omt32) != 1.0 - float(tau32)  # (float)(1.0 - tau), not 1.0f - tau32
    assert qm.round_fraction32(Fraction(1) + Fraction(1, 2 ** 24)) == f32(1.0)  # a tie goes to the even neighbour
    assert qm.round_fraction32(Fraction(1) + Fraction(3, 2 ** 24)) == f32(1.0 + 2.0 ** -22)
    assert qm.round_fraction32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)) == f32(1.0 + 2.0 ** -23)  # float64 would tie
    # the fusion shows: tau * p + m with one rounding differs from two on some element
    rng = np.random.default_rng(5)
    t, p = rng.standard_normal(2000).astype(np.float32), rng.standard_normal(2000).astype(np.float32)
    two = ((t * omt32).astype(np.float32) + (tau32 * p).astype(np.float32)).astype(np.float32)
    assert not pb.same_bits(qm.polyak_bits(t, p, 0.005), two)


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------
def test_the_case_table_covers_what_it_must():
    pairs = {(c[0], c[1]) for c in qm.CASES.values()}
    assert pairs == {(5, 3), (126, 1), (127, 2), (128, 5), (129, 65), (250, 6), (388, 50), (7680, 512)}
    assert {c[2] for c in qm.CASES.values()} == set(qm.TRUNKS) and {c[3] for c in qm.CASES.values()} == {1, 2}
    assert qm.BATCHES == (1, 16, 17) and qm.ROWS == 17
    assert qm.TRUNKS["deep-critic"] == ((), (33, 130, 70, 1)) and qm.TRUNKS["deep-actor"] == ((33, 130, 70), (1,))
    named = [n for _, _, n in qm.COMPOSE] + list(qm.POLYAK_CASES) + [qm.INVARIANCE_CASE, qm.REFUSAL_CASE, qm.HOSTILE_CASE, qm.DESCRIBE_CASE]
    assert all(n in qm.CASES for n in named), [n for n in named if n not in qm.CASES]
    assert {a for a, _, _ in qm.COMPOSE} == {"relu", "tanh"} and ("tanh", "tanh", "388x50-c400-300-1-2") in qm.COMPOSE
    assert sum(len(net) for net in [qm.network(qm.REFUSAL_CASE)[0]] + qm.network(qm.REFUSAL_CASE)[1]) == 3  # 6 tensors
    for name in qm.POLYAK_CASES:  # ragged layers: the padding is there to stay zero
        actor, critics = qm.network(name)
        assert any(w.shape[1] % 4 and w.shape[0] % 64 for net in [actor] + critics for w, _ in net), name
    for name, (D, A, trunk, nc) in qm.CASES.items():
        actor, critics = qm.network(name)
        assert actor[0][0].shape[1] == D and actor[-1][0].shape[0] == A and len(critics) == nc
        assert all(c[0][0].shape[1] == D + A and c[-1][0].shape[0] == 1 for c in critics)


@pytest.mark.parametrize("name", sorted(qm.CASES))
def test_every_case_exercises_both_critics_both_clips_and_both_dones(name):
    """(The two 7680-wide cases take a few seconds each: their model walks 8192 input columns twice.)"""
    assert all(qm.facts(name).values()), qm.facts(name)
