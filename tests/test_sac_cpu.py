"""SAC's actor and soft targets without a GPU: the C ABI's section, its bindings and struct layouts against a compiled probe, every
refusal that needs no device, the SB3 state-dict parser, and the restatement of tests/sac_model.py against plain float64 torch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sac_model as sm

ROOT = sm.ROOT
ENTRIES = ("fleet_sac_create", "fleet_sac_last_error", "fleet_sac_act_dev", "fleet_sac_target_dev")
PARAM_FIELDS = ["struct_bytes", "obs_dim", "n_critics", "reserved", "actor", "critic"]
ACT_FIELDS = ["struct_bytes", "noise_mode", "deterministic", "env_id_offset", "seed", "step", "noise", "actions", "gaussian_actions",
              "log_prob", "mean", "log_std"]
TARGET_FIELDS = ["struct_bytes", "noise_mode", "seed", "step", "row_offset", "gamma", "ent_coef", "noise", "target_q", "next_actions",
                 "next_log_prob", "q"]
TITLE = "SAC on the device: squashed-Gaussian actor and soft Q targets"
OTHER_FAMILIES = ("NORM", "STATE", "ROLLOUT", "REPLAY", "POLICY", "EXPLORE", "NOISE", "QTARGET", "PPO", "TD3", "ADAM", "TRAIN", "VCLIP", "KL",
                  "OFFPOLICY", "COLLECT", "EVAL")


def _header():
    return open(os.path.join(ROOT, "include", "fleet_hip.h")).read()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_in_their_own_section_bound_and_exported():
    import fleetrl_amd
    from fleetrl_amd import _capi, build, sac

    hdr = _header()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = re.findall(r"^(?:int|const char\*)\s+(fleet_sac_\w+)\s*\(", hdr, flags=re.M)
    assert tuple(declared) == ENTRIES == _capi.SAC_SYMBOLS and set(declared) <= set(_capi.EXPORTED_SYMBOLS)
    assert hdr.count(TITLE) == 1
    section = hdr[hdr.index(TITLE):]
    assert hdr.index("int fleet_ppo_grad_gated_dev(") < hdr.index(TITLE)  # behind the last entry of the last "----" section
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    assert not re.search(r"^(?:extern |FLEET_API )?(?:int|const char\*)\s+fleet_(?!sac_)", section, flags=re.M)  # no entry of a neighbour in it
    assert all(hdr.index(f" {name}(") > hdr.index(TITLE) for name in ENTRIES)
    for said in ("} FleetSacParams;", "} FleetSacActArgs;", "} FleetSacTargetArgs;",
                 "ls[j]       = l[j] < -20.0f ? -20.0f : (l[j] > 2.0f ? 2.0f : l[j])",
                 "sd[j]       = expf(ls[j]);   u[j] = fmaf(sd[j], eps[j], m[j]);   a[j] = tanhf(u[j])",
                 "t[j]        = fmaf(-0.5f * eps[j], eps[j], -ls[j]) - 0.9189385332f",
                 "c[j]        = logf((1.0f - a[j] * a[j]) + 1e-6f)", "log_prob    = S(t) - S(c)",
                 "p = alpha * lp;  v = qmin - p;  t = (1.0f - dones[b]) * gamma;  y[b] = rewards[b] + t * v",
                 "Deviation from SB3", "SEED OF ITS OWN", "handles that do not launch on one stream", "REFUSE", "Out of scope"):
        assert said in section, said
    assert "fleet_sac.hip" in build.SOURCES
    assert fleetrl_amd.DeviceSACNetworks is sac.DeviceSACNetworks
    lib = C.CDLL(build.build())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_sac_create.argtypes) == 4 and len(lib.fleet_sac_act_dev.argtypes) == 5 and len(lib.fleet_sac_target_dev.argtypes) == 7


def test_no_sac_symbol_carries_another_familys_prefix_and_no_list_intersects():
    from fleetrl_amd import _capi

    prefixes = [m for m in ("norm", "state", "rollout", "replay", "policy", "explore", "noise", "qtarget", "ppo", "td3", "adam", "train",
                            "offpolicy", "collect", "eval", "log", "lp", "direct", "rccl")]
    for name in _capi.SAC_SYMBOLS:
        assert name.startswith("fleet_sac_") and not any(name.startswith(f"fleet_{p}_") for p in prefixes), name
    for family in OTHER_FAMILIES:
        assert not set(getattr(_capi, family + "_SYMBOLS")) & set(_capi.SAC_SYMBOLS), family
    assert len(_capi.EXPORTED_SYMBOLS) == len(set(_capi.EXPORTED_SYMBOLS))


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetSacParams", _capi.FleetSacParams, PARAM_FIELDS), ("FleetSacActArgs", _capi.FleetSacActArgs, ACT_FIELDS),
                               ("FleetSacTargetArgs", _capi.FleetSacTargetArgs, TARGET_FIELDS)):
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
    assert (C.sizeof(_capi.FleetSacParams), C.sizeof(_capi.FleetSacActArgs), C.sizeof(_capi.FleetSacTargetArgs)) == (136, 80, 80)


# ---- refusals without a device ---------------------------------------------------------------------------------------------------
def _params(D=7, actor=(64, 10), critics=((64, 1), (64, 1)), **over):
    from fleetrl_amd import _capi

    p = _capi.FleetSacParams()
    p.struct_bytes, p.obs_dim, p.n_critics = C.sizeof(p), D, len(critics)
    for head, widths in [(p.actor, actor)] + [(p.critic[c], w) for c, w in enumerate(critics)]:
        head.n_layers = len(widths)
        for l, w in enumerate(widths):
            head.width[l] = w
        head.activation, head.output = _capi.POLICY_ACT_RELU, _capi.POLICY_OUT_NONE
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _create(p, weights=True, out=True):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    w = np.zeros(1 << 16, np.float32)
    h = C.c_void_p()
    rc = lib.fleet_sac_create(0, C.byref(p) if p is not None else None, w.ctypes.data if weights else None, C.byref(h) if out else None)
    return rc, lib.fleet_sac_last_error(None).decode()


def _tweak(fn):
    p = _params()
    fn(p)
    return p


CREATE_REFUSALS = {
    "struct_bytes": (lambda: _params(struct_bytes=8), "FleetSacParams.struct_bytes does not match"),
    "obs_dim": (lambda: _params(D=0), "obs_dim must be in 1..8192"),
    "n_critics": (lambda: _params(n_critics=3), "n_critics must be 1 or 2, got 3"),
    "odd last actor width": (lambda: _params(actor=(64, 11)), "actor: the last width must be even"),
    "2A > 512": (lambda: _params(actor=(64, 514)), "actor: width of layer 1 must be in 1..512, got 514"),
    "actor output": (lambda: _tweak(lambda p: setattr(p.actor, "output", 2)), "actor: the output transform must be NONE"),
    "critic last width": (lambda: _params(critics=((64, 1), (64, 2))), "critic 1: the last width must be 1, got 2"),
    "critic output": (lambda: _tweak(lambda p: setattr(p.critic[0], "output", 2)), "critic 0: the output transform must be NONE"),
    "D + A": (lambda: _params(D=8190, actor=(64, 6)), "obs_dim + act_dim must be at most 8192 (a critic's input), got 8190 + 3"),
    "layers": (lambda: _tweak(lambda p: setattr(p.actor, "n_layers", 5)), "actor: n_layers must be in 1..4, got 5"),
    "activation": (lambda: _tweak(lambda p: setattr(p.critic[1], "activation", 7)), "critic 1: unknown activation"),
}


@pytest.mark.parametrize("case", sorted(CREATE_REFUSALS))
def test_create_refuses_bad_parameters_before_the_device_is_touched(case):
    from fleetrl_amd import _capi

    make, reason = CREATE_REFUSALS[case]
    rc, msg = _create(make())
    assert rc == _capi.ERR_INVALID and msg.startswith("fleet_sac_create: ") and reason in msg, msg


def test_create_refuses_null_pointers():
    from fleetrl_amd import _capi

    for kwargs, reason in ((dict(p=None), "null FleetSacParams"), (dict(p=_params(), weights=False), "null host_weights"),
                           (dict(p=_params(), out=False), "null output handle")):
        rc, msg = _create(**kwargs)
        assert rc == _capi.ERR_INVALID and msg == "fleet_sac_create: " + reason, msg


def _act_args(**over):
    from fleetrl_amd import _capi

    a = _capi.FleetSacActArgs()
    a.struct_bytes, a.actions = C.sizeof(a), 4096
    for k, v in over.items():
        setattr(a, k, v)
    return a


ACT_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=12), {}, "FleetSacActArgs.struct_bytes does not match"),
    "noise_mode": (dict(noise_mode=2), {}, "unknown noise_mode 2"),
    "E": ({}, dict(E=0), "E must be >= 1, got 0"),
    "obs": ({}, dict(obs=None), "null obs"),
    "actions": (dict(actions=None), {}, "null actions"),
    "given": (dict(noise_mode=1), {}, "noise_mode GIVEN with a null noise"),
    "offset": (dict(env_id_offset=-1), {}, "env_id_offset must be >= 0, got -1"),
    "deterministic value": (dict(deterministic=2), {}, "deterministic must be 0 or 1, got 2"),
    "deterministic log_prob": (dict(deterministic=1, log_prob=4096), {}, "log_prob asked with deterministic"),
    "deterministic gaussian": (dict(deterministic=1, gaussian_actions=4096), {}, "gaussian_actions asked with deterministic"),
    "deterministic noise": (dict(deterministic=1, noise=4096), {}, "noise given with deterministic"),
    "null handle": ({}, {}, "null handle"),
}


@pytest.mark.parametrize("case", sorted(ACT_REFUSALS))
def test_act_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_sac_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    over, call, reason = ACT_REFUSALS[case]
    call = {"obs": 4096, "E": 4, **call}
    rc = lib.fleet_sac_act_dev(None, call["obs"], call["E"], None, C.byref(_act_args(**over)))
    msg = lib.fleet_sac_last_error(None).decode()
    assert rc == _capi.ERR_INVALID and msg.startswith("fleet_sac_act_dev: ") and reason in msg, msg
    assert lib.fleet_sac_act_dev(None, 4096, 4, None, None) == _capi.ERR_INVALID
    assert lib.fleet_sac_last_error(None).decode() == "fleet_sac_act_dev: null FleetSacActArgs"


def _target_args(**over):
    from fleetrl_amd import _capi

    a = _capi.FleetSacTargetArgs()
    a.struct_bytes, a.ent_coef, a.target_q, a.gamma = C.sizeof(a), 4096, 4096, 0.99
    for k, v in over.items():
        setattr(a, k, v)
    return a


TARGET_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=12), {}, "FleetSacTargetArgs.struct_bytes does not match"),
    "noise_mode": (dict(noise_mode=-1), {}, "unknown noise_mode -1"),
    "B": ({}, dict(B=0), "B must be >= 1, got 0"),
    "next_obs": ({}, dict(next_obs=None), "null next_obs"),
    "rewards": ({}, dict(rewards=None), "null rewards"),
    "dones": ({}, dict(dones=None), "null dones"),
    "ent_coef": (dict(ent_coef=None), {}, "null ent_coef"),
    "target_q": (dict(target_q=None), {}, "null target_q"),
    "given": (dict(noise_mode=1), {}, "noise_mode GIVEN with a null noise"),
    "offset": (dict(row_offset=-3), {}, "row_offset must be >= 0, got -3"),
    "null handle": ({}, {}, "null handle"),
}


@pytest.mark.parametrize("case", sorted(TARGET_REFUSALS))
def test_target_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    over, call, reason = TARGET_REFUSALS[case]
    call = {"next_obs": 4096, "rewards": 4096, "dones": 4096, "B": 4, **call}
    rc = lib.fleet_sac_target_dev(None, None, call["next_obs"], call["rewards"], call["dones"], call["B"], C.byref(_target_args(**over)))
    msg = lib.fleet_sac_last_error(None).decode()
    assert rc == _capi.ERR_INVALID and msg.startswith("fleet_sac_target_dev: ") and reason in msg, msg
    assert lib.fleet_sac_target_dev(None, None, 4096, 4096, 4096, 4, None) == _capi.ERR_INVALID
    assert lib.fleet_sac_last_error(None).decode() == "fleet_sac_target_dev: null FleetSacTargetArgs"


# ---- SB3's state dict ----------------------------------------------------------------------------------------------------------------
def test_from_state_dict_concatenates_mu_and_log_std_and_picks_the_critics():
    from fleetrl_amd import sac

    actor, critics, _ = sm.networks("tanh", 7, 5, n_critics=2)
    _, targets, _ = sm.networks("tanh", 7, 5, n_critics=2, salt=1)
    sd = sm.sac_state_dict(actor, critics, targets)
    for which, want in (("online", critics), ("target", targets)):
        got = sac.parse_sac_state_dict(sd, which)
        assert len(got["actor_layers"]) == 3 and len(got["critics_layers"]) == 2
        for (w, b), (w0, b0) in zip(got["actor_layers"], actor):
            assert np.array_equal(np.asarray(w), w0) and np.array_equal(np.asarray(b), b0)
        w, b = got["actor_layers"][-1]
        assert w.shape == (10, 64) and np.array_equal(w[:5], sd["actor.mu.weight"]) and np.array_equal(w[5:], sd["actor.log_std.weight"])
        assert np.array_equal(b[:5], sd["actor.mu.bias"]) and np.array_equal(b[5:], sd["actor.log_std.bias"])
        for net, net0 in zip(got["critics_layers"], want):
            for (w, b), (w0, b0) in zip(net, net0):
                assert np.array_equal(np.asarray(w), w0) and np.array_equal(np.asarray(b), b0)
    one = sac.parse_sac_state_dict({k: v for k, v in sd.items() if ".qf1." not in k})
    assert len(one["critics_layers"]) == 1


def test_from_state_dict_refuses_unknown_keys_by_name_and_a_wrong_which():
    from fleetrl_amd import sac

    actor, critics, _ = sm.networks("one", 7, 3, n_critics=1)
    sd = sm.sac_state_dict(actor, critics)
    assert len(sac.parse_sac_state_dict(sd)["actor_layers"]) == 1  # no latent_pi layer: the heads over the observation
    for key in ("actor.features_extractor.cnn.0.weight", "log_ent_coef", "actor_target.mu.0.weight", "critic.qf2.0.weight"):
        with pytest.raises(ValueError, match=re.escape(repr(key))):
            sac.parse_sac_state_dict({**sd, key: np.zeros(1, np.float32)})
    with pytest.raises(ValueError, match="which must be 'online' or 'target'"):
        sac.parse_sac_state_dict(sd, "both")
    with pytest.raises(ValueError, match="actor.log_std"):
        sac.parse_sac_state_dict({k: v for k, v in sd.items() if not k.startswith("actor.log_std")})
    with pytest.raises(ValueError, match="critic_target.qf0"):
        sac.parse_sac_state_dict({k: v for k, v in sd.items() if not k.startswith("critic_target")}, "target")


# ---- the model against SB3's expressions in float64 torch ------------------------------------------------------------------------
@pytest.mark.parametrize("A", (1, 5, 130))
def test_the_eps_form_of_the_log_probability_is_sb3s_quantity(A):
    """Normal(mean, std).log_prob(u).sum(1) - log(1 - tanh(u)^2 + 1e-6).sum(1) in float64 torch against the model's form with the
    Gaussian term written in eps.  Tolerance, float64 rounding only: (u - m) / sd restates eps to a few 2^-53 relative, so each of the
    A Gaussian terms moves by <= 8 * 2^-53 * (eps^2 + 1) and each sum of A terms of size <= 40 rounds within A * 2^-53 * 40.  The
    correction cancels: one ulp of tanh (NumPy's and torch's may differ by that) moves log(1 - a^2 + 1e-6) by 2^-53 * 2 |a| / (1 - a^2 +
    1e-6), up to 2e-10 at saturation; four such ulps are allowed."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(A)
    E = 64
    mean, raw, eps = rng.standard_normal((E, A)) * 2, rng.uniform(-25, 4, (E, A)), rng.standard_normal((E, A))
    got = sm.act64(mean, raw, eps)
    m, ls = torch.from_numpy(mean), torch.clamp(torch.from_numpy(raw), sm.LOG_STD_MIN, sm.LOG_STD_MAX)
    u = m + ls.exp() * torch.from_numpy(eps)
    want = torch.distributions.Normal(m, ls.exp()).log_prob(u).sum(1) - torch.log(1 - torch.tanh(u) ** 2 + 1e-6).sum(1)
    # where sd is tiny against m, u = m + sd * eps loses eps's low bits: (u - m) / sd restates eps only to 2^-53 |u| / sd
    lost = (2.0 ** -53 * np.abs(u.numpy()) / np.exp(ls.numpy()))
    a = np.abs(np.tanh(u.numpy()))
    cancel = 4 * 2.0 ** -53 * 2 * a / (1 - a * a + 1e-6)
    tol = (2.0 ** -53 * (8 * (eps ** 2 + 1) + 80) + 2 * np.abs(eps) * lost + lost ** 2 + cancel).sum(1) + 2.0 ** -52 * np.abs(want.numpy())
    assert np.array_equal(got["log_std"], ls.numpy()) and np.array_equal(got["gaussian_actions"], u.numpy())
    assert (np.abs(got["log_prob"] - want.numpy()) <= tol).all(), float(np.abs(got["log_prob"] - want.numpy()).max())
    assert (np.abs(sm.sb3_log_prob64(mean, ls.numpy(), u.numpy()) - want.numpy()) <= tol).all()


@pytest.mark.parametrize("nc", (1, 2))
def test_the_target_is_sb3s(nc):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(nc)
    B = 33
    r, d = rng.standard_normal(B), (rng.random(B) < 0.3).astype(np.float64)
    q, lp = rng.standard_normal((B, nc)) * 5, rng.standard_normal(B) * 10
    tq, tlp = torch.from_numpy(q), torch.from_numpy(lp).reshape(-1, 1)
    next_q, _ = torch.min(tq, dim=1, keepdim=True)
    next_q = next_q - 0.37 * tlp
    want = (torch.from_numpy(r).reshape(-1, 1) + (1 - torch.from_numpy(d).reshape(-1, 1)) * 0.99 * next_q).reshape(-1).numpy()
    got = sm.sb3_target64(r, d, 0.99, q, 0.37, lp)
    assert (np.abs(got - want) <= 2.0 ** -51 * (np.abs(want) + np.abs(r))).all()
    assert np.array_equal(got[d == 1], r[d == 1])


def test_the_float32_chain_stays_near_the_float64_one_and_the_sum_is_the_lane_order():
    """The float32 restatement from stored values against float64 on the same values; and S on inputs whose sum is exact in any
    order, and on one where the order shows."""
    rng = np.random.default_rng(5)
    E, A = 37, 130
    ls = sm.clamp_log_std32(rng.uniform(-25, 4, (E, A)).astype(np.float32))
    assert ls.min() == -20 and ls.max() == 2
    eps = rng.standard_normal((E, A)).astype(np.float32)
    a = np.tanh(rng.standard_normal((E, A)) * 3).astype(np.float32)
    a[0, :] = 1.0  # saturated
    t64, c64 = sm.log_prob_terms64(ls, eps, a)
    got = sm.log_prob32(ls, eps, a).astype(np.float64)
    assert (np.abs(got - (t64.sum(1) - c64.sum(1))) <= 1e-3).all()
    assert np.array_equal(sm.terms32(ls, eps, a)[1][0], np.full(A, np.log(np.float64(np.float32(1e-6))), np.float32))
    ints = rng.integers(-1000, 1000, (E, A)).astype(np.float32)
    assert np.array_equal(sm.lane_sum32(ints), ints.sum(1))
    x = np.zeros((1, 65), np.float32)
    x[0, 0], x[0, 1], x[0, 64] = 2.0 ** 24, 1.0, 1.0  # lane 0 adds columns 0 and 64 first: 2^24 + 1 rounds to 2^24, then + lane 1's 1
    assert sm.lane_sum32(x)[0] == np.float32(2.0 ** 24) and sm.sum_depth(65) == 8
    y = sm.target32([1.0], [0.0], 0.5, [[3.0, 2.0]], 0.25, [4.0])
    assert y.dtype == np.float32 and y[0] == np.float32(1.0 + 0.5 * (2.0 - 1.0))
