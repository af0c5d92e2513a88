"""TD3 / DDPG's whole update without a GPU: the C ABI's section, its position, bindings and struct layouts against a compiled probe,
every refusal that needs no handle, the delay schedule against SB3's rule, and the NumPy restatement of the closing launch
(tests/offpolicy_model.py) against math.fsum."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import offpolicy_model as om

ROOT = om.ROOT
F32 = np.float32
ENTRIES = ("fleet_offpolicy_create", "fleet_offpolicy_destroy", "fleet_offpolicy_last_error", "fleet_offpolicy_describe",
           "fleet_offpolicy_td3_dev", "fleet_offpolicy_polyak_dev")
PARAM_FIELDS = ["struct_bytes", "max_steps"]
ARG_FIELDS = ["struct_bytes", "gradient_steps", "batch_size", "policy_delay", "reserved", "gamma", "tau", "noise_clip", "act_lo", "act_hi",
              "sigma", "lr", "beta1", "beta2", "eps", "max_grad_norm", "seed", "first_update", "norm", "stats"]
INFO_FIELDS = ["obs_dim", "act_dim", "n_critics", "max_batch", "max_steps", "n_actor_tensors", "n_critic_tensors", "reserved",
               "staging_bytes", "staging", "slots"]
TITLE = "TD3 / DDPG's whole update on the device"
TARGETS_TITLE = "TD3 / DDPG learning targets on the device"
PPO_TRAIN_TITLE = "PPO's whole update on the device"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_lies_between_the_targets_and_ppos_update_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_offpolicy_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.OFFPOLICY_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    assert hdr.count("---- " + TITLE) == 1
    titles = re.findall(r"^/\* ---- (.*?) \(", hdr, flags=re.M)
    assert titles.count(TITLE) == 1 and not any(t in TITLE for t in titles if t != TITLE)  # no other title inside this one
    at = titles.index(TITLE)
    assert titles[at - 1] == TARGETS_TITLE and titles[at + 1] == PPO_TRAIN_TITLE
    assert hdr.index("int fleet_qtarget_describe(") < hdr.index("---- " + TITLE) < hdr.index("---- " + PPO_TRAIN_TITLE)
    section = hdr[hdr.index("---- " + TITLE):hdr.index("---- " + PPO_TRAIN_TITLE)]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    for said in ("} FleetOffpolicyParams;", "} FleetOffpolicyArgs;", "} FleetOffpolicyInfo;", "#define FLEET_OFFPOLICY_MAX_STEPS 65536",
                 "#define FLEET_OFFPOLICY_SLOT_FLOATS 16", "t' = fmaf(tau32, p, t * omt32)", "(u + 1) % policy_delay == 0", "must outlive",
                 "FIVE launches", "NINE", "walks the zero", "the divergence is the caller's", "NaN when n == 0", "ONE stream",
                 "g_0 = (policy_delay - (first_update % policy_delay + 1) % policy_delay) % policy_delay", "first_update + G"):
        assert said in section, said
    assert not re.search(r"^(?:int|const char\*)\s+fleet_(?!offpolicy_)", section, flags=re.M)  # no entry of a neighbour in it
    assert len(re.findall(r"^/\* ---- ", section, flags=re.M)) == 0
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_offpolicy_create.argtypes) == 7 and len(lib.fleet_offpolicy_td3_dev.argtypes) == 8
    assert len(lib.fleet_offpolicy_polyak_dev.argtypes) == 2 and len(lib.fleet_offpolicy_describe.argtypes) == 2


def test_the_family_is_built_exported_and_restated_with_the_headers_constants():
    import fleetrl_amd
    from fleetrl_amd import _capi, build, offpolicy

    assert "fleet_offpolicy.hip" in build.SOURCES and "fleet_offpolicy.h" in build.HEADERS
    assert fleetrl_amd.DeviceTD3Train is offpolicy.DeviceTD3Train and offpolicy.DeviceTD3Train._prefix == "offpolicy"
    assert offpolicy.STATS == om.STATS and len(offpolicy.SB3_NAMES) == len(offpolicy.STATS)
    assert (_capi.OFFPOLICY_MAX_STEPS, _capi.OFFPOLICY_SLOT_FLOATS, _capi.TRAIN_STATS) == (om.MAX_STEPS, om.SLOT, om.STATS_LEN) == (65536, 16, 16)
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_offpolicy.h")).read()
    for name, want in (("kOffpolicyThreads", om.LANES), ("kOffpolicyMaxBlocks", om.MAX_BLOCKS), ("kOffpolicySlot", om.SLOT),
                       ("kOffpolicyActorAt", om.ACTOR_AT), ("kOffpolicyMaxSteps", om.MAX_STEPS)):
        assert re.search(rf"constexpr int {name} = (\d+);", src).group(1) == str(want), name


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetOffpolicyParams", _capi.FleetOffpolicyParams, PARAM_FIELDS),
                               ("FleetOffpolicyArgs", _capi.FleetOffpolicyArgs, ARG_FIELDS),
                               ("FleetOffpolicyInfo", _capi.FleetOffpolicyInfo, INFO_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["FLEET_OFFPOLICY_MAX_STEPS", "FLEET_OFFPOLICY_SLOT_FLOATS", "FLEET_TRAIN_STATS"]
    want += [_capi.OFFPOLICY_MAX_STEPS, _capi.OFFPOLICY_SLOT_FLOATS, _capi.TRAIN_STATS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert (C.sizeof(_capi.FleetOffpolicyParams), C.sizeof(_capi.FleetOffpolicyArgs), C.sizeof(_capi.FleetOffpolicyInfo)) == (8, 160, 56)


# ---- refusals that need no handle ------------------------------------------------------------------------------------------------
def _args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetOffpolicyArgs()
    a.struct_bytes, a.gradient_steps, a.batch_size, a.policy_delay = C.sizeof(a), 4, 64, 2
    a.gamma, a.tau, a.noise_clip, a.act_lo, a.act_hi, a.lr = 0.99, 0.005, 0.5, -1.0, 1.0, 1e-3
    for o in range(2):
        a.beta1[o], a.beta2[o], a.eps[o], a.max_grad_norm[o] = 0.9, 0.999, 1e-8, 0.0
    a.seed, a.first_update, a.sigma, a.stats = 1, 0, 2048, 4096
    for k, v in kw.items():
        if isinstance(v, tuple):  # (index, value) of a per-optimiser field
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def _ptrs(n=6, null_at=None, base=256):
    """(never dereferenced: nothing is launched)"""
    return (C.c_void_p * n)(*[None if i == null_at else base + 64 * i for i in range(n)])


NAN, INF = float("nan"), float("inf")
REFUSALS = {
    "struct_bytes": (dict(struct_bytes=152), "FleetOffpolicyArgs.struct_bytes does not match this library"),
    "gradient_steps-zero": (dict(gradient_steps=0), "gradient_steps must be >= 1, got 0"),
    "gradient_steps-negative": (dict(gradient_steps=-2), "gradient_steps must be >= 1, got -2"),
    "batch_size-zero": (dict(batch_size=0), "batch_size must be >= 1, got 0"),
    "policy_delay-zero": (dict(policy_delay=0), "policy_delay must be >= 1, got 0"),
    "policy_delay-negative": (dict(policy_delay=-1), "policy_delay must be >= 1, got -1"),
    "reserved": (dict(reserved=1), "reserved must be 0"),
    "stats-null": (dict(stats=None), "null stats"),
    # fleet_qtarget_target_dev's and fleet_qtarget_polyak_dev's, in their words
    "sigma-null": (dict(sigma=None), "null sigma"),
    "bounds-crossed": (dict(act_lo=1.0, act_hi=-1.0), "the bounds need act_lo <= act_hi"),
    "bounds-nan": (dict(act_hi=NAN), "the bounds need act_lo <= act_hi"),
    "noise_clip-negative": (dict(noise_clip=-0.5), "noise_clip must be >= 0"),
    "noise_clip-nan": (dict(noise_clip=NAN), "noise_clip must be >= 0"),
    "tau-above": (dict(tau=1.5), "tau must be in [0, 1], got 1.5"),
    "tau-negative": (dict(tau=-1e-9), "tau must be in [0, 1], got"),
    "tau-nan": (dict(tau=NAN), "tau must be in [0, 1], got"),
    # fleet_adam_step_dev's, in its words
    "lr-negative": (dict(lr=-1e-3), "lr must be finite and >= 0"),
    "lr-nan": (dict(lr=NAN), "lr must be finite and >= 0"),
    "lr-inf": (dict(lr=INF), "lr must be finite and >= 0"),
    "eps-actor-negative": (dict(eps=(0, -1e-8)), "eps must be finite and >= 0 (the actor optimiser's)"),
    "eps-critic-nan": (dict(eps=(1, NAN)), "eps must be finite and >= 0 (the critic optimiser's)"),
    "beta1-actor-one": (dict(beta1=(0, 1.0)), "beta1 must be in [0, 1) (the actor optimiser's)"),
    "beta1-critic-nan": (dict(beta1=(1, NAN)), "beta1 must be in [0, 1) (the critic optimiser's)"),
    "beta2-actor-negative": (dict(beta2=(0, -1e-9)), "beta2 must be in [0, 1) (the actor optimiser's)"),
    "beta2-critic-one": (dict(beta2=(1, 1.0)), "beta2 must be in [0, 1) (the critic optimiser's)"),
    "max_grad_norm-actor-nan": (dict(max_grad_norm=(0, NAN)), "max_grad_norm is NaN (the actor optimiser's)"),
    "max_grad_norm-critic-nan": (dict(max_grad_norm=(1, NAN)), "max_grad_norm is NaN (the critic optimiser's)"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_update_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_offpolicy_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = REFUSALS[case]
    rc = lib.fleet_offpolicy_td3_dev(None, C.byref(_args(**fields)), _ptrs(), _ptrs(base=8192), 6, _ptrs(12, base=16384), _ptrs(12, base=32768), 12)
    why = lib.fleet_offpolicy_last_error(None).decode()
    assert rc == _capi.ERR_INVALID and why.startswith("fleet_offpolicy_td3_dev: ") and word in why, why


def test_the_update_refuses_null_structs_arrays_and_aliases_and_names_the_null_handle():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fn = lib.fleet_offpolicy_td3_dev
    last = lambda: lib.fleet_offpolicy_last_error(None).decode()  # noqa: E731
    P, G, Q, H = _ptrs(), _ptrs(base=8192), _ptrs(12, base=16384), _ptrs(12, base=32768)
    a = C.byref(_args())
    assert fn(None, None, P, G, 6, Q, H, 12) == _capi.ERR_INVALID and last() == "fleet_offpolicy_td3_dev: null FleetOffpolicyArgs"
    assert fn(None, a, None, G, 6, Q, H, 12) == _capi.ERR_INVALID and "actor: null params" in last()
    assert fn(None, a, P, None, 6, Q, H, 12) == _capi.ERR_INVALID and "actor: null grads" in last()
    assert fn(None, a, P, G, 6, None, H, 12) == _capi.ERR_INVALID and "critics: null params" in last()
    assert fn(None, a, P, G, 6, Q, None, 12) == _capi.ERR_INVALID and "critics: null grads" in last()
    assert fn(None, a, P, G, 0, Q, H, 12) == _capi.ERR_INVALID and "actor: count must be in 1..24, got 0" in last()
    assert fn(None, a, P, G, 6, _ptrs(25), _ptrs(25, base=8192), 25) == _capi.ERR_INVALID and "critics: count must be in 1..24, got 25" in last()
    assert fn(None, a, _ptrs(null_at=2), G, 6, Q, H, 12) == _capi.ERR_INVALID and "actor: parameter tensor 2 is null" in last()
    assert fn(None, a, P, G, 6, Q, _ptrs(12, null_at=7, base=32768), 12) == _capi.ERR_INVALID and "critics: gradient tensor 7 is null" in last()
    alias = _ptrs(base=8192)
    alias[1] = P[1]
    assert fn(None, a, P, alias, 6, Q, H, 12) == _capi.ERR_INVALID and "actor: parameter tensor 1 is its own gradient" in last()
    for ok in (_args(), _args(tau=0.0), _args(tau=1.0), _args(noise_clip=INF), _args(lr=0.0), _args(norm=None), _args(policy_delay=2 ** 31 - 1),
               _args(gradient_steps=2 ** 31 - 1, batch_size=2 ** 31 - 1, seed=2 ** 64 - 1, first_update=2 ** 63, max_grad_norm=(1, 0.5))):
        assert fn(None, C.byref(ok), P, G, 6, Q, H, 12) == _capi.ERR_INVALID and last() == "fleet_offpolicy_td3_dev: null handle"


def test_create_describe_and_polyak_refuse_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_offpolicy_last_error(None).decode()  # noqa: E731
    h = C.c_void_p()
    fake = C.c_void_p(4096)  # (never dereferenced: the null handle in front of it is met first)
    good = _capi.FleetOffpolicyParams(C.sizeof(_capi.FleetOffpolicyParams), 1024)
    create = lib.fleet_offpolicy_create
    for k, word in enumerate(("null replay handle", "null target networks handle", "null gradient handle", "null actor optimiser handle",
                              "null critic optimiser handle")):
        handles = [fake] * k + [None] + [fake] * (4 - k)
        assert create(*handles, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h
        assert last() == "fleet_offpolicy_create: " + word
    assert create(None, None, None, None, None, C.byref(good), None) == _capi.ERR_INVALID and last() == "fleet_offpolicy_create: null output handle"
    assert create(None, None, None, None, None, None, C.byref(h)) == _capi.ERR_INVALID and last() == "fleet_offpolicy_create: null FleetOffpolicyParams"
    for p, word in ((_capi.FleetOffpolicyParams(4, 8), "FleetOffpolicyParams.struct_bytes does not match this library"),
                    (_capi.FleetOffpolicyParams(8, 0), "max_steps must be in 1..65536, got 0"),
                    (_capi.FleetOffpolicyParams(8, -1), "max_steps must be in 1..65536, got -1"),
                    (_capi.FleetOffpolicyParams(8, 65537), "max_steps must be in 1..65536, got 65537")):
        assert create(fake, fake, fake, fake, fake, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
        assert last() == "fleet_offpolicy_create: " + word
    assert lib.fleet_offpolicy_destroy(None) == _capi.OK
    assert lib.fleet_offpolicy_describe(None, None) == _capi.ERR_INVALID
    for tau, word in ((1.5, "tau must be in [0, 1], got 1.5"), (-0.25, "tau must be in [0, 1], got -0.25"), (NAN, "tau must be in [0, 1], got"),
                      (0.0, "null handle"), (1.0, "null handle"), (0.005, "null handle")):
        assert lib.fleet_offpolicy_polyak_dev(None, tau) == _capi.ERR_INVALID
        assert last().startswith("fleet_offpolicy_polyak_dev: ") and word in last(), last()


# ---- the delay schedule ------------------------------------------------------------------------------------------------------------
def sb3_actor_steps(n_updates: int, gradient_steps: int, policy_delay: int) -> list:
    """SB3's TD3.train, restated from its semantics: `for _ in range(gradient_steps): self._n_updates += 1; ...critic update...;
    if self._n_updates % self.policy_delay == 0: ...actor update and polyak...` -- the loop variable's values at which the branch runs."""
    hits = []
    for g in range(gradient_steps):
        n_updates += 1
        if n_updates % policy_delay == 0:
            hits.append(g)
    return hits


def test_the_delay_schedule_is_sb3s():
    for first in range(7):
        for G in range(1, 8):
            for delay in range(1, 4):
                assert om.actor_steps(first, G, delay) == sb3_actor_steps(first, G, delay), (first, G, delay)
    assert om.actor_steps(0, 2, 3) == [] and om.actor_steps(0, 5, 2) == [1, 3] and om.actor_steps(1, 5, 2) == [0, 2, 4]
    assert om.actor_steps(2 ** 40 + 1, 6, 4) == sb3_actor_steps(2 ** 40 + 1, 6, 4) == [2]


# ---- the closing launch's model ------------------------------------------------------------------------------------------------------
def _slots(G, rng, delay, first):
    s = np.zeros((G, om.SLOT), F32)
    s[:, 1], s[:, 2] = rng.random(G).astype(F32) * 3, rng.random(G).astype(F32) * 5
    s[:, 0] = s[:, 1] + s[:, 2]
    hits = om.actor_steps(first, G, delay)
    s[hits, om.ACTOR_AT] = -rng.standard_normal(len(hits)).astype(F32) * 10
    return s, hits


@pytest.mark.parametrize("G", [1, 2, 255, 256, 257, 1024])
def test_the_finish_model_stays_within_the_bound_of_fsum(G):
    """|model - fsum| <= 8 max(eps_ref, 2^-53 sum|x|) per mean: eps_ref = |NumPy's float64 pairwise mean - fsum's|, and 2^-53 sum|x| is
    one rounding of a sum of that size; every mean is divided by its count after the sum, as the reference is."""
    for delay, first in ((1, 0), (2, 0), (2, 1), (3, 5)):
        s, hits = _slots(G, np.random.default_rng(1000 * G + 10 * delay + first), delay, first)
        got = om.finish(s, first, delay)
        cols = [(0, s[:, 0]), (1, s[:, 1]), (2, s[:, 2])] + ([(3, s[hits, om.ACTOR_AT])] if hits else [])
        for k, x in cols:
            x64 = x.astype(np.float64)
            ref = math.fsum(x64.tolist()) / x64.size
            eps_ref = abs(float(x64.sum()) / x64.size - ref)
            bound = 8 * max(eps_ref, 2.0 ** -53 * float(np.abs(x64).sum()) / x64.size)
            print(f"G={G} delay={delay} first={first} [{k}]: model {abs(got[k] - ref):.3g} eps_ref {eps_ref:.3g} bound {bound:.3g}")
            assert abs(got[k] - ref) <= bound
        assert got[4] == np.float64(s[G - 1, 0]) and got[6] == first + G and got[7] == len(hits) and not got[8:].any()
        if hits:
            assert got[5] == np.float64(s[hits[-1], om.ACTOR_AT])
        else:
            assert np.isnan(got[3]) and np.isnan(got[5])


@pytest.mark.parametrize("G", [1, 2, 255, 256, 257, 1024])
def test_the_finish_model_is_exact_on_constant_slots(G):
    s = np.zeros((G, om.SLOT), F32)
    s[:, 0], s[:, 1], s[:, 2], s[:, om.ACTOR_AT] = F32(1.5), F32(0.5), F32(1.0), F32(-2.25)  # (G * 2.25 is exact far beyond G = 1024)
    got = om.finish(s, 0, 1)
    assert got[:8].tolist() == [1.5, 0.5, 1.0, -2.25, 1.5, -2.25, float(G), float(G)]


def test_the_finish_model_reports_nan_without_an_actor_step_and_ignores_stale_actor_halves():
    s = np.zeros((2, om.SLOT), F32)
    s[:, 0], s[:, om.ACTOR_AT] = F32(2.0), F32(99.0)  # what an earlier call left in the actor halves
    got = om.finish(s, 0, 3)
    assert np.isnan(got[3]) and np.isnan(got[5]) and got[7] == 0 and got[0] == 2.0 and got[6] == 2.0
    got = om.finish(np.concatenate([s, s]), 0, 3)  # G = 4: the one actor step is g = 2
    assert got[3] == 99.0 and got[5] == 99.0 and got[7] == 1
