"""SAC's whole update without a GPU: the C ABI's section, its position, bindings and struct layouts against a compiled probe, every
refusal that needs no handle, the target-update schedule against SB3's loop, the NumPy restatement of the closing launch
(tests/sac_train_model.py) against math.fsum, the alpha launch's value, and two misreadings of SB3's loop against the bound."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sac_train_model as sm
from fleetrl_amd.sac_train import SAC_TRAIN_STATS  # the model's block is named by the package's own tuple

ROOT = sm.ROOT
F32, F64 = np.float32, np.float64
ENTRIES = ("fleet_sactrain_create", "fleet_sactrain_destroy", "fleet_sactrain_last_error", "fleet_sactrain_describe",
           "fleet_sactrain_alpha_dev", "fleet_sactrain_scale_dev", "fleet_sactrain_polyak_dev", "fleet_sactrain_sac_dev")
PARAM_FIELDS = ["struct_bytes", "max_steps"]
ARG_FIELDS = ["struct_bytes", "gradient_steps", "batch_size", "target_update_interval", "gamma", "target_entropy", "tau", "loss_scale", "lr",
              "beta1", "beta2", "eps", "max_grad_norm", "seed", "target_seed", "first_update", "ent_coef", "log_ent_coef", "log_ent_coef_grad",
              "norm", "stats"]
INFO_FIELDS = ["obs_dim", "act_dim", "n_critics", "max_batch", "max_steps", "n_actor_tensors", "n_critic_tensors", "learned_alpha",
               "scale_chunks", "reserved", "staging_bytes", "staging", "alpha", "slots"]
TITLE = "SAC's whole update on the device"
OTHER_LISTS = ("EXPORTED", "NORM", "STATE", "ROLLOUT", "REPLAY", "POLICY", "EXPLORE", "NOISE", "QTARGET", "PPO", "TD3", "ADAM", "TRAIN", "VCLIP",
               "KL", "OFFPOLICY", "SAC", "SAC_GRAD", "COLLECT", "EVAL")


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_section_is_the_headers_last_and_every_entry_is_bound_and_exported():
    import fleetrl_amd
    from fleetrl_amd import _capi, build, sac_train

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = re.findall(r"^FLEET_API extern (?:int|const char\*)\s+(fleet_\w+)\s*\(", hdr, flags=re.M)
    assert tuple(declared) == ENTRIES == _capi.SACTRAIN_SYMBOLS
    assert hdr.count("==== " + TITLE) == 1
    titles = re.findall(r"^/\* (?:----|====) (.*?) \(", hdr, flags=re.M)
    assert titles[-1] == TITLE and titles.count(TITLE) == 1  # the last section
    section = hdr[hdr.index("==== " + TITLE):]
    assert hdr.index("int fleet_sac_actor_grad_dev(") < hdr.index("==== " + TITLE)
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    assert all(hdr.index(f" {name}(") > hdr.index("==== " + TITLE) for name in ENTRIES)
    assert re.findall(r"^[A-Za-z_ ]*?(?:int|const char\*)\s+(fleet_\w+)\s*\(", section, flags=re.M) == list(ENTRIES)  # and nobody else's
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for said in ("} FleetSacTrainParams;", "} FleetSacTrainArgs;", "} FleetSacTrainInfo;", "#define FLEET_SACTRAIN_MAX_STEPS 65536",
                 "#define FLEET_SACTRAIN_SLOT_FLOATS 16", "alpha = (float)exp((double)log_ent_coef[0])", "must outlive",
                 "iff g % target_update_interval == 0", "the index INSIDE the call", "BEFORE the entropy coefficient's optimiser step",
                 "grad[i] = grad[i] * (float)loss_scale", "(G - 1) / target_update_interval + 1", "NaN with a fixed alpha", "ONE stream",
                 "(double)(float)loss_scale * S((double)c[g][0]) / (double)G", "bit-equal to the same entries called one by one"):
        assert said in flat, said
    assert "fleet_sactrain.hip" in build.SOURCES and "fleet_offpolicy.hip" in build.SOURCES and "fleet_offpolicy.h" in build.HEADERS
    for name in ("DeviceSACTrain", "SAC_TRAIN_STATS", "SAC_TRAIN_SB3_NAMES"):
        assert getattr(fleetrl_amd, name) is getattr(sac_train, name)
    assert sac_train.DeviceSACTrain._prefix == "sactrain" and sac_train.SAC_TRAIN_STATS == sm.SAC_TRAIN_STATS
    assert len(sac_train.SAC_TRAIN_SB3_NAMES) == len(sac_train.SAC_TRAIN_STATS)
    assert [n for n in sac_train.SAC_TRAIN_SB3_NAMES if n] == ["train/critic_loss", "train/actor_loss", "train/ent_coef", "train/ent_coef_loss",
                                                             "train/n_updates"]
    built = C.CDLL(build.build())
    lib = _capi.load_library()
    for name in ENTRIES:
        assert hasattr(built, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_sactrain_create.argtypes) == 8 and len(lib.fleet_sactrain_sac_dev.argtypes) == 8
    assert len(lib.fleet_sactrain_alpha_dev.argtypes) == 3 and len(lib.fleet_sactrain_scale_dev.argtypes) == 4
    graft = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_capi.SACTRAIN_SYMBOLS" in graft


def test_the_symbol_list_intersects_no_other_list_and_the_constants_are_the_headers():
    from fleetrl_amd import _capi

    for family in OTHER_LISTS:
        assert not set(getattr(_capi, family + "_SYMBOLS")) & set(_capi.SACTRAIN_SYMBOLS), family
    assert all(n.startswith("fleet_sactrain_") for n in _capi.SACTRAIN_SYMBOLS) and len(set(_capi.SACTRAIN_SYMBOLS)) == 8
    assert (_capi.SACTRAIN_MAX_STEPS, _capi.SACTRAIN_SLOT_FLOATS, _capi.SACTRAIN_SCALE_CHUNK) == (sm.MAX_STEPS, sm.SLOT, sm.SCALE_CHUNK)
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_offpolicy.h")).read()
    assert re.search(r"constexpr int kSacTrainChunk = (\d+);", src).group(1) == str(sm.SCALE_CHUNK)
    csrc = os.path.join(ROOT, "fleetrl_amd", "csrc")
    td3, hip = open(os.path.join(csrc, "fleet_offpolicy.hip")).read(), open(os.path.join(csrc, "fleet_sactrain.hip")).read()
    # one Polyak kernel and one launch site for the two families: the kernel is not copied, the SAC family goes through its launch
    assert td3.count("void offpolicy_polyak(") == 1 and td3.count("hipLaunchKernelGGL(offpolicy_polyak,") == 1
    assert "void offpolicy_polyak(" not in hip and "offpolicy_launch_polyak(h, h->tgt, h->img," in hip
    assert "int offpolicy_launch_polyak(" in src and "double tree_total(" in src and "double tree_total(" not in td3 + hip
    for kernel in ("sactrain_alpha", "sactrain_scale", "sactrain_finish"):
        assert f"void {kernel}(" in hip
    assert not re.search(r"atomic[A-Z_(]|__hip_atomic|__atomic|\basm\b", hip)  # launch boundaries are the only visibility mechanism


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetSacTrainParams", _capi.FleetSacTrainParams, PARAM_FIELDS),
                               ("FleetSacTrainArgs", _capi.FleetSacTrainArgs, ARG_FIELDS),
                               ("FleetSacTrainInfo", _capi.FleetSacTrainInfo, INFO_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["FLEET_SACTRAIN_MAX_STEPS", "FLEET_SACTRAIN_SLOT_FLOATS", "FLEET_SACTRAIN_SCALE_CHUNK", "FLEET_TRAIN_STATS"]
    want += [_capi.SACTRAIN_MAX_STEPS, _capi.SACTRAIN_SLOT_FLOATS, _capi.SACTRAIN_SCALE_CHUNK, _capi.TRAIN_STATS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert (C.sizeof(_capi.FleetSacTrainParams), C.sizeof(_capi.FleetSacTrainArgs), C.sizeof(_capi.FleetSacTrainInfo)) == (8, 208, 72)


# ---- refusals that need no handle ------------------------------------------------------------------------------------------------
def _args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetSacTrainArgs()
    a.struct_bytes, a.gradient_steps, a.batch_size, a.target_update_interval = C.sizeof(a), 4, 64, 1
    a.gamma, a.tau, a.lr, a.loss_scale, a.target_entropy = 0.99, 0.005, 1e-3, 0.5, -3.0
    for o in range(3):
        a.beta1[o], a.beta2[o], a.eps[o], a.max_grad_norm[o] = 0.9, 0.999, 1e-8, 0.0
    a.seed, a.target_seed, a.first_update, a.log_ent_coef, a.log_ent_coef_grad, a.stats = 1, 2, 0, 2048, 3072, 4096
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
BOTH = "give exactly one of ent_coef (a fixed alpha) and log_ent_coef (a learned one)"
TOGETHER = "log_ent_coef and log_ent_coef_grad must be given together or both be null"
REFUSALS = {
    "struct_bytes": (dict(struct_bytes=200), "FleetSacTrainArgs.struct_bytes does not match this library"),
    "gradient_steps-zero": (dict(gradient_steps=0), "gradient_steps must be >= 1, got 0"),
    "gradient_steps-negative": (dict(gradient_steps=-2), "gradient_steps must be >= 1, got -2"),
    "batch_size-zero": (dict(batch_size=0), "batch_size must be >= 1, got 0"),
    "interval-zero": (dict(target_update_interval=0), "target_update_interval must be >= 1, got 0"),
    "interval-negative": (dict(target_update_interval=-1), "target_update_interval must be >= 1, got -1"),
    "stats-null": (dict(stats=None), "null stats"),
    "both-alphas": (dict(ent_coef=1024), BOTH),
    "no-alpha": (dict(log_ent_coef=None, log_ent_coef_grad=None), BOTH),
    "log_ent_coef-without-its-grad": (dict(log_ent_coef_grad=None), TOGETHER),
    "grad-without-log_ent_coef": (dict(log_ent_coef=None, ent_coef=1024), TOGETHER),
    "log_ent_coef-is-its-own-grad": (dict(log_ent_coef_grad=2048), "parameter tensor 0 is its own gradient (the entropy coefficient optimiser's)"),
    "loss_scale-nan": (dict(loss_scale=NAN), "loss_scale must be finite"),
    "loss_scale-inf": (dict(loss_scale=INF), "loss_scale must be finite"),
    # the Polyak update's, in its words
    "tau-above": (dict(tau=1.5), "tau must be in [0, 1], got 1.5"),
    "tau-negative": (dict(tau=-1e-9), "tau must be in [0, 1], got"),
    "tau-nan": (dict(tau=NAN), "tau must be in [0, 1], got"),
    # fleet_adam_step_dev's, in its words
    "lr-negative": (dict(lr=-1e-3), "lr must be finite and >= 0"),
    "lr-nan": (dict(lr=NAN), "lr must be finite and >= 0"),
    "lr-inf": (dict(lr=INF), "lr must be finite and >= 0"),
    "eps-actor-negative": (dict(eps=(0, -1e-8)), "eps must be finite and >= 0 (the actor optimiser's)"),
    "eps-critic-nan": (dict(eps=(1, NAN)), "eps must be finite and >= 0 (the critic optimiser's)"),
    "eps-ent-inf": (dict(eps=(2, INF)), "eps must be finite and >= 0 (the entropy coefficient optimiser's)"),
    "beta1-actor-one": (dict(beta1=(0, 1.0)), "beta1 must be in [0, 1) (the actor optimiser's)"),
    "beta1-ent-nan": (dict(beta1=(2, NAN)), "beta1 must be in [0, 1) (the entropy coefficient optimiser's)"),
    "beta2-critic-one": (dict(beta2=(1, 1.0)), "beta2 must be in [0, 1) (the critic optimiser's)"),
    "beta2-ent-negative": (dict(beta2=(2, -1e-9)), "beta2 must be in [0, 1) (the entropy coefficient optimiser's)"),
    "max_grad_norm-actor-nan": (dict(max_grad_norm=(0, NAN)), "max_grad_norm is NaN (the actor optimiser's)"),
    "max_grad_norm-ent-nan": (dict(max_grad_norm=(2, NAN)), "max_grad_norm is NaN (the entropy coefficient optimiser's)"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_update_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_sactrain_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = REFUSALS[case]
    rc = lib.fleet_sactrain_sac_dev(None, C.byref(_args(**fields)), _ptrs(), _ptrs(base=8192), 6, _ptrs(12, base=16384), _ptrs(12, base=32768), 12)
    why = lib.fleet_sactrain_last_error(None).decode()
    assert rc == _capi.ERR_INVALID and why.startswith("fleet_sactrain_sac_dev: ") and word in why, why


def test_the_update_refuses_null_structs_arrays_and_aliases_and_names_the_null_handle():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fn = lib.fleet_sactrain_sac_dev
    last = lambda: lib.fleet_sactrain_last_error(None).decode()  # noqa: E731
    P, G, Q, H = _ptrs(), _ptrs(base=8192), _ptrs(12, base=16384), _ptrs(12, base=32768)
    a = C.byref(_args())
    assert fn(None, None, P, G, 6, Q, H, 12) == _capi.ERR_INVALID and last() == "fleet_sactrain_sac_dev: null FleetSacTrainArgs"
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
    fixed = dict(log_ent_coef=None, log_ent_coef_grad=None, ent_coef=1024)
    for ok in (_args(), _args(**fixed), _args(tau=0.0), _args(tau=1.0), _args(lr=0.0), _args(norm=None), _args(loss_scale=1.0),
               _args(loss_scale=0.0), _args(target_update_interval=2 ** 31 - 1), _args(target_entropy=NAN, **fixed),
               _args(gradient_steps=2 ** 31 - 1, batch_size=2 ** 31 - 1, seed=2 ** 64 - 1, target_seed=2 ** 64 - 1, first_update=2 ** 63,
                     max_grad_norm=(2, 0.5))):
        assert fn(None, C.byref(ok), P, G, 6, Q, H, 12) == _capi.ERR_INVALID and last() == "fleet_sactrain_sac_dev: null handle"


def test_create_describe_alpha_scale_and_polyak_refuse_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_sactrain_last_error(None).decode()  # noqa: E731
    h = C.c_void_p()
    fake = C.c_void_p(4096)  # (never dereferenced: the null handle in front of it is met first)
    good = _capi.FleetSacTrainParams(C.sizeof(_capi.FleetSacTrainParams), 1024)
    create = lib.fleet_sactrain_create
    for k, word in enumerate(("null replay handle", "null target networks handle", "null gradient handle", "null actor optimiser handle",
                              "null critic optimiser handle")):
        handles = [fake] * k + [None] + [fake] * (4 - k)
        assert create(*handles, None, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h
        assert last() == "fleet_sactrain_create: " + word
    assert create(None, None, None, None, None, None, C.byref(good), None) == _capi.ERR_INVALID and last() == "fleet_sactrain_create: null output handle"
    assert create(None, None, None, None, None, None, None, C.byref(h)) == _capi.ERR_INVALID
    assert last() == "fleet_sactrain_create: null FleetSacTrainParams"
    for p, word in ((_capi.FleetSacTrainParams(4, 8), "FleetSacTrainParams.struct_bytes does not match this library"),
                    (_capi.FleetSacTrainParams(8, 0), "max_steps must be in 1..65536, got 0"),
                    (_capi.FleetSacTrainParams(8, -1), "max_steps must be in 1..65536, got -1"),
                    (_capi.FleetSacTrainParams(8, 65537), "max_steps must be in 1..65536, got 65537")):
        assert create(fake, fake, fake, fake, fake, fake, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
        assert last() == "fleet_sactrain_create: " + word
    assert lib.fleet_sactrain_destroy(None) == _capi.OK
    assert lib.fleet_sactrain_describe(None, None) == _capi.ERR_INVALID
    for tau, word in ((1.5, "tau must be in [0, 1], got 1.5"), (-0.25, "tau must be in [0, 1], got -0.25"), (NAN, "tau must be in [0, 1], got"),
                      (0.0, "null handle"), (1.0, "null handle"), (0.005, "null handle")):
        assert lib.fleet_sactrain_polyak_dev(None, tau) == _capi.ERR_INVALID
        assert last().startswith("fleet_sactrain_polyak_dev: ") and word in last(), last()
    for x, out, word in ((None, fake, "null log_ent_coef"), (fake, fake, "null handle"), (fake, None, "null handle")):
        assert lib.fleet_sactrain_alpha_dev(None, x, out) == _capi.ERR_INVALID
        assert last() == "fleet_sactrain_alpha_dev: " + word
    Q = _ptrs(12, base=16384)
    for grads, n, s, word in ((Q, 12, NAN, "the scale must be finite"), (Q, 12, INF, "the scale must be finite"), (None, 12, 0.5, "null grads"),
                              (Q, 0, 0.5, "count must be in 1..24, got 0"), (_ptrs(25), 25, 0.5, "count must be in 1..24, got 25"),
                              (_ptrs(12, null_at=5), 12, 0.5, "gradient tensor 5 is null"), (Q, 12, 0.5, "null handle"), (Q, 12, 1.0, "null handle")):
        assert lib.fleet_sactrain_scale_dev(None, grads, n, s) == _capi.ERR_INVALID
        assert last() == "fleet_sactrain_scale_dev: " + word


# ---- the schedule --------------------------------------------------------------------------------------------------------------------
def sb3_target_steps(n_updates: int, gradient_steps: int, target_update_interval: int) -> list:
    """SB3 2.3.2's SAC.train, restated from its semantics: `for gradient_step in range(gradient_steps): ...; if gradient_step %
    self.target_update_interval == 0: polyak_update(...)`, then `self._n_updates += gradient_steps` -- the loop variable's values at which
    the branch runs.  The update count does not enter."""
    del n_updates
    hits = []
    for gradient_step in range(gradient_steps):
        if gradient_step % target_update_interval == 0:
            hits.append(gradient_step)
    return hits


def test_the_target_update_schedule_is_sb3s():
    for first in (0, 1, 3, 2 ** 40 + 1):
        for G in range(1, 8):
            for interval in range(1, 5):
                hits = sm.target_steps(G, interval)
                assert hits == sb3_target_steps(first, G, interval), (first, G, interval)
                assert len(hits) == sm.target_updates(G, interval) == (G - 1) // interval + 1 and hits[0] == 0
    assert sm.target_steps(5, 2) == [0, 2, 4] and sm.target_steps(5, 3) == [0, 3] and sm.target_steps(2, 3) == [0]


# ---- the closing launch's model ------------------------------------------------------------------------------------------------------
def _slots(G, rng):
    s = np.zeros((G, sm.SLOT), F32)
    s[:, 1], s[:, 2] = rng.random(G).astype(F32) * 3, rng.random(G).astype(F32) * 5
    s[:, 0] = s[:, 1] + s[:, 2]
    a = sm.ACTOR_AT
    s[:, a] = -rng.standard_normal(G).astype(F32) * 10
    s[:, a + 1] = rng.standard_normal(G).astype(F32) + 2
    s[:, a + 2] = rng.standard_normal(G).astype(F32) - 4
    s[:, a + 3] = rng.standard_normal(G).astype(F32) * 7 + 9
    s[:, a + 4] = np.exp(rng.standard_normal(G)).astype(F32)
    return s


@pytest.mark.parametrize("G", [1, 2, 255, 256, 257, 1024])
def test_the_finish_model_stays_within_the_bound_of_fsum(G):
    """|model - fsum| <= 8 max(eps_ref, 2^-53 sum|x|) per mean: eps_ref = |NumPy's float64 pairwise mean - fsum's|, and 2^-53 sum|x| is
    one rounding of a sum of that size; every mean is divided by its count after the sum, as the reference is.  The critic loss's factor
    0.5 is exact and is applied to the reference too."""
    a = sm.ACTOR_AT
    for interval, first, learned in ((1, 0, True), (2, 0, True), (3, 5, False)):
        s = _slots(G, np.random.default_rng(1000 * G + 10 * interval + first))
        got = sm.finish(s, first, interval, 0.5, learned)
        cols = [(0, s[:, 0], 0.5), (1, s[:, a], 1.0), (2, s[:, a + 4], 1.0), (8, s[:, a + 2], 1.0), (9, s[:, a + 3], 1.0)]
        if learned:
            cols.append((3, s[:, a + 1], 1.0))
        for k, x, f in cols:
            x64 = x.astype(F64)
            ref = f * math.fsum(x64.tolist()) / x64.size
            eps_ref = abs(f * float(x64.sum()) / x64.size - ref)
            bound = 8 * max(eps_ref, 2.0 ** -53 * f * float(np.abs(x64).sum()) / x64.size)
            print(f"G={G} interval={interval} first={first} [{k}]: model {abs(got[k] - ref):.3g} eps_ref {eps_ref:.3g} bound {bound:.3g}")
            assert abs(got[k] - ref) <= bound
        assert np.isnan(got[3]) == (not learned)
        assert got[4] == 0.5 * F64(s[G - 1, 0]) and got[5] == F64(s[G - 1, a]) and got[6] == first + G
        assert got[7] == (G - 1) // interval + 1 and not got[10:].any()


@pytest.mark.parametrize("G", [1, 2, 255, 256, 257, 1024])
def test_the_finish_model_is_exact_on_constant_slots(G):
    s = np.zeros((G, sm.SLOT), F32)
    a = sm.ACTOR_AT
    s[:, 0], s[:, a], s[:, a + 1], s[:, a + 2], s[:, a + 3], s[:, a + 4] = F32(1.5), F32(-2.25), F32(0.75), F32(-3.5), F32(4.0), F32(0.25)
    got = sm.finish(s, 7, 2, 0.5, True)
    assert dict(zip(SAC_TRAIN_STATS, got)) == dict(critic_loss=0.75, actor_loss=-2.25, ent_coef=0.25, ent_coef_loss=0.75, last_critic_loss=0.75,
                                                   last_actor_loss=-2.25, n_updates=float(7 + G), target_updates=float((G - 1) // 2 + 1),
                                                   log_prob_mean=-3.5, qmin_mean=4.0)
    assert np.isnan(sm.finish(s, 7, 2, 0.5, False)[3])
    assert sm.finish(s, 0, 1, 0.3, True)[0] == F64(F32(0.3)) * 1.5  # the factor is the float32 one


# ---- the alpha launch's value --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", [-20.0, -1.6094379, 0.0, 0.5, 2.0])
def test_alpha_is_the_double_exponential_rounded_once(x):
    """(float)exp((double)x) restated in NumPy: the float32 nearest to the float64 exponential of the float32 x -- within half an ulp of
    math.exp, so never further than one ulp from a float32 exponential that is itself within one ulp."""
    x32 = F32(x)
    got = sm.alpha32(x)
    assert got.dtype == F32 and got == F32(math.exp(float(x32)))
    exact = math.exp(float(x32))
    assert abs(float(got) - exact) <= 0.5 * float(np.spacing(got)) * (1 + 2.0 ** -20)
    assert abs(int(got.view(np.int32)) - int(np.exp(x32).astype(F32).view(np.int32))) <= 1  # NumPy's float32 exp: within one ulp
    if x == 0.0:
        assert got == F32(1.0)


# ---- two misreadings of SB3's loop against the bound ------------------------------------------------------------------------------------
def _cpu_case():
    import sac_grad_model as gm

    shape = "7-64-64-A5-relu"
    c = sm.parity_inputs(shape, 0)
    rng = np.random.default_rng(99)
    B, D, A, G = c["B"], c["D"], c["A"], sm.PARITY["G"]
    batches = [(np.clip(rng.standard_normal((B, D)), -3, 3).astype(F32), rng.uniform(-1, 1, (B, A)).astype(F32),
                np.clip(rng.standard_normal((B, D)), -3, 3).astype(F32), (rng.random(B) < 0.2).astype(F32), rng.standard_normal(B).astype(F32))
               for _ in range(G)]
    noise = [np.clip(rng.standard_normal((B, A)), -2.5, 2.5).astype(F32) for _ in range(G)]
    target_noise = [np.clip(rng.standard_normal((B, A)), -2.5, 2.5).astype(F32) for _ in range(G)]
    kw = dict(activation=c["activation"], gamma=sm.PARITY["gamma"], tau=sm.PARITY["tau"], lr=sm.PARITY["lr"], interval=sm.PARITY["interval"],
              log_ent_coef=c["log_ent_coef"])
    nets = (c["actor"], c["critics"], c["actor"], c["target_critics"], batches, noise, target_noise)
    run = lambda **more: sm.sac_train_reference(*nets, **dict(kw, **more))  # noqa: E731
    return gm, run, nets, kw


def test_the_reference_follows_the_schedule_and_each_misreading_leaves_a_tensor_class_outside_the_bound():
    gm, run, _, _ = _cpu_case()
    r64, r32 = run(dtype="float64"), run(dtype="float32")
    assert r64["stats"]["updated"] == [True, False, True, False]
    own = sm.class_ratios(r32, r64, r32)
    assert all(v <= 1.0 for v in own.values()), own  # the float32 reading is inside its own bound (by construction: 1/8 at most)
    for mutant in sm.MUTANTS:
        m = run(dtype="float64", mutant=mutant)
        worst = sm.class_ratios(m, r64, r32)
        print(mutant, {k: round(float(v), 3) for k, v in worst.items()})
        assert max(worst.values()) > 1.0, (mutant, worst)
    assert run(dtype="float64", mutant="polyak_on_update_count")["stats"]["updated"] == [False, True, False, True]


def test_the_reference_at_interval_1_is_the_existing_loop():
    gm, run, nets, kw = _cpu_case()
    kw = {k: v for k, v in kw.items() if k != "interval"}
    old = gm.sac_gradient_steps(*nets, **kw)
    new = run(dtype="float64", interval=1)
    for k in sm.TENSOR_CLASSES:
        assert all(np.array_equal(x, y) for x, y in zip(old[k], new[k])), k
    assert new["stats"]["updated"] == [True] * sm.PARITY["G"]
