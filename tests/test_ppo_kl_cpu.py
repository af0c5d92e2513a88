"""PPO's early stopping on approx_kl without a GPU: the new entries' declarations, bindings and struct layouts against a compiled probe,
that the existing entry lists are what they were, every refusal that needs no device, and the statistics model of
tests/ppo_kl_model.py against a plain float64 evaluation written here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ppo_kl_model as klm
import train_model as tm

ROOT = klm.ROOT
F32, F64 = np.float32, np.float64
ENTRIES = ("fleet_ppo_grad_gated_dev", "fleet_adam_step_gated_dev", "fleet_adam_settle_dev", "fleet_train_ppo_kl_dev")
GATE_FIELDS = ["skip", "decided", "threshold"]
GRAD_FIELDS = ["struct_bytes", "clip_range_vf", "old_values", "gate", "base"]
TRAIN_FIELDS = ["struct_bytes", "clip_range_vf", "target_kl", "base"]
NAN, INF = float("nan"), float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "fleet_hip.h")).read()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_are_declared_in_their_sections_bound_and_exported():
    from fleetrl_amd import _capi, build

    hdr = _header()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    assert hdr.count('#define FLEET_API __attribute__((visibility("default")))') == 1
    assert hdr.index("#define FLEET_API") < hdr.index("/* ---- lifetime")
    declared = re.findall(r"^FLEET_API int\s+(fleet_\w+)\s*\(", hdr, flags=re.M)
    assert sorted(declared) == sorted(ENTRIES) and _capi.KL_SYMBOLS == ENTRIES
    train = hdr[hdr.index("---- PPO's whole update on the device"):hdr.index("---- Adam and clip_grad_norm_ on the device")]
    adam = hdr[hdr.index("---- Adam and clip_grad_norm_ on the device"):hdr.index("---- TD3 / DDPG minibatch gradients on the device")]
    ppo = hdr[hdr.index("---- PPO minibatch gradients on the device"):]
    assert "} FleetTrainPpoKlArgs;" in train and "FLEET_API int fleet_train_ppo_kl_dev(" in train
    assert train.index("extern int fleet_train_describe_vclip(") < train.index("/* -- the update with early stopping on approx_kl")
    assert "FLEET_API int fleet_adam_step_gated_dev(" in adam and "FLEET_API int fleet_adam_settle_dev(" in adam
    assert adam.index("int fleet_adam_export_image_dev(") < adam.index("/* -- a step the device may skip")
    assert "} FleetPpoGate;" in ppo and "} FleetPpoGradGatedArgs;" in ppo and "FLEET_API int fleet_ppo_grad_gated_dev(" in ppo
    assert ppo.index("extern int fleet_ppo_grad_vclip_dev(") < ppo.index("/* -- the same behind a gate")
    flat = lambda text: re.sub(r"\s*\n \*\s*", " ", text)  # noqa: E731  (a comment's line breaks do not matter)
    train, adam = flat(train), flat(adam)
    for said in ("(double)approx_kl > thr", "a NaN does NOT stop", "STOPPING minibatch's gradients", "NOT capturable",
                 "NO launch reads a word that a workgroup of the SAME launch may write", "[9] optimiser steps taken", "[10] epochs entered",
                 "[11] 1.0 if the update stopped early", "[12] approx_kl of the last minibatch that ran", "[13] the mean of approx_kl",
                 "slot [13] of fleet_train_ppo_kl_dev"):
        assert said in train, said
    for said in ("write NOTHING", "Settling on use", "pinned host memory", "no kernel writes host memory", "FLEET_ERR_STATE"):
        assert said in adam, said
    lib = C.CDLL(build.build())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert len(lib.fleet_ppo_grad_gated_dev.argtypes) == 4 and len(lib.fleet_train_ppo_kl_dev.argtypes) == 5
    assert len(lib.fleet_adam_step_gated_dev.argtypes) == 6 and len(lib.fleet_adam_settle_dev.argtypes) == 3


def test_the_existing_entry_lists_are_what_they_were():
    from fleetrl_amd import _capi

    assert _capi.PPO_SYMBOLS == ("fleet_ppo_create", "fleet_ppo_destroy", "fleet_ppo_last_error", "fleet_ppo_describe", "fleet_ppo_grad_dev")
    assert _capi.TRAIN_SYMBOLS == ("fleet_train_create", "fleet_train_destroy", "fleet_train_last_error", "fleet_train_describe",
                                   "fleet_train_ppo_dev", "fleet_train_indices_dev")
    assert _capi.ADAM_SYMBOLS == ("fleet_adam_create_policy", "fleet_adam_create_qtarget", "fleet_adam_destroy", "fleet_adam_last_error",
                                  "fleet_adam_describe", "fleet_adam_step_dev", "fleet_adam_state_dev", "fleet_adam_export_image_dev")
    assert _capi.VCLIP_SYMBOLS == ("fleet_ppo_grad_vclip_dev", "fleet_train_ppo_vclip_dev", "fleet_train_describe_vclip")
    assert not set(ENTRIES) & (set(_capi.EXPORTED_SYMBOLS) | set(_capi.VCLIP_SYMBOLS))
    hdr = _header()
    assert set(re.findall(r"^(?:int|const char\*)\s+(fleet_\w+)\s*\(", hdr, flags=re.M)) == set(_capi.EXPORTED_SYMBOLS)
    assert len(_capi.EXPORTED_SYMBOLS) == len(set(_capi.EXPORTED_SYMBOLS))
    assert set(re.findall(r"^extern int\s+(fleet_\w+)\s*\(", hdr, flags=re.M)) == set(_capi.VCLIP_SYMBOLS)
    graft = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_capi.EXPORTED_SYMBOLS + _capi.VCLIP_SYMBOLS + _capi.KL_SYMBOLS" in graft


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetPpoGate", _capi.FleetPpoGate, GATE_FIELDS), ("FleetPpoGradGatedArgs", _capi.FleetPpoGradGatedArgs, GRAD_FIELDS),
                               ("FleetTrainPpoKlArgs", _capi.FleetTrainPpoKlArgs, TRAIN_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["sizeof(FleetPpoGradArgs)", "sizeof(FleetTrainPpoArgs)", "sizeof(FleetAdamStepArgs)", "FLEET_TRAIN_STATS"]
    want += [96, 96, C.sizeof(_capi.FleetAdamStepArgs), 16]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert C.sizeof(_capi.FleetPpoGate) == 24 and C.sizeof(_capi.FleetPpoGradGatedArgs) == 136 and C.sizeof(_capi.FleetTrainPpoKlArgs) == 112
    assert dict(_capi.FleetPpoGradGatedArgs._fields_)["base"] is _capi.FleetPpoGradArgs
    assert dict(_capi.FleetTrainPpoKlArgs._fields_)["base"] is _capi.FleetTrainPpoArgs


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _set(a, kw):
    for k, v in kw.items():
        if k.startswith("base_"):
            setattr(a.base, k[5:], v)
        elif k.startswith("gate_"):
            setattr(a.gate, k[5:], v)
        else:
            setattr(a, k, v)
    return a


def _grad_args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetPpoGradGatedArgs()
    a.struct_bytes, a.clip_range_vf, a.old_values = C.sizeof(a), 0.0, None  # (nothing is dereferenced: nothing is launched)
    a.gate.skip, a.gate.decided, a.gate.threshold = 512, 516, 0.015
    b = a.base
    b.struct_bytes, b.B, b.clip_range, b.vf_coef, b.ent_coef = C.sizeof(b), 4, 0.2, 0.5, 0.0
    b.obs = b.actions = b.old_log_prob = b.advantages = b.returns = b.log_std = b.stats = 256
    return _set(a, kw)


def _train_args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetTrainPpoKlArgs()
    a.struct_bytes, a.clip_range_vf, a.target_kl = C.sizeof(a), 0.0, 0.01
    b = a.base
    b.struct_bytes, b.n_epochs, b.batch_size, b.normalize_advantage = C.sizeof(b), 2, 64, 1
    b.clip_range, b.vf_coef, b.ent_coef, b.lr, b.beta1, b.beta2, b.eps, b.max_grad_norm = 0.2, 0.5, 0.0, 3e-4, 0.9, 0.999, 1e-5, 0.5
    b.seed, b.first_epoch, b.stats = 1, 0, 4096
    return _set(a, kw)


def _step_args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetAdamStepArgs()
    a.struct_bytes, a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = C.sizeof(a), 3e-4, 0.9, 0.999, 1e-5, 0.5
    return _set(a, kw)


def _ptrs(n=5, base=256):
    return (C.c_void_p * n)(*[base + 64 * i for i in range(n)])


KL_WORDS = "target_kl must be finite and > 0"
VF_WORDS = "clip_range_vf must be finite and >= 0 (0: no value clip)"
TRAIN_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=104), "FleetTrainPpoKlArgs.struct_bytes does not match this library"),
    "base-struct_bytes": (dict(base_struct_bytes=112), "FleetTrainPpoArgs.struct_bytes does not match this library"),
    "base-reserved": (dict(base_reserved=1), "reserved must be 0"),
    "base-n_epochs": (dict(base_n_epochs=0), "n_epochs must be >= 1, got 0"),
    "base-null-stats": (dict(base_stats=None), "null stats"),
    "kl-zero": (dict(target_kl=0.0), KL_WORDS),
    "kl-negative": (dict(target_kl=-0.01), KL_WORDS),
    "kl-nan": (dict(target_kl=NAN), KL_WORDS),
    "kl-inf": (dict(target_kl=INF), KL_WORDS),
    "vf-negative": (dict(clip_range_vf=-0.2), VF_WORDS),
    "vf-nan": (dict(clip_range_vf=NAN), VF_WORDS),
    "vf-inf": (dict(clip_range_vf=INF), VF_WORDS),
}
GRAD_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=112), "FleetPpoGradGatedArgs.struct_bytes does not match this library"),
    "base-struct_bytes": (dict(base_struct_bytes=136), "FleetPpoGradArgs.struct_bytes does not match this library"),
    "base-B": (dict(base_B=0), "B must be >= 1, got 0"),
    "base-null-returns": (dict(base_returns=None), "null returns"),
    "vf-negative": (dict(clip_range_vf=-0.2), VF_WORDS),
    "vf-nan": (dict(clip_range_vf=NAN), VF_WORDS),
    "vf-without-old_values": (dict(clip_range_vf=0.2), "null old_values"),
    "null-skip": (dict(gate_skip=None), "null gate.skip"),
    "null-decided": (dict(gate_decided=None), "null gate.decided"),
    "one-word": (dict(gate_decided=512), "gate.skip and gate.decided are the same word"),
    "nan-threshold": (dict(gate_threshold=NAN), "gate.threshold is NaN"),
}


@pytest.mark.parametrize("case", sorted(TRAIN_REFUSALS))
def test_the_update_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = TRAIN_REFUSALS[case]
    assert lib.fleet_train_ppo_kl_dev(None, C.byref(_train_args(**fields)), _ptrs(), _ptrs(base=8192), 5) == _capi.ERR_INVALID
    assert lib.fleet_train_last_error(None).decode() == "fleet_train_ppo_kl_dev: " + word


@pytest.mark.parametrize("case", sorted(GRAD_REFUSALS))
def test_the_gradient_entry_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = GRAD_REFUSALS[case]
    assert lib.fleet_ppo_grad_gated_dev(None, C.byref(_grad_args(**fields)), _ptrs(), 5) == _capi.ERR_INVALID
    assert lib.fleet_ppo_last_error(None).decode() == "fleet_ppo_grad_gated_dev: " + word


def test_null_structs_null_words_and_the_null_handle_are_named():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    ppo = lambda: lib.fleet_ppo_last_error(None).decode()  # noqa: E731
    train = lambda: lib.fleet_train_last_error(None).decode()  # noqa: E731
    adam = lambda: lib.fleet_adam_last_error(None).decode()  # noqa: E731
    P, G = _ptrs(), _ptrs(base=8192)
    assert lib.fleet_ppo_grad_gated_dev(None, None, P, 5) == _capi.ERR_INVALID and ppo() == "fleet_ppo_grad_gated_dev: null FleetPpoGradGatedArgs"
    assert lib.fleet_ppo_grad_gated_dev(None, C.byref(_grad_args()), None, 5) == _capi.ERR_INVALID and ppo().endswith("null grads")
    for kw in (dict(), dict(clip_range_vf=0.2, old_values=1024), dict(gate_threshold=INF), dict(gate_threshold=-1.0)):  # all pass the checks
        assert lib.fleet_ppo_grad_gated_dev(None, C.byref(_grad_args(**kw)), P, 5) == _capi.ERR_INVALID
        assert ppo() == "fleet_ppo_grad_gated_dev: null handle"
    assert lib.fleet_train_ppo_kl_dev(None, None, P, G, 5) == _capi.ERR_INVALID and train() == "fleet_train_ppo_kl_dev: null FleetTrainPpoKlArgs"
    assert lib.fleet_train_ppo_kl_dev(None, C.byref(_train_args()), P, P, 5) == _capi.ERR_INVALID and "is its own gradient" in train()
    for kw in (dict(), dict(clip_range_vf=0.2), dict(target_kl=1e-300), dict(target_kl=1e300)):
        assert lib.fleet_train_ppo_kl_dev(None, C.byref(_train_args(**kw)), P, G, 5) == _capi.ERR_INVALID
        assert train() == "fleet_train_ppo_kl_dev: null handle"
    # the optimiser's two entries
    assert lib.fleet_adam_step_gated_dev(None, None, P, G, 5, 512) == _capi.ERR_INVALID and adam() == "fleet_adam_step_gated_dev: null FleetAdamStepArgs"
    assert lib.fleet_adam_step_gated_dev(None, C.byref(_step_args(lr=-1.0)), P, G, 5, 512) == _capi.ERR_INVALID
    assert adam() == "fleet_adam_step_gated_dev: lr must be finite and >= 0"
    assert lib.fleet_adam_step_gated_dev(None, C.byref(_step_args()), P, G, 5, None) == _capi.ERR_INVALID and adam() == "fleet_adam_step_gated_dev: null skip"
    assert lib.fleet_adam_step_gated_dev(None, C.byref(_step_args()), P, G, 5, 512) == _capi.ERR_INVALID and adam() == "fleet_adam_step_gated_dev: null handle"
    assert lib.fleet_adam_settle_dev(None, -1, 512) == _capi.ERR_INVALID and adam() == "fleet_adam_settle_dev: base_step must be >= 0, got -1"
    assert lib.fleet_adam_settle_dev(None, 3, None) == _capi.ERR_INVALID and adam() == "fleet_adam_settle_dev: null steps_taken"
    assert lib.fleet_adam_settle_dev(None, 3, 512) == _capi.ERR_INVALID and adam() == "fleet_adam_settle_dev: null handle"
    # the existing entries answer as before
    assert lib.fleet_train_ppo_dev(None, C.byref(_train_args().base), P, G, 5) == _capi.ERR_INVALID and train() == "fleet_train_ppo_dev: null handle"
    assert lib.fleet_ppo_grad_dev(None, C.byref(_grad_args().base), P, 5) == _capi.ERR_INVALID and ppo() == "fleet_ppo_grad_dev: null handle"
    assert lib.fleet_adam_step_dev(None, C.byref(_step_args()), P, G, 5) == _capi.ERR_INVALID and adam() == "fleet_adam_step_dev: null handle"


# ---- Python ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, -0.01, NAN, INF])
def test_python_refuses_a_target_kl_that_is_not_positive_and_finite(bad):
    from fleetrl_amd import DevicePPOTrain
    from fleetrl_amd.train import check_target_kl

    with pytest.raises(ValueError, match="`target_kl` must be positive and finite"):
        check_target_kl(bad)
    self = object.__new__(DevicePPOTrain)  # the check runs before anything touches a handle or a device
    with pytest.raises(ValueError, match="`target_kl` must be positive and finite"):
        self.train([], n_epochs=1, batch_size=1, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, lr=0.0, seed=0, first_epoch=0, target_kl=bad)


def test_python_carries_the_arguments_and_the_new_statistics_names():
    from fleetrl_amd import DeviceAdam, DevicePPOGrad, DevicePPOTrain, train
    from fleetrl_amd.train import check_target_kl

    assert check_target_kl(None) is None and check_target_kl(0.01) == 0.01 and check_target_kl(1) == 1.0
    for fn, name in ((DevicePPOTrain.train, "target_kl"), (DevicePPOGrad.grad, "gate")):
        p = inspect.signature(fn).parameters[name]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(DeviceAdam.step).parameters["skip"].default is None
    assert train.STATS == tm.STATS and len(train.SB3_NAMES) == len(train.STATS) == 9  # the pinned tuples are what they were
    assert train.KL_STATS == klm.KL_STATS and len(train.KL_SB3_NAMES) == len(train.KL_STATS) == 5
    assert len(train.STATS) + len(train.KL_STATS) == 14 and all(n.startswith("train/") for n in train.KL_SB3_NAMES)
    assert not set(train.KL_SB3_NAMES) & set(train.SB3_NAMES)


# ---- the statistics model --------------------------------------------------------------------------------------------------------
def _rows(kls, seed=0):
    """One f32[8] row per minibatch with the given approx_kl and arbitrary other statistics."""
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((len(kls), 8)).astype(F32)
    out[:, klm.KL] = np.asarray(kls, dtype=F32)
    out[:, 6:] = 0
    return list(out)


def _plain(rows, per_epoch, thr, ev, std):
    """The same block from SB3's loop, written independently: lists that are appended to, a break, numpy means replaced by the ordered
    float64 sum the header states."""
    lists = {k: [] for k in tm.STATS[:5]}
    steps = epochs = 0
    stop, losses, cont = None, [], True
    kls = []
    n_epochs = -(-len(rows) // per_epoch)
    i = 0
    for _ in range(n_epochs):
        kls = []
        epochs += 1
        for row in rows[i:i + per_epoch]:
            d = dict(zip(tm.GRAD_STATS, (float(x) for x in np.asarray(row, dtype=F32)[:6])))  # float32 -> float64, exact
            for k in lists:
                lists[k].append(d[k])
            losses.append(d["loss"])
            kls.append(d["approx_kl"])
            if d["approx_kl"] > float(thr):
                cont, stop = False, i
                break
            steps += 1
            i += 1
        if not cont:
            break
    ordered = lambda xs: float(sum((F64(x) for x in xs), F64(0.0)))  # noqa: E731  (left to right from 0.0)
    ran = len(losses)
    out = [ordered(lists[k]) / ran for k in tm.STATS[:5]] + [losses[-1], float(ran), ev, std, float(steps), float(epochs),
                                                             0.0 if cont else 1.0, kls[-1], ordered(kls) / len(kls), 0.0, 0.0]
    return stop, np.array(out, dtype=F64)


def same64(a, b):
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


SEQ = [0.0, 0.002, 0.001, 0.004, 0.003, 0.003, 0.009, 0.005, 0.012, 0.011, 0.010, 0.02]  # 3 epochs of 4; records at 0, 1, 3, 6, 8, 11
MODEL_CASES = {
    "no-stop": (SEQ, 4, 1.0, None),
    "stop-at-0": ([0.5] + SEQ[1:], 4, 0.1, 0),
    "stop-in-epoch-0": (SEQ, 4, 0.003, 3),
    "stop-at-an-epochs-first": (SEQ, 4, 0.0105, 8),
    "stop-in-a-later-epoch": (SEQ, 4, 0.007, 6),
    "stop-on-the-last": (SEQ, 4, 0.015, 11),
    "nan-does-not-stop": ([0.0, NAN, 0.001, NAN, 0.003, 0.2, 0.1], 3, 0.05, 5),
    "all-nan": ([NAN] * 5, 2, 0.01, None),
    "equal-does-not-stop": ([0.25, 0.25, 0.5], 3, 0.25, 2),
    "one-minibatch-per-epoch": ([0.0, 0.1, 0.3, 0.2], 1, 0.25, 2),
    "short-last-epoch": (SEQ[:10], 4, 1.0, None),
}


@pytest.mark.parametrize("case", sorted(MODEL_CASES))
def test_the_statistics_model_equals_a_plain_float64_evaluation_of_sb3s_loop(case):
    kls, per_epoch, thr, want_stop = MODEL_CASES[case]
    rows = _rows(kls, seed=len(case))
    stop, block = klm.stats_block(rows, per_epoch, thr, ev=0.25, std=0.5)
    ref_stop, ref = _plain(rows, per_epoch, thr, 0.25, 0.5)
    assert stop == ref_stop == want_stop
    assert same64(block, ref) or (np.isnan(block) == np.isnan(ref)).all() and same64(np.nan_to_num(block), np.nan_to_num(ref)), (block, ref)
    ran = len(kls) if stop is None else stop + 1
    assert block[6] == ran and block[9] == (ran if stop is None else stop) and block[11] == (stop is not None)
    assert block[10] == (ran - 1) // per_epoch + 1 and not block[14:].any()
    last = np.asarray(rows[ran - 1], dtype=F32)
    assert same64(block[12], F64(last[klm.KL])) or np.isnan(block[12]) and np.isnan(last[klm.KL])
    assert same64(block[5], F64(last[klm.LOSS]))
    if stop is None and not np.isnan(kls).any():  # without a stop slots 0..8 are the existing model's
        assert same64(block[:9], tm.stats_block(rows, 0.25, 0.5)[:9])


def test_records_and_the_threshold_that_stops_at_one():
    assert klm.records(SEQ) == [0, 1, 3, 6, 8, 11] and klm.records([NAN, 0.1, NAN, 0.2]) == [1, 3]
    for r in klm.records(SEQ)[1:]:
        t = klm.target_for(SEQ, r)
        thr = klm.threshold(t)
        assert max(SEQ[:r]) < thr < SEQ[r] and klm.stats_block(_rows(SEQ), 4, thr)[0] == r
        assert [i for i, x in enumerate(SEQ) if klm.stops(x, thr)][0] == r
    assert klm.threshold(0.01) == 1.5 * 0.01 and not klm.stops(NAN, 0.0) and klm.stops(F32(0.1), 0.1) is True  # float32(0.1) > 0.1
    assert not klm.stops(0.25, 0.25)
