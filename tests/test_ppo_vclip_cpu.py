"""PPO's value-function clipping without a GPU: the float64 model of tests/ppo_vclip_model.py against torch float64 autograd of SB3's
own expression, the tie rule, the conditions every case of the GPU table must meet, the new entries' declarations, bindings and struct
layouts against a compiled probe, every refusal that needs no device, and that the existing entries are what they were."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ppo_model as ppm
import ppo_vclip_model as vcm

torch = pytest.importorskip("torch")

ROOT = vcm.ROOT
ENTRIES = ("fleet_ppo_grad_vclip_dev", "fleet_train_ppo_vclip_dev", "fleet_train_describe_vclip")
GRAD_FIELDS = ["struct_bytes", "clip_range_vf", "old_values", "base"]
TRAIN_FIELDS = ["struct_bytes", "clip_range_vf", "base"]
NAN, INF = float("nan"), float("inf")


# ---- the model against autograd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_analytic_gradients_equal_float64_autograd_of_sb3s_clipped_loss(name):
    """Both sides are float64 and the operations are the same: rounding noise separates them, 1e-12 relative (the tolerance of
    tests/test_ppo_grad_cpu.py for the unclipped loss)."""
    for B in ppm.CASES[name][5]:
        m, t = vcm.model(name, B), vcm.torch_loss_and_grads(*vcm.batch_args(vcm.case(name), B))
        assert len(m["grads"]) == len(t["grads"]) == len(ppm.tensor_names(name))
        for n, g, r in zip(ppm.tensor_names(name), m["grads"], t["grads"]):
            assert g.shape == r.shape and g.dtype == np.float64
            assert np.abs(g - r).max() <= 1e-12 * max(np.abs(r).max(), 1e-300), (name, B, n)
        for k in ppm.STATS:
            assert abs(m["stats"][k] - t["stats"][k]) <= 1e-12 * max(abs(t["stats"][k]), 1.0), (name, B, k)


@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_every_case_meets_the_tables_conditions(name):
    c = vcm.case(name)
    facts = vcm.facts_of(name, c["old_values"])
    assert all(facts.values()) and 0 <= c["vclip_salt"] < vcm.MAX_SALT == 8, facts
    assert vcm.seed(name, 3) == __import__("zlib").crc32(f"ppo-vclip/{name}/3".encode()) and vcm.CLIP_RANGE_VF == 0.2
    assert c["old_values"].dtype == np.float32 and c["old_values"].shape == (ppm.ROWS,)
    m = vcm.model(name, ppm.ROWS)
    dl = m["dl"]
    assert (dl[:16] > 0.2).any() and (dl[:16] < -0.2).any() and m["inside"].sum() >= ppm.ROWS // 4
    margin = float(np.abs(np.abs(dl) - 0.2).min())
    print(f"{name}: salt {c['vclip_salt']}, {int(m['inside'].sum())} of {ppm.ROWS} rows inside, smallest margin {margin:.3g}")
    assert margin > 1e-4 and np.abs(dl).max() <= vcm.SPREAD + 1e-6
    assert all(np.isfinite(g).all() for g in m["grads"])
    # the clip bites: the critic's tensors and the value loss differ from the unclipped model's, the rest is the unclipped model's
    u = ppm.model(name, ppm.ROWS)
    na = 2 * (len(ppm.CASES[name][2]) + 1)
    assert all(np.array_equal(a, b) for a, b in zip(m["grads"][:na], u["grads"][:na])) and np.array_equal(m["grads"][-1], u["grads"][-1])
    assert all(not np.array_equal(a, b) for a, b in zip(m["grads"][na:-1], u["grads"][na:-1]))
    assert m["stats"]["value_loss"] != u["stats"]["value_loss"] and m["stats"]["policy_loss"] == u["stats"]["policy_loss"]
    assert np.array_equal(m["values"], u["values"])


@pytest.mark.parametrize("name", sorted(ppm.CASES))
def test_a_range_nothing_reaches_gives_the_unclipped_models_gradients(name):
    B = ppm.CASES[name][5][-1]
    m, u = vcm.loss_and_grads(*vcm.batch_args(vcm.case(name), B), clip_range_vf=1e30), ppm.model(name, B)
    assert m["inside"].all()
    for n, g, r in zip(ppm.tensor_names(name), m["grads"], u["grads"]):
        # vp = old + (v - old) instead of v: one rounding of the critic's output apart
        assert np.abs(g - r).max() <= 1e-12 * max(np.abs(r).max(), 1e-300), (name, n)
    for k in ppm.STATS:
        assert abs(m["stats"][k] - u["stats"][k]) <= 1e-12 * max(abs(u["stats"][k]), 1.0), k


def test_the_two_ties_pass_their_gradient_and_the_two_clipped_rows_do_not():
    """v == 0.5, cv = 0.25, old = 0.25, 0.75, 0.0, 1.0: dl = +cv, -cv, +0.5, -0.5.  The model and torch agree, in both precisions."""
    c = vcm.tie_case()
    args = (c["actor"], c["critic"], "tanh", c["log_std"], c["obs"], c["actions"], c["old_log_prob"], c["advantages"], c["returns"],
            c["old_values"])
    m = vcm.loss_and_grads(*args, clip_range_vf=vcm.TIE_CV)
    assert np.array_equal(m["values"], [0.5] * 4) and np.array_equal(m["dl"], [0.25, -0.25, 0.5, -0.5])
    assert m["inside"].tolist() == [True, True, False, False] and np.array_equal(m["values_pred"], [0.5, 0.5, 0.25, 0.75])
    # db = sum over the two ties of (2 * 0.5 / 4) * (0.5 - ret) = 0.25 * (-0.5) + 0.25 * 1.0
    want_db = 0.25 * (0.5 - 1.0) + 0.25 * (0.5 + 0.5)
    assert m["grads"][3].tolist() == [want_db] == [0.125]
    assert np.array_equal(m["grads"][2][0], 0.25 * (-0.5) * c["obs"][0].astype(np.float64) + 0.25 * c["obs"][1].astype(np.float64))
    for dtype in ("float64", "float32"):
        t = vcm.torch_loss_and_grads(*args, clip_range_vf=vcm.TIE_CV, dtype=dtype)
        assert t["grads"][3].tolist() == [0.125], dtype
        tol = 0.0 if dtype == "float64" else 1e-6
        assert np.abs(t["grads"][2] - m["grads"][2]).max() <= tol + 1e-15
        assert abs(t["stats"]["value_loss"] - m["stats"]["value_loss"]) <= 1e-6
    # torch's clamp backward on its own: ties pass, NaN does not
    x = torch.tensor([0.25, -0.25, 0.5, -0.5, NAN], dtype=torch.float64, requires_grad=True)
    torch.clamp(x, -0.25, 0.25).nansum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "fleet_hip.h")).read()


def test_the_new_entries_are_declared_bound_and_exported_and_the_old_ones_are_what_they_were():
    from fleetrl_amd import _capi

    hdr = _header()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^extern int\s+(fleet_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.VCLIP_SYMBOLS)
    assert _capi.PPO_SYMBOLS == ("fleet_ppo_create", "fleet_ppo_destroy", "fleet_ppo_last_error", "fleet_ppo_describe", "fleet_ppo_grad_dev")
    assert _capi.TRAIN_SYMBOLS == ("fleet_train_create", "fleet_train_destroy", "fleet_train_last_error", "fleet_train_describe",
                                   "fleet_train_ppo_dev", "fleet_train_indices_dev")
    assert not set(ENTRIES) & set(_capi.EXPORTED_SYMBOLS)
    ppo = hdr[hdr.index("---- PPO minibatch gradients on the device"):]
    train = hdr[hdr.index("---- PPO's whole update on the device"):hdr.index("---- Adam and clip_grad_norm_ on the device")]
    assert "} FleetPpoGradVclipArgs;" in ppo and "extern int fleet_ppo_grad_vclip_dev(" in ppo
    assert ppo.index("int fleet_ppo_grad_dev(") < ppo.index("} FleetPpoGradVclipArgs;")
    for said in ("dl  = v - ov", "cd  = dl < -cv ? -cv : (dl > cv ? cv : dl)", "vp  = ov + cd", "inside = (dl >= -cv && dl <= cv)",
                 "dv  = inside ? ((2.0f * vf_coef) * invB) * (vp - ret) : 0.0f", "values[b] stays the unclipped v"):
        assert said in ppo, said
    assert "} FleetTrainPpoVclipArgs;" in train and "extern int fleet_train_ppo_vclip_dev(" in train
    assert "extern int fleet_train_describe_vclip(" in train and "still five launches" in train and "BEHIND" in train
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert len(lib.fleet_ppo_grad_vclip_dev.argtypes) == 4 and len(lib.fleet_train_ppo_vclip_dev.argtypes) == 5
    assert len(lib.fleet_train_describe_vclip.argtypes) == 2
    for name in _capi.PPO_SYMBOLS + _capi.TRAIN_SYMBOLS:
        assert hasattr(lib, name), name


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetPpoGradVclipArgs", _capi.FleetPpoGradVclipArgs, GRAD_FIELDS),
                               ("FleetTrainPpoVclipArgs", _capi.FleetTrainPpoVclipArgs, TRAIN_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["sizeof(FleetPpoGradArgs)", "sizeof(FleetTrainPpoArgs)", "sizeof(FleetTrainInfo)", "sizeof(FleetPpoParams)"]
    want += [96, 96, 56, 8]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert C.sizeof(_capi.FleetPpoGradVclipArgs) == 112 and C.sizeof(_capi.FleetTrainPpoVclipArgs) == 104
    assert dict(_capi.FleetPpoGradVclipArgs._fields_)["base"] is _capi.FleetPpoGradArgs
    assert dict(_capi.FleetTrainPpoVclipArgs._fields_)["base"] is _capi.FleetTrainPpoArgs
    assert C.sizeof(_capi.FleetPpoGradArgs) == 96 and C.sizeof(_capi.FleetTrainPpoArgs) == 96 and C.sizeof(_capi.FleetTrainInfo) == 56


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _grad_args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetPpoGradVclipArgs()
    a.struct_bytes, a.clip_range_vf, a.old_values = C.sizeof(a), 0.2, 256  # (never dereferenced: nothing is launched)
    b = a.base
    b.struct_bytes, b.B, b.clip_range, b.vf_coef, b.ent_coef = C.sizeof(b), 4, 0.2, 0.5, 0.0
    b.obs = b.actions = b.old_log_prob = b.advantages = b.returns = b.log_std = b.stats = 256
    for k, v in kw.items():
        setattr(b if k.startswith("base_") else a, k[5:] if k.startswith("base_") else k, v)
    return a


def _train_args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetTrainPpoVclipArgs()
    a.struct_bytes, a.clip_range_vf = C.sizeof(a), 0.2
    b = a.base
    b.struct_bytes, b.n_epochs, b.batch_size, b.normalize_advantage = C.sizeof(b), 2, 64, 1
    b.clip_range, b.vf_coef, b.ent_coef, b.lr, b.beta1, b.beta2, b.eps, b.max_grad_norm = 0.2, 0.5, 0.0, 3e-4, 0.9, 0.999, 1e-5, 0.5
    b.seed, b.first_epoch, b.stats = 1, 0, 4096
    for k, v in kw.items():
        setattr(b if k.startswith("base_") else a, k[5:] if k.startswith("base_") else k, v)
    return a


def _ptrs(n=5, base=256):
    return (C.c_void_p * n)(*[base + 64 * i for i in range(n)])


VF_WORDS = "clip_range_vf must be finite and > 0"
GRAD_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=96), "FleetPpoGradVclipArgs.struct_bytes does not match this library"),
    "base-struct_bytes": (dict(base_struct_bytes=112), "FleetPpoGradArgs.struct_bytes does not match this library"),
    "base-B": (dict(base_B=0), "B must be >= 1, got 0"),
    "base-null-returns": (dict(base_returns=None), "null returns"),
    "null-old_values": (dict(old_values=None), "null old_values"),
    "vf-zero": (dict(clip_range_vf=0.0), VF_WORDS),
    "vf-negative": (dict(clip_range_vf=-0.2), VF_WORDS),
    "vf-inf": (dict(clip_range_vf=INF), VF_WORDS),
    "vf-nan": (dict(clip_range_vf=NAN), VF_WORDS),
}
TRAIN_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=96), "FleetTrainPpoVclipArgs.struct_bytes does not match this library"),
    "base-struct_bytes": (dict(base_struct_bytes=104), "FleetTrainPpoArgs.struct_bytes does not match this library"),
    "base-reserved": (dict(base_reserved=1), "reserved must be 0"),
    "base-n_epochs": (dict(base_n_epochs=0), "n_epochs must be >= 1, got 0"),
    "vf-zero": (dict(clip_range_vf=0.0), VF_WORDS),
    "vf-negative": (dict(clip_range_vf=-1e-3), VF_WORDS),
    "vf-inf": (dict(clip_range_vf=INF), VF_WORDS),
    "vf-nan": (dict(clip_range_vf=NAN), VF_WORDS),
}


@pytest.mark.parametrize("case", sorted(GRAD_REFUSALS))
def test_the_gradient_entry_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = GRAD_REFUSALS[case]
    assert lib.fleet_ppo_grad_vclip_dev(None, C.byref(_grad_args(**fields)), _ptrs(), 5) == _capi.ERR_INVALID
    assert lib.fleet_ppo_last_error(None).decode() == "fleet_ppo_grad_vclip_dev: " + word


@pytest.mark.parametrize("case", sorted(TRAIN_REFUSALS))
def test_the_update_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = TRAIN_REFUSALS[case]
    assert lib.fleet_train_ppo_vclip_dev(None, C.byref(_train_args(**fields)), _ptrs(), _ptrs(base=8192), 5) == _capi.ERR_INVALID
    assert lib.fleet_train_last_error(None).decode() == "fleet_train_ppo_vclip_dev: " + word


def test_null_structs_and_the_null_handle_are_named():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    ppo = lambda: lib.fleet_ppo_last_error(None).decode()  # noqa: E731
    train = lambda: lib.fleet_train_last_error(None).decode()  # noqa: E731
    assert lib.fleet_ppo_grad_vclip_dev(None, None, _ptrs(), 5) == _capi.ERR_INVALID and ppo() == "fleet_ppo_grad_vclip_dev: null FleetPpoGradVclipArgs"
    assert lib.fleet_ppo_grad_vclip_dev(None, C.byref(_grad_args()), None, 5) == _capi.ERR_INVALID and ppo().endswith("null grads")
    assert lib.fleet_ppo_grad_vclip_dev(None, C.byref(_grad_args()), _ptrs(), 5) == _capi.ERR_INVALID and ppo() == "fleet_ppo_grad_vclip_dev: null handle"
    for cv in (1e-30, 0.2, 1e30):  # every positive finite range passes
        assert lib.fleet_ppo_grad_vclip_dev(None, C.byref(_grad_args(clip_range_vf=cv)), _ptrs(), 5) == _capi.ERR_INVALID
        assert ppo() == "fleet_ppo_grad_vclip_dev: null handle"
    P, G = _ptrs(), _ptrs(base=8192)
    assert lib.fleet_train_ppo_vclip_dev(None, None, P, G, 5) == _capi.ERR_INVALID
    assert train() == "fleet_train_ppo_vclip_dev: null FleetTrainPpoVclipArgs"
    assert lib.fleet_train_ppo_vclip_dev(None, C.byref(_train_args()), P, P, 5) == _capi.ERR_INVALID and "is its own gradient" in train()
    assert lib.fleet_train_ppo_vclip_dev(None, C.byref(_train_args()), P, G, 5) == _capi.ERR_INVALID
    assert train() == "fleet_train_ppo_vclip_dev: null handle"
    assert lib.fleet_train_describe_vclip(None, C.byref(C.c_uint64())) == _capi.ERR_INVALID
    # the existing entries answer as before
    a = _train_args().base
    assert lib.fleet_train_ppo_dev(None, C.byref(a), P, G, 5) == _capi.ERR_INVALID and train() == "fleet_train_ppo_dev: null handle"
    g = _grad_args().base
    assert lib.fleet_ppo_grad_dev(None, C.byref(g), _ptrs(), 5) == _capi.ERR_INVALID and ppo() == "fleet_ppo_grad_dev: null handle"


# ---- Python ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 0.0, -0.2, NAN, INF])
def test_python_refuses_a_clip_range_vf_that_is_not_positive_in_sb3s_words(bad):
    from fleetrl_amd.ppo import check_clip_range_vf

    with pytest.raises(ValueError, match="`clip_range_vf` must be positive, pass `None` to deactivate vf clipping"):
        check_clip_range_vf(bad)


def test_python_takes_none_and_positive_floats_and_both_methods_carry_the_argument():
    import inspect

    from fleetrl_amd import DevicePPOGrad, DevicePPOTrain
    from fleetrl_amd.ppo import check_clip_range_vf

    assert check_clip_range_vf(None) is None and check_clip_range_vf(0.2) == 0.2 and check_clip_range_vf(1) == 1.0
    for fn in (DevicePPOGrad.grad, DevicePPOTrain.train):
        p = inspect.signature(fn).parameters["clip_range_vf"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    # the check runs before anything touches a handle or a device
    for cls, method in ((DevicePPOGrad, "grad"), (DevicePPOTrain, "train")):
        self = object.__new__(cls)
        with pytest.raises(ValueError, match="must be positive"):
            if method == "grad":
                self.grad(None, None, 0.2, 0.5, 0.0, into=[], clip_range_vf=0.0)
            else:
                self.train([], n_epochs=1, batch_size=1, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, lr=0.0, seed=0, first_epoch=0,
                           clip_range_vf=-1.0)
