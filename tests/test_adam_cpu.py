"""The optimiser step without a GPU: the C ABI's section, bindings and struct layouts against a compiled probe, every refusal that needs
no device, the bit model of tests/adam_model.py against torch's own clip_grad_norm_ + Adam in float64 under the project's rule, known
answers, and the conditions every case of the GPU table must meet."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adam_model as am

torch = pytest.importorskip("torch")

ROOT = am.ROOT
F32 = np.float32
ENTRIES = ("fleet_adam_create_policy", "fleet_adam_create_qtarget", "fleet_adam_destroy", "fleet_adam_last_error", "fleet_adam_describe",
           "fleet_adam_step_dev", "fleet_adam_state_dev", "fleet_adam_export_image_dev")
PARAM_FIELDS = ["struct_bytes", "first_net", "n_nets", "n_extra", "extra_len"]
STEP_FIELDS = ["struct_bytes", "lr", "beta1", "beta2", "eps", "max_grad_norm", "norm_out"]
INFO_FIELDS = ["state_bytes", "n_elements", "step", "n_tensors", "norm_chunk", "step_tile", "reserved"]
TITLE = "Adam and clip_grad_norm_ on the device"
TARGETS_TITLE = "TD3 / DDPG learning targets on the device"
TD3_TITLE = "TD3 / DDPG minibatch gradients on the device"
PPO_TITLE = "PPO minibatch gradients on the device"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_lies_between_the_targets_and_the_td3_gradients_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_adam_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.ADAM_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    assert hdr.count(TITLE) == 1 and hdr.count(TD3_TITLE) == 1 and hdr.count(PPO_TITLE) == 1 and hdr.count(TARGETS_TITLE) == 1
    assert hdr.index(TARGETS_TITLE) < hdr.index("int fleet_qtarget_describe(") < hdr.index(TITLE) < hdr.index(TD3_TITLE) < hdr.index(PPO_TITLE)
    section = hdr[hdr.index(TITLE):hdr.index(TD3_TITLE)]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    for struct in ("} FleetAdamParams;", "} FleetAdamStepArgs;", "} FleetAdamInfo;", "#define FLEET_ADAM_MAX_EXTRA 2"):
        assert struct in section
    assert not re.search(r"^(?:int|const char\*)\s+fleet_(?!adam_)", section, flags=re.M)  # no entry of a neighbour in it
    assert len(re.findall(r"^/\* ---- ", section[len(TITLE):], flags=re.M)) == 1  # the next section's opening, and none between
    for said in ("m' = fmaf(g' - m, omb1, m)", "v' = fmaf(g' * omb2, g', v * b2)", "den = sqrtf(v') / bs + eps", "p' = fmaf(m' / den, nstep, p)",
                 "nstep = -(lr / (1 - beta1^t))", "bs = sqrt(1 - beta2^t)", "q = maxn32 / (norm + 1e-6f);  c = q > 1.0f ? 1.0f : q",
                 "off = 32, 16, 8, 4, 2, 1", "((wave 0 + wave 1) + wave 2) + wave 3", "in ascending chunk order", "never straddles",
                 "NOT written back", "must outlive", "IMAGE handle's stream", "NOT bit-equal", "applied even when c == 1"):
        assert said in section, said
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_adam_step_dev.argtypes) == 5 and len(lib.fleet_adam_state_dev.argtypes) == 6
    assert len(lib.fleet_adam_create_policy.argtypes) == 3 and len(lib.fleet_adam_create_qtarget.argtypes) == 3
    assert len(lib.fleet_adam_describe.argtypes) == 3


def test_no_entry_carries_another_familys_prefix_and_the_class_is_exported():
    import fleetrl_amd
    from fleetrl_amd import _capi, build

    for other in (_capi.POLICY_SYMBOLS, _capi.EXPLORE_SYMBOLS, _capi.ROLLOUT_SYMBOLS, _capi.QTARGET_SYMBOLS, _capi.PPO_SYMBOLS,
                  _capi.TD3_SYMBOLS, _capi.NOISE_SYMBOLS):
        assert not set(other) & set(_capi.ADAM_SYMBOLS)
    assert all(n.startswith("fleet_adam_") for n in _capi.ADAM_SYMBOLS)
    assert "fleet_adam.hip" in build.SOURCES and "fleet_adam.h" in build.HEADERS
    assert fleetrl_amd.DeviceAdam.__name__ == "DeviceAdam" and fleetrl_amd.DeviceAdam._prefix == "adam"


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetAdamParams", _capi.FleetAdamParams, PARAM_FIELDS), ("FleetAdamStepArgs", _capi.FleetAdamStepArgs, STEP_FIELDS),
                               ("FleetAdamInfo", _capi.FleetAdamInfo, INFO_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["FLEET_ADAM_MAX_EXTRA", "FLEET_ADAM_STATE_EXPORT", "FLEET_ADAM_STATE_LOAD"]
    want += [_capi.ADAM_MAX_EXTRA, _capi.ADAM_STATE_EXPORT, _capi.ADAM_STATE_LOAD]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert C.sizeof(_capi.FleetAdamParams) == 24 and C.sizeof(_capi.FleetAdamStepArgs) == 56 and C.sizeof(_capi.FleetAdamInfo) == 40


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetAdamStepArgs()
    a.struct_bytes, a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = C.sizeof(a), 3e-4, 0.9, 0.999, 1e-8, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _ptrs(n=4, null_at=None, base=256):
    """(never dereferenced: nothing is launched)"""
    return (C.c_void_p * n)(*[None if i == null_at else base + 64 * i for i in range(n)])


STEP_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=48), "struct_bytes"),
    "lr-negative": (dict(lr=-1e-3), "lr must be finite and >= 0"),
    "lr-nan": (dict(lr=float("nan")), "lr must be finite and >= 0"),
    "lr-inf": (dict(lr=float("inf")), "lr must be finite and >= 0"),
    "eps-negative": (dict(eps=-1e-8), "eps must be finite and >= 0"),
    "eps-inf": (dict(eps=float("inf")), "eps must be finite and >= 0"),
    "eps-nan": (dict(eps=float("nan")), "eps must be finite and >= 0"),
    "beta1-one": (dict(beta1=1.0), "beta1 must be in [0, 1)"),
    "beta1-negative": (dict(beta1=-0.1), "beta1 must be in [0, 1)"),
    "beta1-nan": (dict(beta1=float("nan")), "beta1 must be in [0, 1)"),
    "beta2-one": (dict(beta2=1.0), "beta2 must be in [0, 1)"),
    "beta2-negative": (dict(beta2=-1e-9), "beta2 must be in [0, 1)"),
    "max_grad_norm-nan": (dict(max_grad_norm=float("nan")), "max_grad_norm is NaN"),
}


@pytest.mark.parametrize("case", sorted(STEP_REFUSALS))
def test_step_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_adam_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = STEP_REFUSALS[case]
    assert lib.fleet_adam_step_dev(None, C.byref(_args(**fields)), _ptrs(), _ptrs(base=8192), 4) == _capi.ERR_INVALID
    why = lib.fleet_adam_last_error(None).decode()
    assert why.startswith("fleet_adam_step_dev: ") and word in why, why


def test_step_refuses_null_structs_arrays_and_aliases_and_names_the_null_handle():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fn = lib.fleet_adam_step_dev
    last = lambda: lib.fleet_adam_last_error(None).decode()  # noqa: E731
    P, G = _ptrs(), _ptrs(base=8192)
    assert fn(None, None, P, G, 4) == _capi.ERR_INVALID and last() == "fleet_adam_step_dev: null FleetAdamStepArgs"
    assert fn(None, C.byref(_args()), None, G, 4) == _capi.ERR_INVALID and "null params" in last()
    assert fn(None, C.byref(_args()), P, None, 4) == _capi.ERR_INVALID and "null grads" in last()
    assert fn(None, C.byref(_args()), P, G, 0) == _capi.ERR_INVALID and "count" in last()
    assert fn(None, C.byref(_args()), _ptrs(27), _ptrs(27, base=8192), 27) == _capi.ERR_INVALID and "count" in last()  # above 2 * 3 * 4 + 2
    assert fn(None, C.byref(_args()), _ptrs(null_at=2), G, 4) == _capi.ERR_INVALID and "parameter tensor 2 is null" in last()
    assert fn(None, C.byref(_args()), P, _ptrs(null_at=3, base=8192), 4) == _capi.ERR_INVALID and "gradient tensor 3 is null" in last()
    alias = _ptrs(base=8192)
    alias[1] = P[1]
    assert fn(None, C.byref(_args()), P, alias, 4) == _capi.ERR_INVALID and "parameter tensor 1 is its own gradient" in last()
    for ok in (_args(), _args(max_grad_norm=0.0), _args(max_grad_norm=-1.0), _args(lr=0.0, eps=0.0, beta1=0.0, beta2=0.0), _args(norm_out=256)):
        assert fn(None, C.byref(ok), P, G, 4) == _capi.ERR_INVALID and last() == "fleet_adam_step_dev: null handle"


@pytest.mark.parametrize("entry", ["fleet_adam_create_policy", "fleet_adam_create_qtarget"])
def test_create_refuses_bad_parameters_before_it_looks_at_the_image(entry):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    create = getattr(lib, entry)
    last = lambda: lib.fleet_adam_last_error(None).decode()  # noqa: E731

    def P(first=0, n=1, n_extra=0, lens=(0, 0), size=None):
        p = _capi.FleetAdamParams()
        p.struct_bytes, p.first_net, p.n_nets, p.n_extra = C.sizeof(p) if size is None else size, first, n, n_extra
        p.extra_len[0], p.extra_len[1] = lens
        return p

    h = C.c_void_p()
    noun = "policy" if entry.endswith("policy") else "networks"
    for p, word in ((None, "null FleetAdamParams"), (P(size=16), "struct_bytes"), (P(first=-1), "span of nets"), (P(n=-1), "span of nets"),
                    (P(first=4), "span of nets"), (P(n=4), "span of nets"), (P(n_extra=3, lens=(1, 1)), "n_extra must be in 0..2, got 3"),
                    (P(n_extra=-1), "n_extra"), (P(n_extra=1, lens=(0, 0)), "extra_len[0] must be in 1..16777216, got 0"),
                    (P(n_extra=2, lens=(5, -2)), "extra_len[1] must be in 1..16777216, got -2"),
                    (P(n_extra=1, lens=((1 << 24) + 1, 0)), "extra_len[0]"), (P(n=0), "nothing to optimise"),
                    (P(), f"null {noun} handle"), (P(n=0, n_extra=1, lens=(1025, 0)), f"null {noun} handle")):
        assert create(None, C.byref(p) if p is not None else None, C.byref(h)) == _capi.ERR_INVALID and not h
        assert last().startswith(entry + ": ") and word in last(), last()
    assert create(None, C.byref(P()), None) == _capi.ERR_INVALID and "null output handle" in last()
    assert lib.fleet_adam_destroy(None) == _capi.OK
    assert lib.fleet_adam_describe(None, None, None) == _capi.ERR_INVALID
    assert lib.fleet_adam_export_image_dev(None, None, 0) == _capi.ERR_INVALID and last() == "fleet_adam_export_image_dev: null handle"


def test_state_entry_refuses_bad_arguments_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fn = lib.fleet_adam_state_dev
    last = lambda: lib.fleet_adam_last_error(None).decode()  # noqa: E731
    M, V, step = _ptrs(), _ptrs(base=8192), C.c_int64(0)
    for args, word in (((2, M, V, 4, C.byref(step)), "unknown mode 2"), ((0, None, V, 4, C.byref(step)), "null exp_avg"),
                       ((0, M, None, 4, C.byref(step)), "null exp_avg_sq"), ((0, M, V, 4, None), "null step"),
                       ((0, M, V, 0, C.byref(step)), "count"), ((1, _ptrs(null_at=1), V, 4, C.byref(step)), "exp_avg tensor 1 is null"),
                       ((1, M, _ptrs(null_at=0), 4, C.byref(step)), "exp_avg_sq tensor 0 is null"),
                       ((1, M, V, 4, C.byref(C.c_int64(-1))), "step must be >= 0, got -1"), ((1, M, V, 4, C.byref(step)), "null handle")):
        assert fn(None, *args) == _capi.ERR_INVALID
        assert last().startswith("fleet_adam_state_dev: ") and word in last(), last()


# ---- the model against torch ---------------------------------------------------------------------------------------------------------
PAIRS = [(name, first, n, clip) for name in sorted(am.CASES) for _, first, n in am.spans(name) for clip in (True, False)]


@pytest.mark.parametrize("name,first,n,clip", PAIRS)
def test_the_model_stays_within_the_projects_bound_of_torchs_float64_adam(name, first, n, clip):
    """Per tensor and per step: |model - torch64| <= 8 max(eps_ref, 2^-24 max|torch64|), eps_ref = |torch32 - torch64|."""
    got, r64, r32 = am.run(name, first, n, clip), am.torch_reference(name, first, n, clip, True), am.torch_reference(name, first, n, clip, False)
    for s in range(am.STEPS):
        ratios = am.bound_ratios(got[s], r64[s], r32[s])
        print(name, first, n, clip, s, ratios)
        assert all(r <= 1.0 for r in ratios.values()), (s, ratios)


# ---- known answers -------------------------------------------------------------------------------------------------------------------
def test_known_answer_the_first_step_moves_every_parameter_by_lr_against_the_gradients_sign():
    """From a zero state m' = (1 - b1) g and v' = (1 - b2) g^2, so m_hat / sqrt(v_hat) = sign(g) when |g| >> eps."""
    g = [np.array([[0.5, -2.0, 1e-3], [7.0, -0.25, 3.0]], F32), np.array([-1.0, 40.0], F32)]
    p = [np.array([[1.0, -1.0, 0.5], [0.25, 2.0, -3.0]], F32), np.array([0.0, 10.0], F32)]
    zero = [np.zeros_like(a) for a in p]
    P, M, V, norm = am.step(p, g, zero, zero, 1, lr=1e-2, eps=1e-8)
    for a, b, c in zip(P, p, g):
        assert np.abs((a - b) - F32(-1e-2) * np.sign(c)).max() <= 2.0 ** -23 * 10.0 + 1e-2 * 1e-4  # a rounding of p, and eps / |g|
    assert float(norm) == pytest.approx(math.sqrt(sum(float((a.astype(np.float64) ** 2).sum()) for a in g)), rel=1e-6)
    assert all(np.allclose(m, 0.1 * c, rtol=1e-6) for m, c in zip(M, g)) and all(np.allclose(v, 1e-3 * c * c, rtol=1e-5) for v, c in zip(V, g))


def test_known_answer_the_clip_coefficient_is_exactly_one_below_the_threshold_and_a_nan_stays():
    assert am.clip_coef(F32(0.25), 0.5) == F32(1.0) and am.clip_coef(F32(0.4999), 0.5) == F32(1.0)
    assert am.clip_coef(F32(0.5), 0.5) < F32(1.0)  # the 1e-6: at the threshold the gradients already shrink
    assert am.clip_coef(F32(1.0), 0.5) == F32(0.5) / (F32(1.0) + F32(1e-6))
    assert np.isnan(am.clip_coef(F32(np.nan), 0.5)) and am.clip_coef(F32(np.inf), 0.5) == 0.0
    g, p = [np.array([0.3, -0.1], F32)], [np.array([1.0, 2.0], F32)]
    zero = [np.zeros(2, F32)]
    a, b = am.step(p, g, zero, zero, 1, lr=1e-3, max_grad_norm=0.5), am.step(p, g, zero, zero, 1, lr=1e-3, max_grad_norm=None)
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]  # c == 1: g * 1 is g
    nan = am.step(p, [np.array([np.nan, -0.1], F32)], zero, zero, 1, lr=1e-3, max_grad_norm=0.5)
    assert np.isnan(nan[0][0]).all() and np.isnan(nan[3])
    only = am.step(p, [np.array([np.nan, -0.1], F32)], zero, zero, 1, lr=1e-3, max_grad_norm=None)
    assert np.isnan(only[0][0][0]) and only[0][0][1] == b[0][0][1]


def test_known_answer_a_loaded_step_count_changes_the_bias_corrections_as_computed_by_hand():
    k1, k1001 = am.scalars(1, 3e-4, (0.9, 0.999), 1e-8), am.scalars(1001, 3e-4, (0.9, 0.999), 1e-8)
    assert k1["nstep"] == F32(-3e-4 / 0.1) or abs(float(k1["nstep"]) + 3e-3) < 1e-9
    assert float(k1["bs"]) == pytest.approx(math.sqrt(1e-3), rel=1e-6)
    assert float(k1001["nstep"]) == pytest.approx(-3e-4, rel=1e-6)  # 0.9^1001 ~ 1.6e-46
    assert float(k1001["bs"]) == pytest.approx(math.sqrt(1.0 - math.exp(1001 * math.log(0.999))), rel=1e-6)
    assert 0.79 < float(k1001["bs"]) < 0.80
    assert k1["omb1"] == F32(1 - 0.9) and k1["omb2"] == F32(1 - 0.999) and k1["b2"] == F32(0.999) and k1["eps"] == F32(1e-8)


def test_known_answer_the_norms_order_is_the_stated_one_and_not_numpys():
    """One chunk of 1024 with a large first element: the butterfly's order gives other bits than a left-to-right float32 sum."""
    rng = np.random.default_rng(5)
    g = rng.standard_normal(1024).astype(F32)
    part = am.chunk_partials(g)
    assert part.shape == (1,) and float(part[0]) == pytest.approx(float((g.astype(np.float64) ** 2).sum()), rel=1e-6)
    assert am.chunk_partials(np.concatenate([g, g[:1]])).shape == (2,)
    assert am.chunk_partials(g[:1023])[0] == am.chunk_partials(np.concatenate([g[:1023], np.zeros(1, F32)]))[0]
    two = am.grad_norm([g, g[:1]])
    assert float(two) == pytest.approx(math.sqrt(float((g.astype(np.float64) ** 2).sum()) + float(g[0]) ** 2), rel=1e-6)


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------
def test_the_case_table_was_drawn_for_the_librarys_chunk_and_tile():
    """A later change of either launch shape fails here (and, through describe(), in the GPU tests) instead of losing the edges."""
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_adam.h")).read()
    assert re.search(r"constexpr int kAdamChunk = (\d+);", src).group(1) == str(am.CHUNK)
    assert re.search(r"constexpr int kAdamTile = (\d+);", src).group(1) == str(am.TILE)
    assert re.search(r"constexpr int kAdamThreads = (\d+);", src).group(1) == str(am.THREADS)
    assert (am.CHUNK, am.TILE, am.THREADS) == (1024, 32, 256) and am.FLAT_LEN == am.CHUNK + 1
    assert am.SCALES == (3.0, 1e-3, 0.2, 40.0, 1e-2, 1.0) and am.MAX_GRAD_NORM == 0.5 and am.STEPS == 6


@pytest.mark.parametrize("name", sorted(am.CASES))
def test_every_case_meets_the_tables_conditions(name):
    facts = am.facts_of(name)
    print(name, sorted(facts))
    assert all(facts.values()), facts
    c = am.CASES[name]
    assert max(max(sizes) for sizes in c["nets"]) <= 129
    for _, first, n in am.spans(name):
        for clip in (True, False):
            assert all(np.isfinite(a).all() for r in am.run(name, first, n, clip) for part in r[:3] for a in part)
