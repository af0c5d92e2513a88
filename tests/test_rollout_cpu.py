"""The rollout buffer without a GPU: the C ABI's declarations and bindings, fleet_rollout_layout, the parameter checks of
fleet_rollout_create (made before the device is touched), and the NumPy model of tests/rollout_model.py pinned by known answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rollout_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("fleet_rollout_layout", "fleet_rollout_create", "fleet_rollout_destroy", "fleet_rollout_last_error",
           "fleet_rollout_set_stream", "fleet_rollout_slot", "fleet_rollout_add_dev", "fleet_rollout_finish_dev",
           "fleet_rollout_gather_dev", "fleet_rollout_arrays", "fleet_rollout_check_errors")


def test_header_declares_the_entries_under_abi_11_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_rollout_\w+)\s*\(", hdr, flags=re.M)) - {"fleet_rollout_policy_dev"}
    assert declared == set(ENTRIES) == set(_capi.ROLLOUT_SYMBOLS)
    section = hdr[hdr.index("rollout buffer on the device"):]
    assert "added under FLEET_ABI_VERSION 11" in section[:400]
    for struct in ("FleetRolloutParams", "FleetRolloutLayout", "FleetRolloutArrays", "FleetRolloutSlot"):
        assert f"}} {struct};" in section
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert fn.restype is (C.c_char_p if name == "fleet_rollout_last_error" else C.c_int), name
    assert set(ENTRIES) <= set(_capi.EXPORTED_SYMBOLS)


def test_struct_sizes_match_the_header(tmp_path):
    import subprocess

    from fleetrl_amd import _capi

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu", '
                   'sizeof(FleetRolloutParams), offsetof(FleetRolloutParams, gamma), sizeof(FleetRolloutLayout), '
                   'offsetof(FleetRolloutLayout, error_offset), sizeof(FleetRolloutArrays), sizeof(FleetRolloutSlot));return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P, L = _capi.FleetRolloutParams, _capi.FleetRolloutLayout
    assert got == [C.sizeof(P), P.gamma.offset, C.sizeof(L), L.error_offset.offset, C.sizeof(_capi.FleetRolloutArrays),
                   C.sizeof(_capi.FleetRolloutSlot)]


@pytest.mark.parametrize("E,K,D,A", [(1, 1, 1, 1), (7, 3, 37, 5), (4096, 192, 388, 50)])
def test_layout_gives_the_models_sizes_and_aligned_offsets(E, K, D, A):
    from fleetrl_amd import _capi

    L = _capi.rollout_layout(E, K, D, A)
    want = rm.layout(E, K, D, A)
    assert L.struct_bytes == C.sizeof(_capi.FleetRolloutLayout) and L.alignment == 256 == _capi.ROLLOUT_ALIGN
    assert _capi.ROLLOUT_ARRAY_NAMES == rm.ARRAYS
    end = 0
    for i, n in enumerate(rm.ARRAYS):
        assert (L.offset[i], L.bytes[i], L.row_bytes[i]) == (want[n]["offset"], want[n]["bytes"], want[n]["row_bytes"]), n
        assert L.offset[i] % 256 == 0 and L.offset[i] >= end and L.bytes[i] == K * L.row_bytes[i]
        end = L.offset[i] + L.bytes[i]
    itemsize = {"episode_starts": 1}
    per_env = {"obs": D, "actions": A}
    for i, n in enumerate(rm.ARRAYS):
        assert L.bytes[i] == K * E * per_env.get(n, 1) * itemsize.get(n, 4)
    assert L.error_offset == want["error_offset"] >= end and L.error_offset % 256 == 0
    assert L.total_bytes == want["total_bytes"] >= L.error_offset + 4


def _params(**over):
    from fleetrl_amd import _capi

    kw = dict(struct_bytes=C.sizeof(_capi.FleetRolloutParams), num_envs=8, n_steps=4, obs_dim=5, act_dim=2, reserved=0, gamma=0.99,
              gae_lambda=0.95)
    kw.update(over)
    return _capi.FleetRolloutParams(**kw)


@pytest.mark.parametrize("bad", [dict(num_envs=0), dict(num_envs=-3), dict(n_steps=0), dict(obs_dim=0), dict(act_dim=0), dict(act_dim=-1),
                                 dict(gamma=-0.01), dict(gamma=1.0001), dict(gamma=float("nan")), dict(gae_lambda=-1e-9),
                                 dict(gae_lambda=1.5), dict(gae_lambda=float("nan")), dict(struct_bytes=0), dict(struct_bytes=44),
                                 dict(num_envs=1 << 20, n_steps=1 << 11)])
def test_create_refuses_bad_parameters_before_it_touches_the_device(bad):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    h = C.c_void_p(0xdead)
    assert lib.fleet_rollout_create(0, C.byref(_params(**bad)), C.byref(h)) == _capi.ERR_INVALID
    assert h.value is None
    why = lib.fleet_rollout_last_error(None).decode()
    key = next(iter(bad))
    assert ("num_envs * n_steps" if len(bad) == 2 else key) in why, why
    assert lib.fleet_rollout_layout(C.byref(_params(**bad)), C.byref(_capi.FleetRolloutLayout())) == _capi.ERR_INVALID
    assert lib.fleet_rollout_create(0, None, C.byref(h)) == _capi.ERR_INVALID
    assert lib.fleet_rollout_create(0, C.byref(_params()), None) == _capi.ERR_INVALID


def test_python_class_raises_invalid_for_bad_parameters():
    from fleetrl_amd import DeviceRolloutBuffer, FleetHipError, _capi

    with pytest.raises(FleetHipError) as ei:
        DeviceRolloutBuffer(8, 4, 5, 2, gamma=1.5)
    assert ei.value.status == _capi.ERR_INVALID and "gamma" in str(ei.value)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _data(rng, K, E):
    mag = lambda: (rng.choice([-1.0, 1.0], (K, E)) * 10.0 ** rng.uniform(-6, 4, (K, E))).astype(np.float32)  # noqa: E731
    return mag(), mag(), (rng.choice([-1.0, 1.0], E) * 10.0 ** rng.uniform(-6, 4, E)).astype(np.float32)


def test_model_known_answer_by_hand():
    """K = 2, E = 1, numbers that are exact in float32: gamma = 0.5, lambda = 0.5."""
    r = np.array([[1.0], [2.0]], np.float32)
    v = np.array([[0.5], [0.25]], np.float32)
    s = np.zeros((2, 1), np.uint8)
    adv, ret = rm.gae(r, v, s, np.array([4.0], np.float32), np.array([0], np.uint8), 0.5, 0.5)
    # t=1: delta = 2 + 0.5*4 - 0.25 = 3.75; last = 3.75.   t=0: delta = 1 + 0.5*0.25 - 0.5 = 0.625; last = 0.625 + 0.25*3.75 = 1.5625
    assert adv.tolist() == [[1.5625], [3.75]] and ret.tolist() == [[2.0625], [4.0]]
    adv, _ = rm.gae(r, v, s, np.array([4.0], np.float32), np.array([1], np.uint8), 0.5, 0.5)  # done: no bootstrap from last_values
    assert adv.tolist() == [[0.625 + 0.25 * 1.75], [1.75]]


@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.5])
def test_model_lambda_one_is_discounted_reward_to_go(gamma):
    """lambda = 1, no episode boundary: advantages[t] = sum_k g^(k-t) r[k] + g^(K-t) last_value - values[t] (the values in between
    telescope), g = float32(gamma).  Bound: every row performs 7 float32 operations, each off by at most 2^-24 of an intermediate
    that the sum of the operands' magnitudes bounds; the error of row t+1 enters row t times g."""
    rng = np.random.default_rng(11)
    K, E = 61, 37
    r, v, lv = _data(rng, K, E)
    adv, _ = rm.gae(r, v, np.zeros((K, E), np.uint8), lv, np.zeros(E, np.uint8), gamma, 1.0)
    g = float(np.float32(gamma))
    togo, bound = lv.astype(np.float64), np.zeros(E)
    r64, v64 = r.astype(np.float64), v.astype(np.float64)
    nv = lv.astype(np.float64)
    for t in reversed(range(K)):
        last_above = togo - nv  # the exact "last" of row t+1
        mag = np.abs(r64[t]) + np.abs(nv) + np.abs(v64[t]) + np.abs(last_above)
        togo = r64[t] + g * togo
        bound = 8 * 2.0 ** -24 * (mag + np.abs(togo - v64[t])) + g * bound
        assert np.all(np.abs(adv[t].astype(np.float64) - (togo - v64[t])) <= bound), t
        nv = v64[t]


def test_model_gamma_zero_is_reward_minus_value_exactly():
    rng = np.random.default_rng(12)
    r, v, lv = _data(rng, 33, 20)
    s = (rng.random((33, 20)) < 0.1).astype(np.uint8)
    adv, ret = rm.gae(r, v, s, lv, np.zeros(20, np.uint8), 0.0, 0.95)
    assert np.array_equal(adv.view(np.uint32), (r - v).view(np.uint32))


def test_model_episode_start_cuts_the_recurrence():
    rng = np.random.default_rng(13)
    K, E, t = 40, 9, 17
    r, v, lv = _data(rng, K, E)
    s = np.zeros((K, E), np.uint8)
    s[t + 1] = 1
    a0, _ = rm.gae(r, v, s, lv, np.zeros(E, np.uint8), 0.99, 0.95)
    r2, v2, lv2 = _data(rng, K, E)
    r2[:t + 1], v2[:t + 1] = r[:t + 1], v[:t + 1]  # rows > t change, rows <= t stay
    a1, _ = rm.gae(r2, v2, s, lv2, np.ones(E, np.uint8), 0.99, 0.95)
    assert np.array_equal(a0[:t + 1].view(np.uint32), a1[:t + 1].view(np.uint32))
    assert not np.array_equal(a0[t + 1:], a1[t + 1:])
    s[t + 1, 0] = 0  # ... and without the start, env 0's rows <= t do change
    a2, _ = rm.gae(r2, v2, s, lv2, np.ones(E, np.uint8), 0.99, 0.95)
    assert not np.array_equal(a0[:t + 1, 0], a2[:t + 1, 0]) and np.array_equal(a1[:, 1:].view(np.uint32), a2[:, 1:].view(np.uint32))


def test_model_returns_minus_advantages_is_values():
    rng = np.random.default_rng(14)
    r, v, lv = _data(rng, 50, 31)
    s = (rng.random((50, 31)) < 0.05).astype(np.uint8)
    adv, ret = rm.gae(r, v, s, lv, (rng.random(31) < 0.5).astype(np.uint8), 0.99, 0.95)
    assert adv.dtype == ret.dtype == np.float32
    assert np.array_equal(ret.view(np.uint32), (adv + v).view(np.uint32))


def test_model_add_rounds_once_and_bootstraps_done_rows_only():
    m = rm.RolloutModel(4, 2, 3, 2, gamma=0.99)
    rew = np.array([0.1, 1.0 + 2.0 ** -30, -3.3, 1e-9])
    z = np.zeros(4, np.float32)
    m.add(np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32), rew, np.zeros(4, np.uint8), z, z)
    assert np.array_equal(m.rewards[0], rew.astype(np.float32)) and m.rewards[0, 1] == 1.0
    tv = np.array([10.0, 20.0, 30.0, 40.0], np.float32)
    m.add(np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32), rew, np.zeros(4, np.uint8), z, z, tv, np.array([0, 1, 0, 1], np.uint8))
    want = rew.astype(np.float32)
    want[[1, 3]] = want[[1, 3]] + np.float32(0.99) * tv[[1, 3]]
    assert np.array_equal(m.rewards[1].view(np.uint32), want.view(np.uint32))
    idx = np.array([0, 1, 2, 7])  # i = e * K + t
    assert np.array_equal(m.sample(idx)[2], m.values[[0, 1, 0, 1], [0, 0, 1, 3]])
