"""VecNormalize on the device, the parts that need no GPU: the model the GPU tests compare against, pinned to exact known
answers; persistence and SB3 import; the C ABI's exports and its parameter checks."""
import ctypes
import os
from fractions import Fraction as F
from types import SimpleNamespace

import numpy as np
import pytest

from fleetrl_amd import _capi
from fleetrl_amd.vec_normalize import NormSettings, NormState, RunningStats, load_state, normalize_obs_np, save_state, state_from_sb3
from vecnorm_model import RMS, VecNormModel

C0 = F(1, 10000)


def exact(rows):
    return np.array([[F(v) for v in r] for r in rows], dtype=object)


def pooled(batches, d):
    """Closed form: moments of all rows plus the prior pseudo-sample (count 1e-4, mean 0, var 1) in column d."""
    xs = [F(r[d]) for b in batches for r in b]
    N = C0 + len(xs)
    mean = sum(xs) / N
    return mean, (C0 * 1 + sum(x * x for x in xs)) / N - mean * mean, N


def test_known_answer_after_a_reset():
    m = VecNormModel(2, 1, exact=True)
    m.reset(exact([[1], [3]]))
    assert m.obs_rms.count == F(20001, 10000)
    assert m.obs_rms.mean[0] == F(40000, 20001)
    assert m.obs_rms.var[0] == F(400120001, 400040001)


def test_running_stats_after_a_reset_and_three_steps_equal_the_closed_form():
    rng = np.random.default_rng(3)
    batches = [rng.integers(-20, 20, size=(4, 3)).tolist() for _ in range(4)]
    rewards = [rng.integers(-5, 5, size=4).tolist() for _ in range(3)]
    m = VecNormModel(4, 3, gamma=F(1, 2), exact=True)
    m.reset(exact(batches[0]))
    returns = [F(0)] * 4
    ret_batches = []
    for k in range(3):
        m.step(exact(batches[k + 1]), np.array(rewards[k], dtype=np.float64), np.zeros(4, bool))
        returns = [g * F(1, 2) + F(r) for g, r in zip(returns, rewards[k])]
        ret_batches.append([[g] for g in returns])
    for d in range(3):
        mean, var, N = pooled(batches, d)
        assert (m.obs_rms.mean[d], m.obs_rms.var[d], m.obs_rms.count) == (mean, var, N)
    mean, var, N = pooled(ret_batches, 0)
    assert (m.ret_rms.mean, m.ret_rms.var, m.ret_rms.count) == (mean, var, N)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_running_merge_of_k_batches_equals_the_moments_of_their_concatenation(k):
    rng = np.random.default_rng(k)
    batches = [rng.integers(-9, 9, size=(int(rng.integers(1, 6)), 2)).tolist() for _ in range(k)]
    rms = RMS((2,), F(0), F(1), C0)
    for b in batches:
        rms.update(exact(b))
    for d in range(2):
        assert (rms.mean[d], rms.var[d], rms.count) == pooled(batches, d)


def test_observations_are_normalised_with_the_updated_statistics():
    m = VecNormModel(1, 1)
    o, _, _ = m.step(np.array([[5.0]]), np.zeros(1), np.zeros(1, bool))
    tot = 1e-4 + 1
    mean = 0.0 + (5.0 - 0.0) * 1 / tot
    var = (1.0 * 1e-4 + 0.0 * 1 + 25.0 * 1e-4 * 1 / tot) / tot
    assert o[0, 0] == np.float32(np.clip((5.0 - mean) / np.sqrt(var + 1e-8), -10, 10))
    assert abs(o[0, 0]) < 0.1  # normalised before the update it would be ~5


def test_returns_are_zeroed_after_the_ret_rms_update():
    m = VecNormModel(2, 1, gamma=F(1, 2), exact=True)
    m.step(exact([[0], [0]]), np.array([4.0, 2.0]), np.array([True, False]))
    assert m.returns[0] == 0 and m.returns[1] == 2
    # ret_rms saw the returns 4 and 2 (not 0 and 2)
    assert (m.ret_rms.mean, m.ret_rms.var, m.ret_rms.count) == pooled([[[4], [2]]], 0)


def test_ret_rms_advances_without_norm_reward_and_the_reward_passes_through():
    m = VecNormModel(3, 1, norm_reward=False)
    _, r, _ = m.step(np.zeros((3, 1)), np.array([1.0, 0.1, 100.0]), np.zeros(3, bool))
    assert m.ret_rms.count == 1e-4 + 3
    assert np.array_equal(r, np.array([1.0, 0.1, 100.0]).astype(np.float32).astype(np.float64))


def test_nothing_advances_without_training_but_done_returns_are_zeroed():
    m = VecNormModel(2, 2, gamma=F(1, 2), exact=True)
    m.returns = np.array([F(3), F(5)], dtype=object)
    m.training = False
    m.reset(exact([[1, 2], [3, 4]]))
    m.returns = np.array([F(3), F(5)], dtype=object)
    m.step(exact([[1, 2], [3, 4]]), np.array([1.0, 1.0]), np.array([False, True]))
    assert m.obs_rms.count == C0 and m.ret_rms.count == C0
    assert list(m.obs_rms.mean) == [0, 0] and list(m.obs_rms.var) == [1, 1]
    assert list(m.returns) == [3, 0]


def test_clipping():
    m = VecNormModel(2, 2, training=False, clip_obs=2.0, clip_reward=0.5)
    o, r, _ = m.step(np.array([[100.0, -100.0], [1.0, -1.0]]), np.array([10.0, -0.25]), np.zeros(2, bool))
    sd = np.sqrt(1 + 1e-8)
    assert o.tolist() == [[2.0, -2.0], [np.float32(1 / sd), np.float32(-1 / sd)]]
    assert r.tolist() == [0.5, -0.25 / sd]


def test_terminal_rows_stay_out_of_the_statistics_and_use_the_updated_ones():
    obs = np.array([[1.0], [2.0], [3.0]])
    term = np.array([[0.0], [1e6], [0.0]], dtype=np.float32)
    a = VecNormModel(3, 1)
    _, _, t = a.step(obs, np.zeros(3), np.array([False, True, False]), term)
    b = VecNormModel(3, 1)
    b.step(obs, np.zeros(3), np.zeros(3, bool))
    assert a.obs_rms.mean == b.obs_rms.mean and a.obs_rms.var == b.obs_rms.var
    assert t[1, 0] == np.float32(np.clip((1e6 - a.obs_rms.mean[0]) / np.sqrt(a.obs_rms.var[0] + 1e-8), -10, 10))
    assert t[0, 0] == 0 and t[2, 0] == 0  # rows of envs that did not finish are left as they were


def test_host_normalize_obs_matches_the_model():
    rng = np.random.default_rng(0)
    m = VecNormModel(16, 5)
    m.reset(rng.normal(3, 2, size=(16, 5)))
    x = rng.normal(3, 9, size=(7, 5)).astype(np.float32)
    rms = RunningStats(m.obs_rms.mean, m.obs_rms.var, m.obs_rms.count)
    assert np.array_equal(normalize_obs_np(x, rms, 10.0, 1e-8), m.normalize_obs(x))


def test_save_load_round_trip(tmp_path):
    s = NormSettings(training=False, norm_obs=True, norm_reward=False, clip_obs=5.0, clip_reward=3.0, gamma=0.9, epsilon=1e-6)
    st = NormState(RunningStats(np.array([1.5, -2.25, 1e4]), np.array([0.5, 3.0, 1e-2]), 123.0001),
                   RunningStats(np.float64(0.25), np.float64(7.5), 40.0001), np.arange(3.0))
    p = tmp_path / "vecnorm"
    save_state(p, s, st)
    assert os.path.exists(p)
    s2, st2 = load_state(p)
    assert s2 == s
    assert np.array_equal(st2.obs_rms.mean, st.obs_rms.mean) and np.array_equal(st2.obs_rms.var, st.obs_rms.var)
    assert st2.obs_rms.count == st.obs_rms.count
    assert (float(st2.ret_rms.mean), float(st2.ret_rms.var), st2.ret_rms.count) == (0.25, 7.5, 40.0001)
    assert st2.returns is None  # returns are not saved: zero after a load, as in SB3


def sb3_like(**over):
    vn = SimpleNamespace(obs_rms=SimpleNamespace(mean=np.array([1.0, 2.0]), var=np.array([4.0, 9.0]), count=10.0),
                         ret_rms=SimpleNamespace(mean=np.float64(0.5), var=np.float64(2.0), count=10.0), clip_obs=10.0,
                         clip_reward=10.0, gamma=0.99, epsilon=1e-8, training=False, norm_obs=True, norm_reward=True)
    for k, v in over.items():
        setattr(vn, k, v)
    return vn


def test_from_sb3_attributes():
    s, st = state_from_sb3(sb3_like())
    assert s == NormSettings(training=False)
    assert st.obs_rms.mean.tolist() == [1.0, 2.0] and st.obs_rms.var.tolist() == [4.0, 9.0] and st.obs_rms.count == 10.0
    assert (float(st.ret_rms.mean), float(st.ret_rms.var), st.ret_rms.count) == (0.5, 2.0, 10.0)


@pytest.mark.parametrize("over", [dict(clip_obs=0.0), dict(clip_reward=-1.0), dict(gamma=1.5), dict(epsilon=0.0),
                                  dict(obs_rms={"a": None}),
                                  dict(obs_rms=SimpleNamespace(mean=np.zeros(2), var=np.array([1.0, -1.0]), count=1.0)),
                                  dict(ret_rms=SimpleNamespace(mean=np.zeros(2), var=np.ones(2), count=1.0)),
                                  dict(obs_rms=SimpleNamespace(mean=np.zeros(2), var=np.ones(2), count=0.0))])
def test_from_sb3_rejects_bad_parameters(over):
    with pytest.raises(ValueError):
        state_from_sb3(sb3_like(**over))


def test_library_exports_the_normaliser():
    from fleetrl_amd import build

    lib = ctypes.CDLL(build.build())
    for sym in _capi.NORM_SYMBOLS:
        assert hasattr(lib, sym), sym


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){printf("%zu %zu %zu", '
                   'sizeof(FleetNormParams), offsetof(FleetNormParams, clip_obs), offsetof(FleetNormParams, epsilon));return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _capi.FleetNormParams
    assert got == [ctypes.sizeof(P), P.clip_obs.offset, P.epsilon.offset]


@pytest.mark.parametrize("over", [dict(clip_obs=0.0), dict(clip_reward=float("nan")), dict(gamma=-0.1), dict(gamma=1.01),
                                  dict(epsilon=0.0), dict(num_envs=0), dict(obs_dim=0), dict(struct_bytes=8)])
def test_create_rejects_bad_parameters(over):
    lib = _capi.load_library()
    kw = dict(struct_bytes=ctypes.sizeof(_capi.FleetNormParams), num_envs=4, obs_dim=3, training=1, norm_obs=1, norm_reward=1,
              clip_obs=10.0, clip_reward=10.0, gamma=0.99, epsilon=1e-8)
    kw.update(over)
    p = _capi.FleetNormParams(**kw)
    h = ctypes.c_void_p()
    assert lib.fleet_norm_create(0, ctypes.byref(p), ctypes.byref(h)) == _capi.ERR_INVALID
    assert h.value is None
    assert lib.fleet_norm_last_error(None)
