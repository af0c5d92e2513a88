"""Without a GPU: the pattern of tests/large_model.py is honest at the shapes and indices tests/test_large_arrays_gpu.py uses (a
read or write through an address cut to 30, 31 or 32 bits always meets another value), and the rollout and replay buffers refuse,
by name and before the device is touched, every size a 32-bit loop counter of their kernels could not finish."""
import ctypes as C
import os

import numpy as np
import pytest

import large_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the pattern --------------------------------------------------------------------------------------------------------------------
def test_the_modulus_is_an_odd_prime_below_2_24():
    assert lm.M == 16777213 and lm.M % 2 == 1
    assert all(lm.M % d for d in range(2, 4097))  # 4097^2 > 2^24


def test_values_are_exact_float32_in_the_unit_interval():
    i = np.concatenate([np.arange(0, 70000), lm.M + np.arange(-3, 4), (1 << 32) + np.arange(-3, 4), (1 << 33) + lm.M * 5 + np.arange(-3, 4),
                        np.random.default_rng(1).integers(0, 1 << 34, 100000)]).astype(np.int64)
    v = lm.value(i)
    assert v.dtype == np.float32 and not np.isnan(v).any() and v.min() >= 0 and v.max() < 1
    assert np.array_equal(v.astype(np.float64) * 2.0 ** 24, (i % lm.M).astype(np.float64))  # nothing was rounded
    assert lm.value(lm.M)[()] == 0 and lm.value(lm.M - 1)[()] == np.float32((lm.M - 1) * 2.0 ** -24) and lm.value(1)[()] == 2.0 ** -24


@pytest.mark.parametrize("start", [0, 5, lm.M - 7, lm.M, (1 << 32) - 100, (1 << 32) + 131072 - 8192, 4161 * 1048581])
def test_span_is_value_over_consecutive_indices(start):
    for n in (0, 1, 100, 8197, 1048581):
        want = lm.value(start + np.arange(n, dtype=np.int64))
        assert np.array_equal(lm.span(start, n).view(np.uint32), want.view(np.uint32))


def test_aliases_are_the_truncations_inside_the_array():
    i = (1 << 32) + (1 << 31) + (1 << 30) + 5
    assert lm.aliases(i, 1 << 33) == [5, (1 << 30) + 5, (1 << 31) + (1 << 30) + 5]
    assert lm.aliases(i, 1 << 30) == [5]
    assert lm.aliases((1 << 31) + 7, 1 << 33) == [7]  # cut to 30 and to 31 bits alike; 32 bits keep it
    assert lm.aliases((1 << 30) - 1, 1 << 33) == [] == lm.aliases(0, 1 << 33)
    assert lm.deltas((1 << 31) + 1) == [1 << 30, 1 << 31] and lm.deltas(1 << 30) == []
    assert lm.deltas((1 << 32) + 1) == [1 << 30, 1 << 31, 3 << 30, 1 << 32]


def _arrays():
    """(name, rows, width, the rows a GPU test gathers, the rows its `add` checks read back) of every array of the large tests that
    passes 2^32 elements."""
    out = []
    for case, s in lm.ROLLOUT.items():
        n = s["K"] * s["E"]
        rows, more = lm.rollout_rows(case), []
        for t in lm.rollout_add_rows(case):  # the written time row, its neighbours and its alias rows, as buffer rows
            around = [t - 1, t, t + 1] + lm.alias_rows(t, s["K"], s["E"] * s["D"])
            more += [x * s["E"] + e for x in around if 0 <= x < s["K"] for e in (0, s["E"] - 1)]
        out.append((f"rollout/{case}", n, s["D"], rows, more))
    for case, s in lm.REPLAY.items():
        rows = lm.replay_rows(case, s["R"]) + lm.replay_rows(case, lm.REPLAY_PARTIAL_POS)
        p = lm.REPLAY_ADD_POS
        around = [p - 1, p, p + 1] + lm.alias_rows(p, s["R"], s["E"] * s["D"])
        more = [x * s["E"] + e for x in around if 0 <= x < s["R"] for e in (0, s["E"] - 1)]
        out.append((f"replay/{case}", s["R"] * s["E"], s["D"], rows, more))
    out.append(("policy", lm.POLICY["E"], lm.POLICY["D"], lm.policy_rows(), []))
    return out


@pytest.mark.parametrize("name,n_rows,width,rows,more", _arrays(), ids=[a[0] for a in _arrays()])
def test_the_pattern_differs_at_every_alias_of_every_checked_index(name, n_rows, width, rows, more):
    """For EVERY index of the array: no distance a truncation can produce is a multiple of M, so value(i) != value(alias).  Then the
    same by evaluation, at the rows the GPU tests gather: every column of a row (the first and last 4096 and 4096 seeded ones where a
    row is longer than that), under the pattern offset of every array filled that way."""
    n = n_rows * width
    assert n > 1 << 32 and (n - (1 << 32)) // width >= 2  # the array passes 2^32 with two whole rows to spare
    assert lm.deltas(n) and all(d % lm.M for d in lm.deltas(n))
    assert max(rows) == n_rows - 1 and min(rows) == 0
    assert sum(r * width >= 1 << 32 for r in rows) >= 2 and any(r * width < 1 << 30 for r in rows)
    past = [r for r in rows if r * width >= 1 << 32]
    assert all(set(lm.alias_rows(r, n_rows, width)) <= set(rows) for r in past)  # what a cut address reads instead is checked too
    rng = np.random.default_rng(5)
    cols = np.arange(width) if width <= 12288 else np.unique(np.concatenate([np.arange(4096), width - 1 - np.arange(4096),
                                                                             rng.integers(0, width, 4096)]))
    checked = 0
    for r in rows + more:
        i = np.uint64(r * width) + cols.astype(np.uint64)
        for k in lm.TRUNCATIONS:
            j = i & np.uint64((1 << k) - 1)
            cut = j != i
            for off in (0, lm.OFFSETS["next_obs"]):
                assert (lm.value(i + np.uint64(off)) != lm.value(j + np.uint64(off)))[cut].all(), (name, r, k)
            checked += int(cut.sum())
            for a, b in zip(i[cut][:3].tolist(), j[cut][:3].tolist()):
                assert b in lm.aliases(a, n)
    assert checked > 0


def test_the_replay_draws_reach_behind_2_32():
    """`sample` is asked at the call counters large_model.replay_calls names: by the model of the draw, at least two of its 64
    transitions lie behind element 2^32 (and not all of them)."""
    import replay_model as rp

    for case, s in lm.REPLAY.items():
        calls = lm.replay_calls(case)
        assert set(calls) == {"full", "partial"}
        for name, upper in (("full", s["R"]), ("partial", lm.REPLAY_PARTIAL_POS)):
            rows, envs = rp.draw(lm.REPLAY_SEED, calls[name], lm.REPLAY_BATCH, upper, s["E"])
            past = (rows.astype(np.int64) * s["E"] + envs) * s["D"] >= 1 << 32
            assert 2 <= past.sum() < lm.REPLAY_BATCH
        assert lm.REPLAY_PARTIAL_POS * s["E"] * s["D"] > 1 << 32 and lm.REPLAY_ADD_POS + 1 < s["R"]


# ---- the limits ---------------------------------------------------------------------------------------------------------------------
def test_the_limits_follow_from_the_launch_shapes():
    assert lm.limits() == {"rollout_items": 4294443008, "replay_envs": 2147475456, "replay_dim": 2147483584}


def _rollout(E, K, D, A):
    from fleetrl_amd import _capi

    return _capi.FleetRolloutParams(C.sizeof(_capi.FleetRolloutParams), E, K, D, A, 0, 0.99, 0.95)


def _replay(size, E, D, A):
    from fleetrl_amd import _capi

    return _capi.FleetReplayParams(C.sizeof(_capi.FleetReplayParams), E, size, D, A, 0, 0)


def _accepted(family, p):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    layout = _capi.FleetRolloutLayout() if family == "rollout" else _capi.FleetReplayLayout()
    rc = getattr(lib, f"fleet_{family}_layout")(C.byref(p), C.byref(layout))
    assert rc == _capi.OK, getattr(lib, f"fleet_{family}_last_error")(None).decode()
    return layout


def _refused(family, p, *words):
    """Layout and create both refuse, create before it touches the device (this passes on a machine without one), and the message
    holds every word."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    layout = _capi.FleetRolloutLayout() if family == "rollout" else _capi.FleetReplayLayout()
    assert getattr(lib, f"fleet_{family}_layout")(C.byref(p), C.byref(layout)) == _capi.ERR_INVALID
    why = getattr(lib, f"fleet_{family}_last_error")(None).decode()
    h = C.c_void_p(0xdead)
    assert getattr(lib, f"fleet_{family}_create")(0, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and h.value is None
    assert getattr(lib, f"fleet_{family}_last_error")(None).decode() == why
    for w in words:
        assert str(w) in why, (w, why)


def test_rollout_refuses_a_time_row_its_copy_loop_cannot_finish():
    """copy_flat counts a time row's items in an unsigned that advances by up to kRolloutMaxBlocks * kRolloutThreads: the largest row
    accepted is 2^32 minus that stride, in obs_dim and in act_dim alike."""
    L = lm.limits()["rollout_items"]
    assert L == (1 << 19) * 8191 and L + 1 == 54507 * 78787
    assert _accepted("rollout", _rollout(1 << 19, 1, 8191, 1)).row_bytes[0] == 4 * L
    assert _accepted("rollout", _rollout(1 << 19, 1, 1, 8191)).row_bytes[1] == 4 * L
    for D, A in ((78787, 1), (1, 78787)):
        _refused("rollout", _rollout(54507, 1, D, A), "num_envs * obs_dim", "num_envs * act_dim", L, "<=")
    _refused("rollout", _rollout(1 << 19, 1, 8192, 1), L)        # 2^32: what the parent refused first
    _refused("rollout", _rollout(1 << 16, 1, (1 << 16) - 1, 1), L)  # inside the window the parent accepted


def test_rollout_refuses_more_rows_than_an_int32_index_names():
    """E * K < 2^31: flat gather indices are int32."""
    assert _accepted("rollout", _rollout((1 << 31) - 1, 1, 1, 1)).bytes[2] == 4 * ((1 << 31) - 1)
    assert _accepted("rollout", _rollout(1, (1 << 31) - 1, 1, 1)).bytes[3] == (1 << 31) - 1
    for E, K in ((1 << 16, 1 << 15), (1 << 30, 2), (2, 1 << 30), ((1 << 31) - 1, (1 << 31) - 1)):
        _refused("rollout", _rollout(E, K, 1, 1), "num_envs * n_steps", "< 2^31")


def test_replay_refuses_an_env_count_its_row_loop_cannot_finish():
    """replay_add walks the env rows with an int that advances by up to FLEET_REPLAY_MAX_BLOCKS * kReplayWaves."""
    L = lm.limits()["replay_envs"]
    for size in (1, L, (1 << 31) - 1):
        assert _accepted("replay", _replay(size, L, 1, 1)).rows == 1
    for E in (L + 1, (1 << 31) - 1):
        _refused("replay", _replay(1, E, 1, 1), "num_envs", "<=", L)
        _refused("replay", _replay((1 << 31) - 1, E, 1, 1), "num_envs", L)


def test_replay_refuses_a_row_its_lane_loop_cannot_finish():
    """copy_row and sample_row walk a row's words with an int that advances by 64."""
    L = lm.limits()["replay_dim"]
    assert _accepted("replay", _replay(1, 1, L, 1)).bytes[0] == 4 * L == _accepted("replay", _replay(1, 1, 1, L)).bytes[2]
    assert _accepted("replay", _replay(3, 1, L, L)).rows == 3
    for D, A, name in ((L + 1, 1, "obs_dim"), ((1 << 31) - 1, 1, "obs_dim"), (1, L + 1, "act_dim"), (1, (1 << 31) - 1, "act_dim")):
        _refused("replay", _replay(1, 1, D, A), name, "<=", L)


def test_replay_rows_times_envs_stays_an_int32():
    """R * E <= max(buffer_size, E) < 2^31 for int32 parameters, so the header's R * E < 2^31 refusal cannot be reached from outside:
    the largest ring an int32 names is accepted."""
    assert _accepted("replay", _replay((1 << 31) - 1, 1, 1, 1)).rows == (1 << 31) - 1
    assert _accepted("replay", _replay((1 << 31) - 1, 3, 1, 1)).rows == ((1 << 31) - 1) // 3


def test_the_header_states_the_limits():
    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    for words in ("E * max(D, A) <= 2^32 - 2048 * 256", "E <= 2^31 - 2048 * 4", "D, A <= 2^31 - 64", "batch * D (batch * A) <= 2^32 - 2048 * 256"):
        assert words in hdr, words
