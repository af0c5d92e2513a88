"""The replay buffer without a GPU: the C ABI's declarations and bindings, fleet_replay_layout, the parameter checks of
fleet_replay_create (made before the device is touched), and the NumPy model of tests/replay_model.py pinned by known answers:
Philox4x32-10 against the published vectors and the oracle's start-row sampler, the index draw's range and uniformity, the ring."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import replay_model as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("fleet_replay_layout", "fleet_replay_create", "fleet_replay_destroy", "fleet_replay_last_error", "fleet_replay_set_stream",
           "fleet_replay_arrays", "fleet_replay_add_dev", "fleet_replay_gather_dev", "fleet_replay_sample_dev",
           "fleet_replay_check_errors", "fleet_replay_size", "fleet_replay_set_position")


def test_header_declares_the_entries_under_abi_11_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_replay_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.REPLAY_SYMBOLS)
    section = hdr[hdr.index("replay buffer on the device"):]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    for struct in ("FleetReplayParams", "FleetReplayLayout", "FleetReplayArrays"):
        assert f"}} {struct};" in section
    assert "typedef struct FleetReplay* fleet_replay_handle;" in section
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert fn.restype is (C.c_char_p if name == "fleet_replay_last_error" else C.c_int), name
    assert set(ENTRIES) <= set(_capi.EXPORTED_SYMBOLS)


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    import subprocess

    from fleetrl_amd import _capi

    P, L, A = _capi.FleetReplayParams, _capi.FleetReplayLayout, _capi.FleetReplayArrays
    fields = [("FleetReplayParams", P, [n for n, _ in P._fields_]), ("FleetReplayLayout", L, [n for n, _ in L._fields_]),
              ("FleetReplayArrays", A, [n for n, _ in A._fields_])]
    exprs, want = [], []
    for cname, cls, names in fields:
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(cls))
        for n in names:
            exprs.append(f"offsetof({cname}, {n})")
            want.append(getattr(cls, n).offset)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert [n for n, _ in P._fields_] == ["struct_bytes", "num_envs", "buffer_size", "obs_dim", "act_dim", "reserved", "seed"]


# (buffer_size, E, D, A): a tiny one, buffer_size < E (R = 1), a ragged one, the full size, and one whose observation arrays are
# 2^30 * 5 * 4 bytes > 2^32 each
@pytest.mark.parametrize("size,E,D,A", [(1, 1, 1, 1), (5, 8, 7, 3), (1000, 7, 37, 5), (1_000_000, 4096, 388, 50),
                                        (1 << 30, 1 << 10, 5, 1)])
def test_layout_gives_the_models_sizes_and_aligned_offsets(size, E, D, A):
    from fleetrl_amd import _capi

    L = _capi.replay_layout(size, E, D, A)
    want = rp.layout(size, E, D, A)
    R = max(size // E, 1)
    assert L.struct_bytes == C.sizeof(_capi.FleetReplayLayout) and L.alignment == 256 == _capi.REPLAY_ALIGN
    assert L.rows == R == want["rows"]
    assert _capi.REPLAY_ARRAY_NAMES == rp.ARRAYS
    end = 0
    per_env = {"observations": D * 4, "next_observations": D * 4, "actions": A * 4, "rewards": 4, "dones": 1, "timeouts": 1}
    for i, n in enumerate(rp.ARRAYS):
        assert (L.offset[i], L.bytes[i], L.row_bytes[i]) == (want[n]["offset"], want[n]["bytes"], want[n]["row_bytes"]), n
        assert L.offset[i] % 256 == 0 and L.offset[i] >= end and L.bytes[i] == R * L.row_bytes[i]  # aligned, no overlap
        assert L.bytes[i] == R * E * per_env[n]
        end = L.offset[i] + L.bytes[i]
    assert L.error_offset == want["error_offset"] >= end and L.error_offset % 256 == 0
    assert L.total_bytes == want["total_bytes"] >= L.error_offset + 4
    if size == 1 << 30:
        assert L.bytes[0] > 1 << 32 and L.offset[2] > 1 << 33


def _params(**over):
    from fleetrl_amd import _capi

    kw = dict(struct_bytes=C.sizeof(_capi.FleetReplayParams), num_envs=8, buffer_size=64, obs_dim=5, act_dim=2, reserved=0, seed=1)
    kw.update(over)
    return _capi.FleetReplayParams(**kw)


@pytest.mark.parametrize("bad", [dict(num_envs=0), dict(num_envs=-3), dict(buffer_size=0), dict(buffer_size=-1), dict(obs_dim=0),
                                 dict(act_dim=0), dict(act_dim=-1), dict(struct_bytes=0), dict(struct_bytes=28)])
def test_create_refuses_bad_parameters_before_it_touches_the_device(bad):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    h = C.c_void_p(0xdead)
    assert lib.fleet_replay_create(0, C.byref(_params(**bad)), C.byref(h)) == _capi.ERR_INVALID
    assert h.value is None
    why = lib.fleet_replay_last_error(None).decode()
    key = next(iter(bad))
    assert key in why, why
    assert lib.fleet_replay_layout(C.byref(_params(**bad)), C.byref(_capi.FleetReplayLayout())) == _capi.ERR_INVALID
    assert lib.fleet_replay_create(0, None, C.byref(h)) == _capi.ERR_INVALID
    assert "null" in lib.fleet_replay_last_error(None).decode()
    assert lib.fleet_replay_create(0, C.byref(_params()), None) == _capi.ERR_INVALID
    assert lib.fleet_replay_layout(C.byref(_params()), None) == _capi.ERR_INVALID


def test_the_largest_buffer_an_int32_can_name_is_accepted_by_layout():
    """R * E <= max(buffer_size, E) < 2^31 for int32 parameters: the R * E < 2^31 rule of the header holds for every input."""
    from fleetrl_amd import _capi

    L = _capi.replay_layout(2 ** 31 - 1, 1, 1, 1)
    assert L.rows == 2 ** 31 - 1 and L.bytes[0] == 4 * (2 ** 31 - 1)
    most = 2 ** 31 - 2048 * 4  # the most envs replay_add's row loop finishes (tests/test_large_arrays_cpu.py)
    assert _capi.replay_layout(2 ** 31 - 1, most, 1, 1).rows == 1 == _capi.replay_layout(5, most, 1, 1).rows


def test_python_class_raises_invalid_for_bad_parameters():
    from fleetrl_amd import DeviceReplayBuffer, FleetHipError, _capi

    with pytest.raises(FleetHipError) as ei:
        DeviceReplayBuffer(64, 8, 0, 2)
    assert ei.value.status == _capi.ERR_INVALID and "obs_dim" in str(ei.value)
    with pytest.raises(ValueError):
        DeviceReplayBuffer(2 ** 40, 8, 5, 2)


# ---- Philox4x32-10 and the index draw ----------------------------------------------------------------------------------------------
def test_philox_reproduces_the_published_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds (counter, key -> block)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        assert rp.philox4x32_10(counter, key) == want
    # the vectorised form the draw uses is the same function
    x = rp._philox_vec(np.array([0, 5, 0xffffffff]), 7, 9, (3 << 32) | 11)
    for i, c0 in enumerate((0, 5, 0xffffffff)):
        assert tuple(int(v[i]) for v in x) == rp.philox4x32_10((c0, 0, 7, 9), (11, 3))


def test_philox_agrees_with_the_oracles_start_row_sampler():
    """oracle_philox_start(seed, env, episode) is word 0 of the block of counter (env, episode, 0, 0): as far as it exposes it."""
    from oracle import fleet_oracle

    lib = fleet_oracle.load()
    rng = np.random.default_rng(5)
    for _ in range(200):
        seed, env, ep = int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))
        assert lib.oracle_philox_start(seed, env, ep) == rp.philox4x32_10((env, ep, 0, 0), (seed & rp.M32, seed >> 32))[0]
    assert lib.oracle_philox_start(0, 0, 0) == 0x6627e8d5


@pytest.mark.parametrize("n", [1, 2, 3, 244, 4096, 2 ** 31 - 1])
def test_the_draw_never_returns_n(n):
    ones = 2 ** 64 - 1
    assert rp.mulhi64(ones, n) == n - 1 and rp.mulhi64(0, n) == 0
    m = np.uint64(rp.M32)
    assert int(rp._mulhi64_vec(np.array([m]), np.array([m]), n)[0]) == n - 1
    assert int(rp._mulhi64_vec(np.array([np.uint64(0)]), np.array([np.uint64(0)]), n)[0]) == 0


def _chi2_quantile(df, z):
    """Wilson-Hilferty: the chi-square quantile at the standard normal deviate z."""
    return df * (1 - 2 / (9 * df) + z * np.sqrt(2 / (9 * df))) ** 3


def test_the_draw_is_uniform_over_rows_and_envs():
    """2^20 draws at a fixed seed over 244 rows x 4096 envs.  Threshold: the chi-square quantile at z = 4.75 (one-sided p about
    1e-6 for a uniform source), 362.6 for 243 degrees of freedom and 4539 for 4095; a draw with the multiply-high's bias (n / 2^64)
    sits near the mean, df.  The model's own statistics at this seed are 262.1 and 4118.2 (printed below): within one standard
    deviation, sqrt(2 df), of the mean."""
    B, R, E = 1 << 20, 244, 4096
    rows, envs = rp.draw(2024, 3, B, R, E)
    assert rows.min() >= 0 and rows.max() < R and envs.min() >= 0 and envs.max() < E
    for vals, n in ((rows, R), (envs, E)):
        cnt = np.bincount(vals, minlength=n).astype(np.float64)
        chi2 = float(((cnt - B / n) ** 2 / (B / n)).sum())
        limit = _chi2_quantile(n - 1, 4.75)
        print(f"chi-square over {n}: {chi2:.1f} (df {n - 1}, limit {limit:.1f})")
        assert chi2 < limit
    assert abs(_chi2_quantile(243, 4.75) - 362.6) < 0.5 and abs(_chi2_quantile(4095, 4.75) - 4539) < 2


def test_draw_depends_on_seed_call_and_sample_only():
    a = rp.draw(7, 0, 1000, 244, 4096)
    assert all(np.array_equal(x, y) for x, y in zip(a, rp.draw(7, 0, 1000, 244, 4096)))
    assert not np.array_equal(a[0], rp.draw(7, 1, 1000, 244, 4096)[0]) and not np.array_equal(a[0], rp.draw(8, 0, 1000, 244, 4096)[0])
    assert all(np.array_equal(x[:256], y) for x, y in zip(a, rp.draw(7, 0, 256, 244, 4096)))  # sample b does not depend on B
    for b in (0, 1, 999):
        assert (a[0][b], a[1][b]) == rp.draw_one(7, 0, b, 244, 4096)
    big = rp.draw(2 ** 64 - 1, 2 ** 40 + 1, 64, 2 ** 31 - 1, 1)  # both halves of the call counter and of the seed are used
    assert (big[0][5], big[1][5]) == rp.draw_one(2 ** 64 - 1, 2 ** 40 + 1, 5, 2 ** 31 - 1, 1)
    assert not np.array_equal(big[0], rp.draw(2 ** 64 - 1, 1, 64, 2 ** 31 - 1, 1)[0])


# ---- the ring ----------------------------------------------------------------------------------------------------------------------
def test_model_known_answers_on_a_hand_sized_buffer():
    """buffer_size 7, E = 2 -> R = 3 rows; five adds wrap once.  Step k stores obs k, next k + 0.5, terminal 100 + k."""
    m = rp.ReplayModel(7, 2, 1, 1)
    assert m.R == 3 and m.upper() == 0

    def step(k, done, timeout=None):
        f = np.float32
        m.add(np.full((2, 1), k, f), np.full((2, 1), k + 0.5, f), np.full((2, 1), -k, f), np.array([k + 2.0 ** -30, 0.1 * k]),
              np.array(done, np.uint8), np.full((2, 1), 100 + k, f), None if timeout is None else np.array(timeout, np.uint8))

    step(1, [0, 0])
    step(2, [0, 1])
    assert (m.pos, m.full, m.upper()) == (2, False, 2)
    assert m.observations[:2, :, 0].tolist() == [[1, 1], [2, 2]]
    assert m.next_observations[:2, :, 0].tolist() == [[1.5, 1.5], [2.5, 102]]  # the terminal row of the done env only
    assert m.rewards[1].tolist() == [2.0, float(np.float32(0.2))] and m.dones[:2].tolist() == [[0, 0], [0, 1]]
    step(3, [5, 0], timeout=[1, 0])  # any non-zero byte is a done; it was a time limit
    assert (m.pos, m.full, m.upper()) == (0, True, 3)
    step(4, [0, 0])
    step(5, [1, 1], timeout=[0, 1])
    assert (m.pos, m.full) == (2, True)
    assert m.observations[:, 0, 0].tolist() == [4, 5, 3] and m.next_observations[:, :, 0].tolist() == [[4.5, 4.5], [105, 105], [103, 3.5]]
    assert m.actions[:, 1, 0].tolist() == [-4, -5, -3]
    assert m.dones.tolist() == [[0, 0], [1, 1], [1, 0]] and m.timeouts.tolist() == [[0, 0], [0, 1], [1, 0]]
    o, a, n, d, r = m.get_samples([1, 1, 2, 0, 2], [0, 1, 0, 1, 0])
    assert o[:, 0].tolist() == [5, 5, 3, 4, 3] and n[:, 0].tolist() == [105, 105, 103, 4.5, 103] and a[:, 0].tolist() == [-5, -5, -3, -4, -3]
    assert d.shape == r.shape == (5, 1) and d[:, 0].tolist() == [1, 0, 0, 0, 0]  # done * (1 - timeout)
    assert r[:, 0].tolist() == [5.0, 0.5, 3.0, float(np.float32(0.4)), 3.0]
    # normalised at sample time: mean 1, var 3.99999999 + eps 1e-8 -> sd 2; clip 1.5; reward / sqrt(0.25) clipped at 9
    stats = dict(obs_mean=np.array([1.0]), obs_var=np.array([4.0 - 1e-8]), ret_var=0.25 - 1e-8, norm_obs=True, norm_reward=True,
                 clip_obs=1.5, clip_reward=9.0, epsilon=1e-8)
    o, a, n, d, r = m.get_samples([1, 2, 0], [0, 0, 1], stats)
    assert o[:, 0].tolist() == [1.5, 1.0, 1.5] and n[:, 0].tolist() == [1.5, 1.5, 1.5] and a[:, 0].tolist() == [-5, -3, -4]
    assert r[:, 0].tolist() == [9.0, 6.0, float(np.float32(np.float64(np.float32(0.4)) / 0.5))]
    o2, _, _, _, r2 = m.get_samples([1, 2, 0], [0, 0, 1], dict(stats, norm_obs=False))
    assert o2[:, 0].tolist() == [5, 3, 4] and np.array_equal(r2, r)
    (o3, *_), rows, envs = m.sample(4)
    assert m.calls == 1 and rows.max() < 3 and envs.max() < 2 and np.array_equal(o3, m.observations[rows, envs])


def test_model_buffer_smaller_than_the_env_count_keeps_one_row():
    m = rp.ReplayModel(3, 8, 2, 1)
    assert m.R == 1
    z = np.zeros((8, 2), np.float32)
    m.add(z + 1, z, np.zeros((8, 1), np.float32), np.zeros(8), np.zeros(8, np.uint8))
    assert (m.pos, m.full, m.upper()) == (0, True, 1)
    m.add(z + 2, z, np.zeros((8, 1), np.float32), np.zeros(8), np.zeros(8, np.uint8))
    assert m.observations[0, 0, 0] == 2
