"""Rollout collection without a GPU: the C ABI's section, its position, bindings and struct layouts against a compiled probe, every
refusal that needs no device, the ring's slot rule against collections.deque, and the NumPy restatement of the closing launch
(tests/collect_model.py) against math.fsum."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import collect_model as cm

ROOT = cm.ROOT
ENTRIES = ("fleet_collect_create", "fleet_collect_destroy", "fleet_collect_last_error", "fleet_collect_describe", "fleet_collect_reset_dev",
           "fleet_collect_ppo_dev", "fleet_collect_offpolicy_dev", "fleet_collect_episodes_dev", "fleet_collect_finish_dev",
           "fleet_collect_episodes_read")
PARAM_FIELDS = ["struct_bytes", "stats_window"]
PPO_FIELDS = ["struct_bytes", "n_steps", "env_id_offset", "reserved", "buffer", "log_std", "seed", "first_step", "stats"]
OFF_FIELDS = ["struct_bytes", "n_steps", "env_id_offset", "reserved", "learning_starts", "replay", "sigma", "shift", "noise_lo", "noise_hi",
              "noise", "seed", "first_step", "stats"]
INFO_FIELDS = ["num_envs", "obs_dim", "act_dim", "stats_window", "has_norm", "cur", "launches", "reserved", "block_bytes", "carry_obs",
               "raw_obs", "carry_start", "raw_terminal", "raw_reward", "reward", "env_actions", "last_values", "ring_return", "ring_length",
               "ring_count"]
TITLE = "collect_rollouts on the device"
NOISE_TITLE = "correlated action noise on the device"
TARGETS_TITLE = "TD3 / DDPG learning targets on the device"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_lies_between_the_noise_and_the_targets_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_collect_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.COLLECT_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    assert all(name.startswith("fleet_collect_") for name in _capi.COLLECT_SYMBOLS)
    assert hdr.count("---- " + TITLE) == 1
    titles = re.findall(r"^/\* ---- (.*?) \(", hdr, flags=re.M)
    assert titles.count(TITLE) == 1 and not any(t in TITLE or TITLE in t for t in titles if t != TITLE)
    at = titles.index(TITLE)
    assert titles[at - 1] == NOISE_TITLE and titles[at + 1] == TARGETS_TITLE
    assert titles[-1] == "PPO minibatch gradients on the device"  # (the last section stays the last)
    assert hdr.index("int fleet_noise_describe(") < hdr.index("---- " + TITLE) < hdr.index("---- " + TARGETS_TITLE)
    section = hdr[hdr.index("---- " + TITLE):hdr.index("---- " + TARGETS_TITLE)]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    for later in titles[at + 1:]:  # the tests of the later sections find them with hdr.index(title)
        assert later not in section, later
    for said in ("} FleetCollectParams;", "} FleetCollectPpoArgs;", "} FleetCollectOffpolicyArgs;", "} FleetCollectInfo;",
                 "#define FLEET_COLLECT_MAX_WINDOW 4096", "#define FLEET_COLLECT_STATS 16", "(count + k) % W iff c - k <= W", "count += c",
                 "must outlive", "5 K + 3 launches with a normaliser, 4 K + 3 without", "PING-PONG", "NaN when n == 0", "ONE stream",
                 "deque(maxlen = W)", "no atomics", "first_step + steps", "Out of scope", "gSDE", "before the first launch"):
        assert said in section, said
    assert not re.search(r"^(?:int|const char\*)\s+fleet_(?!collect_)", section, flags=re.M)  # no entry of a neighbour in it
    assert len(re.findall(r"^/\* ---- ", section, flags=re.M)) == 0
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_collect_create.argtypes) == 5 and len(lib.fleet_collect_ppo_dev.argtypes) == 2
    assert len(lib.fleet_collect_offpolicy_dev.argtypes) == 2 and len(lib.fleet_collect_episodes_dev.argtypes) == 5
    assert len(lib.fleet_collect_finish_dev.argtypes) == 4 and len(lib.fleet_collect_episodes_read.argtypes) == 4


def test_the_family_is_built_exported_and_restated_with_the_headers_constants():
    import fleetrl_amd
    from fleetrl_amd import _capi, build, collect

    assert "fleet_collect.hip" in build.SOURCES and "fleet_collect.h" in build.HEADERS
    assert fleetrl_amd.DevicePPOCollect is collect.DevicePPOCollect and fleetrl_amd.DeviceTD3Collect is collect.DeviceTD3Collect
    assert collect.DevicePPOCollect._prefix == collect.DeviceTD3Collect._prefix == "collect"
    assert collect.STATS == cm.STATS and len(collect.SB3_NAMES) == len(collect.STATS)
    assert collect.SB3_NAMES[:2] == ("rollout/ep_rew_mean", "rollout/ep_len_mean")
    assert (_capi.COLLECT_MAX_WINDOW, _capi.COLLECT_STATS) == (cm.MAX_WINDOW, cm.STATS_LEN) == (4096, 16)
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_collect.h")).read()
    for name, want in (("kCollectScanThreads", cm.SCAN_THREADS), ("kCollectThreads", cm.LANES), ("kCollectMaxWindow", cm.MAX_WINDOW),
                       ("kCollectStats", cm.STATS_LEN)):
        assert re.search(rf"constexpr int {name} = (\d+);", src).group(1) == str(want), name
    kernels = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_collect.hip")).read()
    assert "atomic" not in kernels.split("// ---- host")[0].replace("No atomics", "")  # the kernels use none


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetCollectParams", _capi.FleetCollectParams, PARAM_FIELDS),
                               ("FleetCollectPpoArgs", _capi.FleetCollectPpoArgs, PPO_FIELDS),
                               ("FleetCollectOffpolicyArgs", _capi.FleetCollectOffpolicyArgs, OFF_FIELDS),
                               ("FleetCollectInfo", _capi.FleetCollectInfo, INFO_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["FLEET_COLLECT_MAX_WINDOW", "FLEET_COLLECT_STATS"]
    want += [_capi.COLLECT_MAX_WINDOW, _capi.COLLECT_STATS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert (C.sizeof(_capi.FleetCollectParams), C.sizeof(_capi.FleetCollectPpoArgs), C.sizeof(_capi.FleetCollectOffpolicyArgs),
            C.sizeof(_capi.FleetCollectInfo)) == (8, 56, 88, 152)


# ---- refusals that need no device --------------------------------------------------------------------------------------------------
def _ppo(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetCollectPpoArgs()
    a.struct_bytes, a.n_steps, a.env_id_offset, a.buffer, a.log_std, a.seed, a.first_step, a.stats = C.sizeof(a), 8, 0, 4096, 2048, 1, 0, 8192
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _off(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetCollectOffpolicyArgs()
    a.struct_bytes, a.n_steps, a.env_id_offset, a.learning_starts, a.replay, a.sigma = C.sizeof(a), 8, 0, 4, 4096, 2048
    a.noise_lo, a.noise_hi, a.seed, a.first_step, a.stats = -1.0, 1.0, 1, 0, 8192
    for k, v in kw.items():
        setattr(a, k, v)
    return a


NAN = float("nan")
PPO_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=48), "FleetCollectPpoArgs.struct_bytes does not match this library"),
    "n_steps-zero": (dict(n_steps=0), "n_steps must be >= 1, got 0"),
    "n_steps-negative": (dict(n_steps=-3), "n_steps must be >= 1, got -3"),
    "reserved": (dict(reserved=1), "reserved must be 0"),
    "env_id_offset": (dict(env_id_offset=-1), "env_id_offset must be >= 0, got -1"),
    "buffer-null": (dict(buffer=None), "null rollout handle"),
    "log_std-null": (dict(log_std=None), "null scale (log_std or sigma)"),
    "stats-null": (dict(stats=None), "null stats"),
}
OFF_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=80), "FleetCollectOffpolicyArgs.struct_bytes does not match this library"),
    "n_steps-zero": (dict(n_steps=0), "n_steps must be >= 1, got 0"),
    "reserved": (dict(reserved=2), "reserved must be 0"),
    "env_id_offset": (dict(env_id_offset=-7), "env_id_offset must be >= 0, got -7"),
    "replay-null": (dict(replay=None), "null replay handle"),
    "sigma-null": (dict(sigma=None), "null scale (log_std or sigma)"),
    "bounds-crossed": (dict(noise_lo=1.0, noise_hi=-1.0), "the bounds need noise_lo <= noise_hi"),
    "bounds-nan": (dict(noise_hi=NAN), "the bounds need noise_lo <= noise_hi"),
    "stats-null": (dict(stats=None), "null stats"),
}


@pytest.mark.parametrize("case", sorted(PPO_REFUSALS))
def test_the_ppo_call_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_collect_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = PPO_REFUSALS[case]
    rc = lib.fleet_collect_ppo_dev(None, C.byref(_ppo(**fields)))
    why = lib.fleet_collect_last_error(None).decode()
    assert rc == _capi.ERR_INVALID and why.startswith("fleet_collect_ppo_dev: ") and word in why, why


@pytest.mark.parametrize("case", sorted(OFF_REFUSALS))
def test_the_offpolicy_call_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = OFF_REFUSALS[case]
    rc = lib.fleet_collect_offpolicy_dev(None, C.byref(_off(**fields)))
    why = lib.fleet_collect_last_error(None).decode()
    assert rc == _capi.ERR_INVALID and why.startswith("fleet_collect_offpolicy_dev: ") and word in why, why


def test_good_arguments_name_the_null_handle_and_null_structs_are_refused():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_collect_last_error(None).decode()  # noqa: E731
    assert lib.fleet_collect_ppo_dev(None, None) == _capi.ERR_INVALID and last() == "fleet_collect_ppo_dev: null FleetCollectPpoArgs"
    assert lib.fleet_collect_offpolicy_dev(None, None) == _capi.ERR_INVALID and last() == "fleet_collect_offpolicy_dev: null FleetCollectOffpolicyArgs"
    for ok in (_ppo(), _ppo(n_steps=2 ** 31 - 1, seed=2 ** 64 - 1, first_step=2 ** 63, env_id_offset=2 ** 31 - 1)):
        assert lib.fleet_collect_ppo_dev(None, C.byref(ok)) == _capi.ERR_INVALID and last() == "fleet_collect_ppo_dev: null handle"
    for ok in (_off(), _off(noise=None, shift=None), _off(noise_lo=0.5, noise_hi=0.5), _off(learning_starts=2 ** 64 - 1, shift=512, noise=1024)):
        assert lib.fleet_collect_offpolicy_dev(None, C.byref(ok)) == _capi.ERR_INVALID and last() == "fleet_collect_offpolicy_dev: null handle"
    assert lib.fleet_collect_reset_dev(None, 0) == _capi.ERR_INVALID and last() == "fleet_collect_reset_dev: null handle"
    fn = lib.fleet_collect_episodes_dev
    for args, word in (((256, 512, 1024, 0), "E must be >= 1, got 0"), ((None, 512, 1024, 4), "null done"), ((256, None, 1024, 4), "null ep_return"),
                       ((256, 512, None, 4), "null ep_len"), ((256, 512, 1024, 4), "null handle")):
        assert fn(None, *args) == _capi.ERR_INVALID and last() == "fleet_collect_episodes_dev: " + word
    fn = lib.fleet_collect_finish_dev
    for args, word in (((0, -1, 256), "steps must be >= 0, got -1"), ((0, 4, None), "null stats"), ((0, 4, 256), "null handle")):
        assert fn(None, *args) == _capi.ERR_INVALID and last() == "fleet_collect_finish_dev: " + word
    assert lib.fleet_collect_episodes_read(None, None, None, None) == _capi.ERR_INVALID and last() == "fleet_collect_episodes_read: null handle"


def test_create_and_describe_refuse_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_collect_last_error(None).decode()  # noqa: E731
    h = C.c_void_p()
    fake = C.c_void_p(4096)  # (never dereferenced: a refusal in front of it is met first)
    good = _capi.FleetCollectParams(C.sizeof(_capi.FleetCollectParams), 100)
    create = lib.fleet_collect_create
    assert create(None, None, fake, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h and last() == "fleet_collect_create: null env handle"
    assert create(fake, None, None, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h and last() == "fleet_collect_create: null policy handle"
    assert create(fake, None, fake, C.byref(good), None) == _capi.ERR_INVALID and last() == "fleet_collect_create: null output handle"
    assert create(fake, None, fake, None, C.byref(h)) == _capi.ERR_INVALID and last() == "fleet_collect_create: null FleetCollectParams"
    for p, word in ((_capi.FleetCollectParams(4, 100), "FleetCollectParams.struct_bytes does not match this library"),
                    (_capi.FleetCollectParams(8, 0), "stats_window must be in 1..4096, got 0"),
                    (_capi.FleetCollectParams(8, -5), "stats_window must be in 1..4096, got -5"),
                    (_capi.FleetCollectParams(8, 4097), "stats_window must be in 1..4096, got 4097")):
        assert create(fake, None, fake, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
        assert last() == "fleet_collect_create: " + word
    assert lib.fleet_collect_destroy(None) == _capi.OK
    assert lib.fleet_collect_describe(None, None) == _capi.ERR_INVALID


# ---- the ring ------------------------------------------------------------------------------------------------------------------------
def _drive(E, W, patterns, seed):
    """The slot rule's ring beside SB3's deque over a sequence of done patterns; the windows must agree after every step."""
    rng = np.random.default_rng(seed)
    ring, sb3 = cm.Ring(W), cm.Sb3Buffer(W)
    for step, done in enumerate(patterns):
        ret, length = rng.standard_normal(E) * 100, rng.integers(1, 500, E).astype(np.int32)
        ring.step(done, ret, length)
        sb3.step(done, ret, length)
        got, want = ring.window(), sb3.window()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (E, W, step)
    assert ring.count == sum(int(np.count_nonzero(d)) for d in patterns)
    return ring


@pytest.mark.parametrize("E,W", [(1, 1), (3, 7), (5, 1), (64, 7), (65, 100), (130, 100), (1025, 100), (300, 4096)])
def test_the_slot_rule_is_a_deque_of_maxlen_w(E, W):
    rng = np.random.default_rng(E * 10007 + W)
    none, every = np.zeros(E, bool), np.ones(E, bool)
    exactly_w = np.zeros(E, bool)
    exactly_w[rng.permutation(E)[:min(W, E)]] = True  # c = W where E allows it
    one = np.zeros(E, bool)
    one[E // 2] = True
    patterns = [none, one, every, exactly_w, none, every, every, one]  # c = 0, 1, E (> W where E > W), W; the ring wraps several times
    patterns += [rng.random(E) < p for p in (0.02, 0.5, 0.9, 0.1, 0.3) for _ in range(3)]
    ring = _drive(E, W, patterns, seed=E + W)
    assert ring.count > W or E * len(patterns) <= W or W == 4096


def test_no_two_kept_episodes_of_a_step_share_a_slot_and_only_the_last_w_are_kept():
    for count in (0, 5, 99, 2 ** 40 + 3):
        for W in (1, 7, 100):
            for c in (0, 1, W - 1, W, W + 1, 3 * W + 2):
                kept = [(k, cm.slot_rule(count, c, k, W)[1]) for k in range(c) if cm.slot_rule(count, c, k, W)[0]]
                assert [k for k, _ in kept] == list(range(max(c - W, 0), c))
                assert len({s for _, s in kept}) == len(kept) and all(0 <= s < W for _, s in kept)


# ---- the closing launch's model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 100, 255, 256, 257, 1000, 4096])
def test_the_ordered_sum_stays_within_the_bound_of_an_ordered_float64_sum(n):
    """|S - fsum| <= (n - 1) 2^-53 sum|x|: the bound of an ordered float64 sum -- n - 1 additions, each rounding a partial sum of at
    most sum|x| in magnitude by at most 2^-53 of it.  Derived, not measured (S's own chains are n / 256 + 8 additions deep at most)."""
    rng = np.random.default_rng(n)
    for scale in (1.0, 1e6, 1e-3):
        x = rng.standard_normal(n) * scale
        ring = cm.Ring(n)
        ring.step(np.ones(n, bool), x, rng.integers(1, 10 ** 6, n).astype(np.int32))
        got = ring.finish(first_step=10, steps=5)
        for k, v in ((0, ring.ret[:n]), (1, ring.len[:n].astype(np.float64))):
            ref = math.fsum(v.tolist())
            bound = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(v).tolist())
            S = cm.tm.tree_sum(v)
            print(f"n={n} scale={scale} [{k}]: |S - fsum| {abs(S - ref):.3g} bound {bound:.3g}")
            assert abs(S - ref) <= bound
            assert got[k] == S / np.float64(n)  # (the mean is S divided once)
        assert got[2] == n and got[3] == n and got[4] == 15 and not got[5:].any()


def test_the_finish_model_reports_nan_on_an_empty_ring_counts_per_call_and_sums_by_slot():
    ring = cm.Ring(7)
    got = ring.finish(3, 4)
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2:5].tolist() == [0.0, 0.0, 7.0] and not got[5:].any()
    ring.step(np.array([1, 0, 1], bool), np.array([1.5, 9.0, 2.5]), np.array([10, 99, 20], np.int32))
    got = ring.finish(0, 1)
    assert got[:5].tolist() == [2.0, 15.0, 2.0, 2.0, 1.0]
    ring.step(np.array([0, 1, 0], bool), np.array([0.0, 5.0, 0.0]), np.array([0, 30, 0], np.int32))
    got = ring.finish(1, 1)
    assert got[:5].tolist() == [3.0, 20.0, 1.0, 3.0, 2.0]
    assert cm.launches_ppo(9, True) == 48 and cm.launches_ppo(1, False) == 7
    assert cm.launches_offpolicy(4, True) == 21 and cm.launches_offpolicy(4, False, 2, 4, True) == 19
