"""The agent's evaluation on the device without a GPU: the C ABI's section, its position, bindings and struct layouts against a compiled
probe, every refusal that needs no handle, the model's episode lists (tests/eval_model.py) against a per-env loop written straight from
SB3's evaluate_policy, the ordered sum against math.fsum, the std against np.std within a derived bound, and the gate's truth table."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import eval_model as em

ROOT = em.ROOT
ENTRIES = ("fleet_eval_create", "fleet_eval_destroy", "fleet_eval_last_error", "fleet_eval_describe", "fleet_eval_sync_norm_dev", "fleet_eval_run_dev",
           "fleet_eval_episodes_dev", "fleet_eval_clear_dev", "fleet_eval_best_load_dev", "fleet_eval_best_export_dev", "fleet_eval_episodes_read")
PARAM_FIELDS = ["struct_bytes", "max_episodes"]
ARGS_FIELDS = ["struct_bytes", "n_eval_episodes", "n_steps", "reward_source", "sync_from", "reserved", "num_timesteps", "stats"]
INFO_FIELDS = ["num_envs", "obs_dim", "act_dim", "max_episodes", "has_norm", "launches", "block_bytes", "snapshot_floats", "obs", "raw_obs", "actions",
               "raw_reward", "reward", "done", "sums", "lengths", "counts", "ep_reward", "ep_length", "listed", "best_mean_reward", "evaluations", "gate",
               "snapshot"]
TITLE = "evaluation of the agent on the device"
EXPLORE_TITLE = "exploration actions on the device"
NOISE_TITLE = "correlated action noise on the device"
U = 2.0 ** -53


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_lies_between_the_exploration_and_the_noise_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_eval_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.EVAL_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    assert _capi.EXPORTED_SYMBOLS[-len(ENTRIES):] == _capi.EVAL_SYMBOLS  # appended
    assert hdr.count("---- " + TITLE) == 1
    titles = re.findall(r"^/\* ---- (.*?) \(", hdr, flags=re.M)
    assert titles.count(TITLE) == 1 and not any(t in TITLE or TITLE in t for t in titles if t != TITLE)
    at = titles.index(TITLE)
    assert titles[at - 1] == EXPLORE_TITLE and titles[at + 1] == NOISE_TITLE
    assert titles[-1] == "PPO minibatch gradients on the device"  # (the last section stays the last)
    assert hdr.index("int fleet_explore_act_dev(") < hdr.index("---- " + TITLE) < hdr.index("---- " + NOISE_TITLE)
    section = hdr[hdr.index("---- " + TITLE):hdr.index("---- " + NOISE_TITLE)]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    for later in titles[at + 1:]:  # the tests of the later sections find them with hdr.index(title)
        assert later not in section, later
    for said in ("} FleetEvalParams;", "} FleetEvalArgs;", "} FleetEvalInfo;", "#define FLEET_EVAL_MAX_EPISODES 65536", "#define FLEET_EVAL_STATS 16",
                 "target_i = (n_eval_episodes + i) / E", "listed += c", "must outlive", "4 n_steps + 5 launches with a normaliser, 3 n_steps + 4 without",
                 "one more with sync_from", "NaN when n == 0", "ONE stream", "no atomics", "starts at -inf", "false for NaN", "population std",
                 "Out of scope", "real_time", "before the first launch", "sqrt(var + dst's epsilon)", "iff the gate is", "Monitor"):
        assert said in section, said
    assert not re.search(r"^(?:int|const char\*)\s+fleet_(?!eval_)", section, flags=re.M)  # no entry of a neighbour in it
    assert len(re.findall(r"^/\* ---- ", section, flags=re.M)) == 0
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_eval_create.argtypes) == 5 and len(lib.fleet_eval_run_dev.argtypes) == 2 and len(lib.fleet_eval_sync_norm_dev.argtypes) == 2
    assert len(lib.fleet_eval_episodes_dev.argtypes) == 8 and len(lib.fleet_eval_best_export_dev.argtypes) == 3
    assert len(lib.fleet_eval_best_load_dev.argtypes) == 2 and len(lib.fleet_eval_episodes_read.argtypes) == 4


def test_the_family_is_built_exported_and_restated_with_the_headers_constants():
    import fleetrl_amd
    from fleetrl_amd import _capi, build, eval_callback

    assert "fleet_eval.hip" in build.SOURCES and "fleet_eval.h" in build.HEADERS
    assert fleetrl_amd.DeviceEvalCallback is eval_callback.DeviceEvalCallback and eval_callback.DeviceEvalCallback._prefix == "eval"
    assert eval_callback.STATS == em.STATS
    assert (_capi.EVAL_MAX_EPISODES, _capi.EVAL_STATS) == (em.MAX_EPISODES, em.STATS_LEN) == (65536, 16)
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_eval.h")).read()
    for name, want in (("kEvalScanThreads", em.SCAN_THREADS), ("kEvalThreads", em.LANES), ("kEvalMaxEpisodes", em.MAX_EPISODES),
                       ("kEvalStats", em.STATS_LEN)):
        assert re.search(rf"constexpr int {name} = (\d+);", src).group(1) == str(want), name
    kernels = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_eval.hip")).read()
    assert "atomic" not in kernels.split("// ---- host")[0].replace("No atomics", "")  # the kernels use none
    norm = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_norm.hip")).read()
    assert norm.index("void norm_derive(") < norm.index("void norm_sync(") < norm.index("struct ApplyArgs")  # next to norm_derive
    internal = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_norm.h")).read()
    assert "fleet_norm_enqueue_sync(" in internal and "fleet_norm_check_sync(" in internal


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetEvalParams", _capi.FleetEvalParams, PARAM_FIELDS), ("FleetEvalArgs", _capi.FleetEvalArgs, ARGS_FIELDS),
                               ("FleetEvalInfo", _capi.FleetEvalInfo, INFO_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["FLEET_EVAL_MAX_EPISODES", "FLEET_EVAL_STATS"]
    want += [_capi.EVAL_MAX_EPISODES, _capi.EVAL_STATS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert (C.sizeof(_capi.FleetEvalParams), C.sizeof(_capi.FleetEvalArgs), C.sizeof(_capi.FleetEvalInfo)) == (8, 48, 168)


# ---- refusals that need no device --------------------------------------------------------------------------------------------------
def _args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetEvalArgs()
    a.struct_bytes, a.n_eval_episodes, a.n_steps, a.reward_source, a.num_timesteps, a.stats = C.sizeof(a), 5, 8, 0, 1000, 8192
    for k, v in kw.items():
        setattr(a, k, v)
    return a


RUN_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=40), "FleetEvalArgs.struct_bytes does not match this library"),
    "episodes-zero": (dict(n_eval_episodes=0), "n_eval_episodes must be >= 1, got 0"),
    "episodes-negative": (dict(n_eval_episodes=-2), "n_eval_episodes must be >= 1, got -2"),
    "n_steps-zero": (dict(n_steps=0), "n_steps must be >= 1, got 0"),
    "source-2": (dict(reward_source=2), "reward_source must be 0 or 1, got 2"),
    "source-negative": (dict(reward_source=-1), "reward_source must be 0 or 1, got -1"),
    "reserved": (dict(reserved=1), "reserved must be 0"),
    "stats-null": (dict(stats=None), "null stats"),
}


@pytest.mark.parametrize("case", sorted(RUN_REFUSALS))
def test_the_run_call_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_eval_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = RUN_REFUSALS[case]
    rc = lib.fleet_eval_run_dev(None, C.byref(_args(**fields)))
    why = lib.fleet_eval_last_error(None).decode()
    assert rc == _capi.ERR_INVALID and why == "fleet_eval_run_dev: " + word, why


def test_good_arguments_name_the_null_handle_and_null_structs_are_refused():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_eval_last_error(None).decode()  # noqa: E731
    assert lib.fleet_eval_run_dev(None, None) == _capi.ERR_INVALID and last() == "fleet_eval_run_dev: null FleetEvalArgs"
    for ok in (_args(), _args(reward_source=1, sync_from=4096, n_eval_episodes=2 ** 31 - 1, n_steps=2 ** 31 - 1, num_timesteps=2 ** 64 - 1)):
        assert lib.fleet_eval_run_dev(None, C.byref(ok)) == _capi.ERR_INVALID and last() == "fleet_eval_run_dev: null handle"
    fn = lib.fleet_eval_episodes_dev
    for args, word in (((256, 512, 1024, 2048, 0, 5, 0), "E must be >= 1, got 0"), ((256, 512, 1024, 2048, 4, 0, 0), "n_eval_episodes must be >= 1, got 0"),
                       ((256, 512, 1024, 2048, 4, 5, 2), "reward_source must be 0 or 1, got 2"), ((None, 512, 1024, 2048, 4, 5, 0), "null done"),
                       ((256, None, 1024, 2048, 4, 5, 0), "null reward"), ((256, 512, None, 2048, 4, 5, 1), "null ep_return"),
                       ((256, 512, 1024, None, 4, 5, 1), "null ep_len"), ((256, 512, None, None, 4, 5, 0), "null handle"),
                       ((256, 512, 1024, 2048, 4, 5, 1), "null handle")):
        assert fn(None, *args) == _capi.ERR_INVALID and last() == "fleet_eval_episodes_dev: " + word, word
    for name, args in (("fleet_eval_clear_dev", ()), ("fleet_eval_best_load_dev", (4096,)), ("fleet_eval_best_export_dev", (None, 0)),
                       ("fleet_eval_episodes_read", (None, None, None))):
        assert getattr(lib, name)(None, *args) == _capi.ERR_INVALID and last() == name + ": null handle"
    sync = lib.fleet_eval_sync_norm_dev
    assert sync(None, None) == _capi.ERR_INVALID and last() == "fleet_eval_sync_norm_dev: null destination normaliser"
    assert sync(C.c_void_p(4096), None) == _capi.ERR_INVALID and last() == "fleet_eval_sync_norm_dev: null source normaliser"


def test_create_and_describe_refuse_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_eval_last_error(None).decode()  # noqa: E731
    h = C.c_void_p()
    fake = C.c_void_p(4096)  # (never dereferenced: a refusal in front of it is met first)
    good = _capi.FleetEvalParams(C.sizeof(_capi.FleetEvalParams), 5)
    create = lib.fleet_eval_create
    assert create(None, None, fake, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h and last() == "fleet_eval_create: null env handle"
    assert create(fake, None, None, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h and last() == "fleet_eval_create: null policy handle"
    assert create(fake, None, fake, C.byref(good), None) == _capi.ERR_INVALID and last() == "fleet_eval_create: null output handle"
    assert create(fake, None, fake, None, C.byref(h)) == _capi.ERR_INVALID and last() == "fleet_eval_create: null FleetEvalParams"
    for p, word in ((_capi.FleetEvalParams(4, 5), "FleetEvalParams.struct_bytes does not match this library"),
                    (_capi.FleetEvalParams(8, 0), "max_episodes must be in 1..65536, got 0"),
                    (_capi.FleetEvalParams(8, -5), "max_episodes must be in 1..65536, got -5"),
                    (_capi.FleetEvalParams(8, 65537), "max_episodes must be in 1..65536, got 65537")):
        assert create(fake, None, fake, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
        assert last() == "fleet_eval_create: " + word
    assert lib.fleet_eval_destroy(None) == _capi.OK
    assert lib.fleet_eval_describe(None, None) == _capi.ERR_INVALID


def test_the_python_layer_refuses_a_real_time_env_before_it_touches_anything():
    """Episode lengths in steps are not fixed there, and n_steps is fixed when the call is enqueued."""
    import types

    from fleetrl_amd import DeviceEvalCallback

    core = types.SimpleNamespace(params=types.SimpleNamespace(real_time=1, episode_steps=8))
    with pytest.raises(ValueError, match="real_time env is refused"):
        DeviceEvalCallback(None, types.SimpleNamespace(core=core, num_envs=3))


# ---- the lists -------------------------------------------------------------------------------------------------------------------------
def _patterns(E, steps, rng):
    """Done patterns with ends at different steps, several in one step, every env ending often enough to go past any quota."""
    none, every, one = np.zeros(E, bool), np.ones(E, bool), np.zeros(E, bool)
    one[E // 2] = True
    out = [none, one, every, rng.random(E) < 0.5, every, none, rng.random(E) < 0.3, every]
    while len(out) < steps:
        out.append(rng.random(E) < rng.choice([0.1, 0.5, 0.9, 1.0]))
    return out


def _cases(E):
    return sorted({n for n in (1, E - 1, E, E + 1, 2 * E, 2 * E + 3, 3 * E) if n >= 1})


@pytest.mark.parametrize("E", [1, 2, 3, 7, 64, 65, 130])
def test_the_models_lists_are_sb3s_in_values_and_in_order(E):
    """evaluate_policy's loop per env (em.sb3_evaluate, from SB3's source) against the model's step: n_eval_episodes < E (targets of 0),
    = E, and E + 1 .. 3 E; envs past their quota keep finishing and must not be listed."""
    for n_eval in _cases(E):
        rng = np.random.default_rng(E * 1000 + n_eval)
        pats = _patterns(E, 24, rng)
        rewards = [rng.standard_normal(E) * 100 for _ in pats]
        want_r, want_n = em.sb3_evaluate(zip(rewards, pats), n_eval)
        ev = em.Evaluation(E, max_episodes=n_eval)
        for r, d in zip(rewards, pats):
            ev.step(d, r, n_eval)
        got_r, got_n = ev.lists()
        assert len(want_r) == n_eval, (E, n_eval)  # (the patterns meet every quota)
        assert got_r.tobytes() == np.array(want_r, np.float64).tobytes() and got_n.tolist() == [int(x) for x in want_n], (E, n_eval)
        assert ev.listed == n_eval and ev.counts.tolist() == em.targets(n_eval, E).tolist()
        assert em.targets(n_eval, E).sum() == n_eval and (n_eval >= E or em.targets(n_eval, E)[0] == 0)


def test_the_monitor_source_lists_the_given_records_and_a_full_list_drops_the_rest():
    E, n_eval = 5, 7
    rng = np.random.default_rng(3)
    ev, plain = em.Evaluation(E, max_episodes=4), em.Evaluation(E, max_episodes=n_eval)
    for _ in range(6):
        d, r = rng.random(E) < 0.6, rng.standard_normal(E)
        ret, length = rng.standard_normal(E) * 10, rng.integers(1, 99, E).astype(np.int32)
        before = plain.listed
        order = [i for i in range(E) if d[i] and plain.counts[i] < em.targets(n_eval, E)[i]]
        ev.step(d, r, n_eval, 1, ret, length)
        plain.step(d, r, n_eval, 1, ret, length)
        assert plain.ep_reward[before:plain.listed].tolist() == ret[order].tolist() and plain.ep_length[before:plain.listed].tolist() == length[order].tolist()
    assert plain.listed == ev.listed == n_eval and ev.lists()[0].size == 4
    assert ev.ep_reward.tolist() == plain.ep_reward[:4].tolist()  # slots at or beyond max_episodes are not written
    ev.clear()
    assert ev.listed == 0 and not ev.counts.any() and not ev.sums.any() and not ev.lengths.any()


# ---- the closing launch's model ----------------------------------------------------------------------------------------------------
def _exact(x):
    n = len(x)
    mu = math.fsum(x.tolist()) / n
    return mu, math.sqrt(math.fsum(((x - mu) ** 2).tolist()) / n)


@pytest.mark.parametrize("n", [1, 2, 5, 100, 255, 256, 257, 1000, 4096])
def test_mean_and_std_stay_within_derived_bounds_of_fsum_and_np_std(n):
    """Mean: |S - fsum| <= (n - 1) u sum|x|, u = 2^-53, the bound of an ordered float64 sum (n - 1 additions, each rounding a partial sum
    of at most sum|x| in magnitude by at most u of it).
    Std: with m the computed mean, |m - mu| <= dm := u (sum|x| + |mu|) (that bound over n, and the division's rounding).  The deviations
    d'_i = fl(x_i - m) differ from d_i = x_i - mu by the common shift mu - m and a rounding u |d'_i|; in V = sum d_i^2 the shift's first
    order term vanishes (sum d_i = 0) and leaves n dm^2, the roundings of the differences and the squares leave 3 u V, the ordered sum
    (n - 1) u V: |V' - V| <= (n + 2) u V + n dm^2.  Dividing by n and the root add 2 u and halve the relative error:
        |std' - std| <= B := std (n / 2 + 3) u + dm^2 / (2 std),   taken as std (n / 2 + 4) u + dm^2 / std for the second-order terms.
    np.std forms the same expression with pairwise sums, whose error bound is smaller than the ordered sum's, so it lies within B of the
    exact std as well: |std' - np.std| <= 2 B.  Inputs: spread of at least a tenth of their magnitude (std >= |mean| / 10)."""
    rng = np.random.default_rng(n)
    for scale, offset in ((1.0, 0.0), (1e6, 5e6), (1e-3, -4e-3), (50.0, -400.0)):
        z = rng.standard_normal(n)
        if n <= 5:  # (few samples: alternate about the offset, so that the spread holds)
            z = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) + 0.1 * z
        x = offset + z * scale
        got_mean, got_std = em.mean_std(x)
        S = em.tm.tree_sum(x)
        ref = math.fsum(x.tolist())
        bound = (n - 1) * U * math.fsum(np.abs(x).tolist())
        print(f"n={n} scale={scale}: |S - fsum| {abs(S - ref):.3g} bound {bound:.3g}")
        assert abs(S - ref) <= bound and got_mean == S / np.float64(n)
        mu, sd = _exact(x)
        if n == 1:
            assert got_std == 0.0 == np.std(x)
            continue
        assert sd >= abs(mu) / 10
        dm = U * (math.fsum(np.abs(x).tolist()) + abs(mu))
        B = sd * (n / 2 + 4) * U + dm * dm / sd
        print(f"    |std - np.std| {abs(got_std - np.std(x)):.3g} bound {2 * B:.3g}; |std - exact| {abs(got_std - sd):.3g}")
        assert abs(got_std - sd) <= B and abs(got_std - np.std(x)) <= 2 * B


def test_the_finish_model_reports_nan_on_empty_lists_population_std_and_counts_evaluations():
    ev = em.Evaluation(3, 8)
    got = ev.finish(7)
    assert np.isnan(got[:4]).all() and got[4] == 0 and got[5] == -np.inf and got[6] == 0 and got[7] == 7 and got[8] == 1 and not got[9:].any()
    for t in range(2):
        ev.step(np.array([1, 0, 1], bool), np.array([1.0, 9.0, 3.0 + 2 * t]), n_eval_episodes=4)
    got = ev.finish(100)  # targets (1, 1, 2): env 0 once, env 2 twice -> rewards 1, 3, 5; env 1 never finished
    assert ev.lists()[0].tolist() == [1.0, 3.0, 5.0] and ev.lists()[1].tolist() == [1, 1, 1]
    assert got[0] == 3.0 and got[1] == np.std([1.0, 3.0, 5.0]) and got[2] == 1.0 and got[3] == 0.0 and got[4] == 3
    assert got[5] == 3.0 and got[6] == 1.0 and got[7] == 100 and got[8] == 2
    assert em.launches(8, True, True) == 38 and em.launches(8, True) == 37 and em.launches(8, False) == 28 and em.launches(1, False) == 7


def test_the_gate_is_sb3s_strict_comparison():
    """-inf start: any finite mean is a new best; an equal mean is not; a NaN mean is not, and leaves the best alone."""
    assert em.new_best(-1e300, -np.inf) and em.new_best(0.0, -1.0) and not em.new_best(-1.0, -1.0) and not em.new_best(-2.0, -1.0)
    assert not em.new_best(np.nan, -np.inf) and not em.new_best(np.nan, 5.0) and not em.new_best(-np.inf, -np.inf)
    ev = em.Evaluation(1, 4)
    seen = []
    for reward in (-5.0, -5.0, -7.0, None, -1.0):
        ev.clear()
        if reward is not None:  # (None: no episode finished, the mean is NaN)
            ev.step(np.array([True]), np.array([reward]), n_eval_episodes=1)
        out = ev.finish()
        seen.append((ev.gate, float(out[5])))
    assert seen == [(1, -5.0), (0, -5.0), (0, -5.0), (0, -5.0), (1, -1.0)] and ev.evaluations == 5
