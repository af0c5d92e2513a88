"""SAC's collector and evaluation without a GPU: the second public header (include/fleet_hip_sac_loop.h) compiles on its own, declares
exactly the two new families and leaves include/fleet_hip.h alone; bindings, exports and struct layouts against a compiled probe; every
refusal that needs no handle, word for word; the uniform kernel and the off-policy loop exist once in the sources; the launch counts."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sac_loop_model as sm

ROOT = sm.ROOT
COLLECT_ENTRIES = ("fleet_saccollect_last_error", "fleet_saccollect_uniform_dev", "fleet_saccollect_create", "fleet_saccollect_sac_dev")
EVAL_ENTRIES = ("fleet_saceval_create", "fleet_saceval_best_load_dev")
UNIFORM_FIELDS = ["struct_bytes", "env_id_offset", "lo", "hi", "seed", "step", "actions"]
COLLECT_FIELDS = ["struct_bytes", "n_steps", "env_id_offset", "reserved", "learning_starts", "replay", "noise_lo", "noise_hi", "seed", "first_step",
                  "stats"]
HEADER = os.path.join(ROOT, "include", "fleet_hip_sac_loop.h")
NAN = float("nan")


def _csrc(name):
    return open(os.path.join(ROOT, "fleetrl_amd", "csrc", name)).read()


def _git(*args):
    """stdout of a git command in the tree, or None when this is no git checkout (or git is missing)."""
    try:
        out = subprocess.run(["git", "-C", ROOT, *args], capture_output=True, text=True)
    except OSError:
        return None
    return out.stdout if out.returncode == 0 else None


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_second_header_compiles_on_its_own_and_declares_exactly_the_two_families(tmp_path):
    from fleetrl_amd import _capi, build

    src = tmp_path / "only.c"
    src.write_text('#include "fleet_hip_sac_loop.h"\nint main(void){return (int)sizeof(FleetSacCollectArgs) == 0;}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "only")], check=True)
    hdr = open(HEADER).read()
    assert '#include "fleet_hip.h"' in hdr and "#define FLEET_ABI_VERSION" not in hdr
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in hdr[:600]
    declared = re.findall(r"^FLEET_API (?:int|const char\*)\s+(fleet_\w+)\s*\(", hdr, flags=re.M)
    assert len(declared) == len(set(declared))
    assert set(declared) == set(COLLECT_ENTRIES) | set(EVAL_ENTRIES)
    assert not re.findall(r"^(?:extern\s+)?(?:FLEET_API\s+)?(?:extern\s+)?(?:int|const char\*)\s+(?!fleet_sac(?:collect|eval)_)\w+\s*\(", hdr, flags=re.M)
    assert _capi.SACCOLLECT_SYMBOLS == COLLECT_ENTRIES and _capi.SACEVAL_SYMBOLS == EVAL_ENTRIES
    assert all(n.startswith("fleet_saccollect_") for n in COLLECT_ENTRIES) and all(n.startswith("fleet_saceval_") for n in EVAL_ENTRIES)
    for said in ("} FleetSacUniformArgs;", "} FleetSacCollectArgs;", "5 n_steps + 1 launches with a normaliser, 4 n_steps + 1 without",
                 "4 n_steps + 5 launches with a normaliser,", "3 n_steps + 4 without, one more with sync_from", "scale_action(sample)",
                 "the action the env got", "explore_uniform", "deterministic = 1", "WHOLE image", "critic 0, then of critic 1",
                 "fleet_qtarget_set_stream them to the env's first", "Out of scope", "gSDE", "stochastic", "152 bytes"):
        assert said in hdr, said
    # the lists are new ones: disjoint from every other, and outside EXPORTED_SYMBOLS, which still ends with the evaluation's
    new = set(COLLECT_ENTRIES) | set(EVAL_ENTRIES)
    assert not set(COLLECT_ENTRIES) & set(EVAL_ENTRIES)
    for name, value in vars(_capi).items():
        if name.endswith("_SYMBOLS") and name not in ("SACCOLLECT_SYMBOLS", "SACEVAL_SYMBOLS"):
            assert not new & set(value), name
    assert _capi.EXPORTED_SYMBOLS[-len(_capi.EVAL_SYMBOLS):] == _capi.EVAL_SYMBOLS
    # no existing regex over the first header meets the new names
    first = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert "fleet_saccollect_" not in first and "fleet_saceval_" not in first
    assert not re.match(r"fleet_collect_\w+|fleet_eval_\w+|fleet_sac_\w+|fleet_sactrain_\w+", "fleet_saccollect_create")
    assert not re.match(r"fleet_collect_\w+|fleet_eval_\w+|fleet_sac_\w+|fleet_sactrain_\w+", "fleet_saceval_create")
    assert os.path.join("..", "..", "include", "fleet_hip_sac_loop.h") in build.HEADERS and os.path.join("..", "..", "include", "fleet_hip.h") in build.HEADERS
    graft = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_capi.SACCOLLECT_SYMBOLS + _capi.SACEVAL_SYMBOLS" in graft and "_capi.SACTRAIN_SYMBOLS" in graft
    # include/fleet_hip.h is as it was: the change that brought the second header does not name it (no git checkout: nothing to ask)
    added = _git("log", "--diff-filter=A", "--format=%H", "--", "include/fleet_hip_sac_loop.h")
    if added is not None:
        commit = added.split()[-1] if added.split() else None
        names = _git("diff", "--name-only", commit + "^", commit) if commit else _git("diff", "--name-only", "HEAD")
        assert names is None or "include/fleet_hip.h" not in names.split()  # (None: a shallow history without the parent)


def test_every_entry_is_bound_with_its_restype_and_exported_by_the_library():
    from fleetrl_amd import _capi, build

    lib = _capi.load_library()
    raw = C.CDLL(build.lib_path())
    for name in COLLECT_ENTRIES + EVAL_ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
        assert getattr(raw, name) is not None
    assert len(lib.fleet_saccollect_uniform_dev.argtypes) == 3 and len(lib.fleet_saccollect_create.argtypes) == 5
    assert len(lib.fleet_saccollect_sac_dev.argtypes) == 2 and len(lib.fleet_saccollect_last_error.argtypes) == 1
    assert len(lib.fleet_saceval_create.argtypes) == 5 and len(lib.fleet_saceval_best_load_dev.argtypes) == 2


def test_the_python_surface_names_the_new_pieces():
    import inspect

    import fleetrl_amd
    from fleetrl_amd import collect, eval_callback, sac

    assert fleetrl_amd.DeviceSACCollect is collect.DeviceSACCollect and "DeviceSACCollect" in collect.__all__
    assert issubclass(collect.DeviceSACCollect, collect._DeviceCollect) and collect.DeviceSACCollect._prefix == "collect"
    assert collect.DeviceSACCollect._create_entry == "fleet_saccollect_create" and collect.DeviceTD3Collect._create_entry == "fleet_collect_create"
    assert "__init__" in vars(collect._DeviceCollect) and collect.DeviceSACCollect.set_stream is collect._DeviceCollect.set_stream
    sig = inspect.signature(collect.DeviceSACCollect.collect)
    assert list(sig.parameters) == ["self", "replay", "n_steps", "learning_starts", "low", "high", "seed", "first_step", "env_id_offset", "stats_out"]
    assert (sig.parameters["low"].default, sig.parameters["high"].default, sig.parameters["env_id_offset"].default) == (-1.0, 1.0, 0)
    sig = inspect.signature(sac.DeviceSACNetworks.sample_uniform)
    assert list(sig.parameters) == ["self", "num_envs", "low", "high", "seed", "step", "env_id_offset", "actions_out"]
    assert all(p.kind is p.KEYWORD_ONLY for n, p in sig.parameters.items() if n not in ("self", "num_envs"))
    assert "stochastic evaluation" in eval_callback.__doc__.split("Out of scope")[1]
    assert "SAC" not in collect.__doc__.split("Out of scope")[1]


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetSacUniformArgs", _capi.FleetSacUniformArgs, UNIFORM_FIELDS),
                               ("FleetSacCollectArgs", _capi.FleetSacCollectArgs, COLLECT_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["sizeof(FleetCollectInfo)", "sizeof(FleetCollectParams)", "sizeof(FleetEvalParams)", "sizeof(FleetEvalInfo)"]
    want += [152, 8, 8, 168]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip_sac_loop.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert (C.sizeof(_capi.FleetSacUniformArgs), C.sizeof(_capi.FleetSacCollectArgs), C.sizeof(_capi.FleetCollectInfo)) == (40, 64, 152)


# ---- refusals that need no handle --------------------------------------------------------------------------------------------------
def _uniform(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetSacUniformArgs()
    a.struct_bytes, a.env_id_offset, a.lo, a.hi, a.seed, a.step, a.actions = C.sizeof(a), 0, -1.0, 1.0, 1, 0, 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _collect(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetSacCollectArgs()
    a.struct_bytes, a.n_steps, a.env_id_offset, a.learning_starts, a.replay = C.sizeof(a), 8, 0, 4, 4096
    a.noise_lo, a.noise_hi, a.seed, a.first_step, a.stats = -1.0, 1.0, 1, 0, 8192
    for k, v in kw.items():
        setattr(a, k, v)
    return a


UNIFORM_REFUSALS = {
    "struct_bytes": (4, dict(struct_bytes=32), "FleetSacUniformArgs.struct_bytes does not match this library"),
    "E-zero": (0, {}, "E must be >= 1, got 0"),
    "E-negative": (-2, {}, "E must be >= 1, got -2"),
    "actions-null": (4, dict(actions=None), "null actions"),
    "env_id_offset": (4, dict(env_id_offset=-1), "env_id_offset must be >= 0, got -1"),
    "bounds-crossed": (4, dict(lo=1.0, hi=-1.0), "the bounds need lo <= hi"),
    "bounds-nan-lo": (4, dict(lo=NAN), "the bounds need lo <= hi"),
    "bounds-nan-hi": (4, dict(hi=NAN), "the bounds need lo <= hi"),
}
COLLECT_REFUSALS = {
    "struct_bytes": (dict(struct_bytes=56), "FleetSacCollectArgs.struct_bytes does not match this library"),
    "n_steps-zero": (dict(n_steps=0), "n_steps must be >= 1, got 0"),
    "n_steps-negative": (dict(n_steps=-3), "n_steps must be >= 1, got -3"),
    "reserved": (dict(reserved=2), "reserved must be 0"),
    "env_id_offset": (dict(env_id_offset=-7), "env_id_offset must be >= 0, got -7"),
    "replay-null": (dict(replay=None), "null replay handle"),
    "bounds-crossed": (dict(noise_lo=1.0, noise_hi=-1.0), "the bounds need noise_lo <= noise_hi"),
    "bounds-nan": (dict(noise_hi=NAN), "the bounds need noise_lo <= noise_hi"),
    "stats-null": (dict(stats=None), "null stats"),
}


@pytest.mark.parametrize("case", sorted(UNIFORM_REFUSALS))
def test_the_uniform_draw_refuses_bad_arguments_before_it_looks_at_the_handle(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    E, fields, word = UNIFORM_REFUSALS[case]
    assert lib.fleet_saccollect_uniform_dev(None, E, C.byref(_uniform(**fields))) == _capi.ERR_INVALID
    assert lib.fleet_saccollect_last_error(None).decode() == "fleet_saccollect_uniform_dev: " + word


@pytest.mark.parametrize("case", sorted(COLLECT_REFUSALS))
def test_the_run_call_refuses_bad_arguments_before_it_looks_at_the_handle(case):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = COLLECT_REFUSALS[case]
    assert lib.fleet_saccollect_sac_dev(None, C.byref(_collect(**fields))) == _capi.ERR_INVALID
    assert lib.fleet_saccollect_last_error(None).decode() == "fleet_saccollect_sac_dev: " + word


def test_good_arguments_name_the_null_handle_and_null_structs_are_refused():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_saccollect_last_error(None).decode()  # noqa: E731
    assert lib.fleet_saccollect_uniform_dev(None, 4, None) == _capi.ERR_INVALID and last() == "fleet_saccollect_uniform_dev: null FleetSacUniformArgs"
    assert lib.fleet_saccollect_sac_dev(None, None) == _capi.ERR_INVALID and last() == "fleet_saccollect_sac_dev: null FleetSacCollectArgs"
    for ok in (_uniform(), _uniform(lo=0.25, hi=0.25), _uniform(seed=2 ** 64 - 1, step=2 ** 63, env_id_offset=2 ** 31 - 1)):
        assert lib.fleet_saccollect_uniform_dev(None, 2 ** 31 - 1, C.byref(ok)) == _capi.ERR_INVALID and last() == "fleet_saccollect_uniform_dev: null handle"
    for ok in (_collect(), _collect(noise_lo=0.5, noise_hi=0.5), _collect(learning_starts=2 ** 64 - 1, n_steps=2 ** 31 - 1, first_step=2 ** 63)):
        assert lib.fleet_saccollect_sac_dev(None, C.byref(ok)) == _capi.ERR_INVALID and last() == "fleet_saccollect_sac_dev: null handle"
    # the string is the collect family's: one place to ask after a call without a handle
    assert lib.fleet_collect_last_error(None).decode() == last()
    assert lib.fleet_saceval_best_load_dev(None, 4096) == _capi.ERR_INVALID
    assert lib.fleet_eval_last_error(None).decode() == "fleet_saceval_best_load_dev: null handle"


def test_the_create_entries_refuse_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    h, fake = C.c_void_p(), C.c_void_p(4096)  # (never dereferenced: a refusal in front of it is met first)
    for create, last, entry, good, bad in (
            (lib.fleet_saccollect_create, lib.fleet_saccollect_last_error, "fleet_saccollect_create",
             _capi.FleetCollectParams(C.sizeof(_capi.FleetCollectParams), 100),
             ((_capi.FleetCollectParams(4, 100), "FleetCollectParams.struct_bytes does not match this library"),
              (_capi.FleetCollectParams(8, 0), "stats_window must be in 1..4096, got 0"),
              (_capi.FleetCollectParams(8, 4097), "stats_window must be in 1..4096, got 4097"))),
            (lib.fleet_saceval_create, lib.fleet_eval_last_error, "fleet_saceval_create", _capi.FleetEvalParams(C.sizeof(_capi.FleetEvalParams), 5),
             ((_capi.FleetEvalParams(4, 5), "FleetEvalParams.struct_bytes does not match this library"),
              (_capi.FleetEvalParams(8, 0), "max_episodes must be in 1..65536, got 0"),
              (_capi.FleetEvalParams(8, 65537), "max_episodes must be in 1..65536, got 65537")))):
        said = lambda: last(None).decode()  # noqa: E731
        assert create(None, None, fake, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h and said() == entry + ": null env handle"
        assert create(fake, None, None, C.byref(good), C.byref(h)) == _capi.ERR_INVALID and not h and said() == entry + ": null networks handle"
        assert create(fake, None, fake, C.byref(good), None) == _capi.ERR_INVALID and said() == entry + ": null output handle"
        assert create(fake, None, fake, None, C.byref(h)) == _capi.ERR_INVALID and said() == entry + ": null " + type(good).__name__
        for p, word in bad:
            assert create(fake, None, fake, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h and said() == entry + ": " + word


# ---- the sources -------------------------------------------------------------------------------------------------------------------
def test_the_uniform_kernel_and_the_offpolicy_loop_exist_once():
    policy, collect, sac, evaluate = _csrc("fleet_policy.hip"), _csrc("fleet_collect.hip"), _csrc("fleet_sac.hip"), _csrc("fleet_eval.hip")
    launch = re.compile(r"hipLaunchKernelGGL\(\s*explore_uniform\b|explore_uniform\s*<<<")
    assert policy.count("void explore_uniform(") == 1 and len(launch.findall(policy)) == 1
    for name, src in (("fleet_collect.hip", collect), ("fleet_sac.hip", sac), ("fleet_eval.hip", evaluate)):
        assert "void explore_uniform(" not in src and not launch.findall(src), name
    # one launch function, declared in the internal header, called by the policy's UNIFORM branch and by the new entry
    assert "hipError_t policy_launch_uniform(hipStream_t stream, int E, int A, const PolicyUniformArgs& u);" in _csrc("fleet_policy.h")
    assert policy.count("policy_launch_uniform(") == 2 and collect.count("policy_launch_uniform(") == 1
    assert policy.index("hipError_t policy_launch_uniform(") < policy.index("int fleet_explore_act_dev(")
    # the off-policy loop's body once: one step, one normaliser step, one add in the loop both run calls go through
    assert collect.count("fleet_replay_add_dev(") == 1 and collect.count("int offpolicy_loop(") == 1
    assert collect.count("return offpolicy_loop(h, ") == 2
    body = collect[collect.index("int offpolicy_loop("):collect.index("int create_on(")]
    for call in ("fleet_step_dev(", "fleet_norm_step_dev(", "fleet_replay_add_dev(", "launch_episodes(", "launch_finish("):
        assert body.count(call) == 1, call
    assert collect.count("fleet_step_dev(") == 2  # (the loop's and the PPO call's)
    # the evaluation's loop once as well: the action is chosen inside it
    assert evaluate.count("eval_episodes<true>") == 1 and evaluate.count("fleet_sac_act_dev(") == 1 and evaluate.count("fleet_policy_forward_dev(") == 1
    assert "atomic" not in collect.split("// ---- host")[0].replace("No atomics", "")


def test_the_launch_counts():
    assert sm.launches_collect(5, True) == 26 and sm.launches_collect(5, False) == 21 and sm.launches_collect(1, True) == 6
    assert sm.launches_collect(12, False) == 49
    for n in (1, 5, 12):
        for with_norm in (False, True):  # the TD3 collector's count without a noise handle, before and after the warm-up
            assert sm.launches_collect(n, with_norm) == sm.cm.launches_offpolicy(n, with_norm, 0, 3, False) == sm.cm.launches_offpolicy(n, with_norm, 7, 3, False)
    assert sm.launches_eval(16, True, True) == 70 and sm.launches_eval(16, True) == 69 and sm.launches_eval(16, False) == 52
    assert sm.launches_eval(8, False) == sm.em.launches(8, False) == 28
    assert [sm.warm_up(s, 3) for s in range(5)] == [True, True, True, False, False]
