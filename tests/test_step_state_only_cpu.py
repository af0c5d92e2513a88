"""Which step-kernel launches have a state-only twin (include/fleet_hip.h fleet_step_has_state_only; no GPU needed): exactly the
single-step launches whose env is a group of 64, 128 or 256 lanes with one EV per lane -- the instances `G64|G128|G256.*.single.f32|f64`
of the launch planner.  Smaller groups, the several-EVs-per-lane instance (`w`), K-step launches, real_time and the data log have
none and keep the run-time `outputs_dead` flag.  The planner's visible set is not touched by the twin: tests/test_step_instances_cpu.py
and tests/test_step_planner_pinned_cpu.py pin it."""
import ctypes
import re

import pytest

from fleetrl_amd import _capi

DEGS = (0, 1, 2)
N_SWEEP = (1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 50, 63, 64, 65, 100, 128, 129, 200, 256, 257, 300, 1000)


def _name(E, N, deg, rt, log, act, K, dc):
    return _capi.step_instance(E, N, deg, rt, log, act, K, dc)[0]


def test_a_twin_exactly_for_single_step_groups_of_whole_wavefronts_with_one_ev_per_lane():
    seen = set()
    for N in N_SWEEP:
        for deg in DEGS:
            for rt in (False, True):
                for log in (False, True):
                    for act in (_capi.ACT_F32, _capi.ACT_F64, _capi.POLICY_UNCONTROLLED):
                        for K, dc in ((1, False), (1, True), (4, False)):
                            name = _name(40, N, deg, rt, log, act, K, dc)
                            has = _capi.step_has_state_only(40, N, deg, rt, log, act, K, dc)
                            want = re.fullmatch(r"G(64|128|256)\.\w+\.single\.f(32|64)", name) is not None
                            assert has == want, (name, N, deg, rt, log, act, K, dc)
                            if has:
                                seen.add(name)
    # 3 group sizes x 3 degradation models x 2 action dtypes
    assert len(seen) == 18, sorted(seen)


@pytest.mark.parametrize("N,want", [(32, False), (33, True), (64, True), (65, True), (128, True), (129, True), (256, True), (257, False)])
def test_group_boundaries(N, want):
    for act in (_capi.ACT_F32, _capi.ACT_F64):
        assert _capi.step_has_state_only(7, N, 2, False, False, act) is want
    # the same envs under real_time, with the data log, K steps per launch, with a done_count buffer, under a built-in policy: never
    assert not _capi.step_has_state_only(7, N, 2, True, False)
    assert not _capi.step_has_state_only(7, N, 2, False, True)
    assert not _capi.step_has_state_only(7, N, 2, False, False, _capi.ACT_F32, 8)
    assert not _capi.step_has_state_only(7, N, 2, False, False, _capi.ACT_F32, 1, True)
    assert not _capi.step_has_state_only(7, N, 2, False, False, _capi.POLICY_UNCONTROLLED)


def test_nonsense_arguments_are_refused_like_fleet_step_instance_refuses_them():
    lib = _capi.load_library()
    out = ctypes.c_int32(7)
    buf, grid = ctypes.create_string_buffer(64), ctypes.c_uint32()
    good = (4, 50, 2, 0, 0, _capi.ACT_F32, 1, 0)
    assert lib.fleet_step_has_state_only(*good, ctypes.byref(out)) == _capi.OK and out.value == 1
    for k, bad in ((0, 0), (0, -3), (1, 0), (1, 65536), (2, -1), (2, 3), (5, _capi.ACT_F32 - 1), (5, _capi.POLICY_NIGHT + 1), (6, 0), (6, -2)):
        args = list(good)
        args[k] = bad
        out.value = 7
        assert lib.fleet_step_instance(*args, buf, len(buf), ctypes.byref(grid)) == _capi.ERR_INVALID, args
        assert lib.fleet_step_has_state_only(*args, ctypes.byref(out)) == _capi.ERR_INVALID, args
        assert out.value == 7  # nothing written
    assert lib.fleet_step_has_state_only(*good, None) == _capi.ERR_INVALID
    with pytest.raises(_capi.FleetHipError):
        _capi.step_has_state_only(0, 50, 2, False, False)


def test_entries_are_declared_bound_and_beside_the_other_direct_run_entries():
    import os

    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    lib = _capi.load_library()
    for name in ("fleet_set_direct_state_only", "fleet_direct_packet_counts", "fleet_step_has_state_only"):
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M) and name in _capi.EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes is not None
        assert hdr.index("int fleet_step_instance(") < hdr.index("int %s(" % name) < hdr.index("int fleet_debug_direct_fault(")
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M)
