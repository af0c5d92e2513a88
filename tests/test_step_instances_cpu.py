"""The case list of tests/step_instances.py covers every instance of the step kernel the launch planner can select, in every way the
instance can be used -- checked against the library's own planner (`fleet_step_instance`: no GPU needed).  An instance added to
`plan_step_gd` without a case makes this fail and names it."""
import collections

import pytest

import step_instances as si
from fleetrl_amd import _capi


@pytest.fixture(scope="module")
def reachable():
    return si.reachable()


@pytest.fixture(scope="module")
def cases():
    return si.cases()


def test_the_entry_names_instances_and_refuses_nonsense():
    import ctypes

    assert _capi.step_instance(4096, 50, _capi.DEG_RAINFLOW, False, False) == ("G64.rainflow.single.f32", 1024)  # the benchmark's
    assert _capi.step_instance(4096, 50, _capi.DEG_RAINFLOW, False, False, _capi.ACT_F64)[0] == "G64.rainflow.single.f64"
    assert _capi.step_instance(21, 130, _capi.DEG_RAINFLOW, False, False, _capi.ACT_F32, 61, True) == ("G256.rainflow.multi.tape", 21)
    assert _capi.step_instance(10, 50, _capi.DEG_NONE, False, True)[0] == "G64.none.multi.log"
    assert _capi.step_instance(10, 70, _capi.DEG_LINEAR, True, False) == ("G64w.linear.multi.rt", 3)
    assert _capi.step_instance(5, 3, _capi.DEG_LINEAR, False, False, _capi.POLICY_NIGHT, 7)[0] == "G4.linear.multi.all"
    lib = _capi.load_library()
    grid = ctypes.c_uint32()
    buf = ctypes.create_string_buffer(64)
    for bad in ((0, 5, 0, 0, 0, 0, 1, 0), (4, 0, 0, 0, 0, 0, 1, 0), (4, 5, 3, 0, 0, 0, 1, 0), (4, 5, 0, 0, 0, 5, 1, 0),
                (4, 5, 0, 0, 0, 0, 0, 0), (4, 65536, 0, 0, 0, 0, 1, 0)):
        assert lib.fleet_step_instance(*bad, buf, len(buf), ctypes.byref(grid)) == _capi.ERR_INVALID, bad
    short = ctypes.create_string_buffer(8)
    assert lib.fleet_step_instance(4, 5, 0, 0, 0, 0, 1, 0, short, len(short), ctypes.byref(grid)) == _capi.ERR_INVALID
    assert lib.fleet_step_instance(4, 5, 0, 0, 0, 0, 1, 0, None, 0, ctypes.byref(grid)) == _capi.ERR_INVALID


def test_reachable_set_is_the_one_the_selection_code_describes(reachable):
    """10 lane groups x 3 degradation models x the launch kinds each group admits (fleet_step_plan.h plan_step_gd)."""
    groups = collections.Counter(name.split(".")[0] for name in reachable)
    assert set(groups) == {"G1", "G2", "G4", "G8", "G16", "G32", "G64", "G128", "G256", "G64w"}
    assert all(n % 3 == 0 for n in groups.values())
    assert len(reachable) == 135


def test_every_reachable_instance_has_a_case(reachable, cases):
    covered = {c.instance for c in cases}
    missing = sorted(set(reachable) - covered)
    assert not missing, f"step-kernel instances the planner can select but no case of tests/step_instances.py runs: {missing}"
    stale = sorted(covered - set(reachable))
    assert not stale, f"cases written for instances the planner no longer selects: {stale}"


def test_every_use_of_every_instance_has_a_case(reachable, cases):
    uses = collections.defaultdict(set)
    for c in cases:
        uses[c.instance] |= set(c.uses)
    gaps = {name: sorted(want - uses[name]) for name, want in reachable.items() if want - uses[name]}
    assert not gaps, f"uses of step-kernel instances that no case runs: {gaps}"
    extra = {name: sorted(uses[name] - want) for name, want in reachable.items() if uses[name] - want}
    assert not extra, f"cases that ask an instance for what the C ABI never asks it: {extra}"
    # the multi-use instances really are: everything behind run-time tests -> every K-step use
    every = {"tape1", "tape", "uncontrolled", "distributed", "night", "rt"}
    for name, want in reachable.items():
        if name.endswith(".multi.all"):
            assert want == every, name
        if name.endswith(".multi.log"):
            assert want == every | {"f32", "f64"}, name


def test_every_launch_of_every_case_takes_the_instance_the_case_is_for(cases):
    for c in cases:
        launches = c.launches()
        assert launches and {si.use_of(ln) for ln in launches} == set(c.uses), c.id
        for ln in launches:
            name, grid = ln.instance(c.num_envs)
            assert name == c.instance, f"{c.id}: {ln} takes {name}"
            assert (ln.n_evs, ln.real_time, ln.log_data, si.DEGS[ln.deg]) == (c.n_evs, c.real_time, c.log_data, c.deg), c.id


def test_batch_sizes_give_whole_workgroups_and_a_partly_filled_last_one(cases):
    """grid >= 3 with E % (envs per workgroup) != 0: whole workgroups plus a partly filled last one, the place where `env_ok` matters.
    A group of four wavefronts is a workgroup of its own (one env per workgroup: no workgroup can be partly filled), so there only
    grid >= 3 can hold."""
    for c in cases:
        epb = si.K_BLOCK // c.lanes
        assert c.instance.startswith(f"G{c.lanes}") and si.K_BLOCK % c.lanes == 0, c.id
        for ln in c.launches():
            grid = ln.instance(c.num_envs)[1]
            assert grid == -(-c.num_envs // epb), f"{c.id}: grid {grid}"  # ceil(E / (kBlock / G))
            assert grid >= 3, c.id
        if epb > 1:
            assert c.num_envs % epb != 0, c.id
    assert {c.lanes for c in cases if si.K_BLOCK // c.lanes == 1} == {256}


def test_widths_and_switches_are_spread_as_intended(cases):
    by_group = collections.defaultdict(set)
    for c in cases:
        by_group[c.instance.split(".")[0]].add(c.n_evs)
        assert not (c.norm and c.pv and not c.building), c.id  # crashes in the reference
    assert by_group == {"G1": {1}, "G2": {2}, "G4": {3}, "G8": {7}, "G16": {13}, "G32": {31}, "G64": {50, 64}, "G128": {100, 128},
                        "G256": {130, 256}, "G64w": {257, 70}}
    # surplus lanes wherever a group has a width that leaves some, and the exact powers of two of the large groups beside them
    for name in {c.instance for c in cases}:
        widths = {c.n_evs for c in cases if c.instance == name}
        group = name.split(".")[0]
        if group in ("G64", "G128", "G256"):
            assert len(widths) == 2, name
        if group == "G64w":
            assert 257 in widths, name
    for switch in ("norm", "aux", "building", "pv", "f64"):
        on = sum(getattr(c, switch) for c in cases)
        assert len(cases) // 4 < on < 3 * len(cases) // 4, switch
    assert {c.uc for c in cases} == {"lmd", "ct", "ut"}
    assert len({c.id for c in cases}) == len(cases)
    assert si.cases() == cases  # deterministic
