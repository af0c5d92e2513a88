"""The launch planner's output, pinned: which instance of the step kernel a configuration takes and with what grid
(`fleet_step_instance`, which reports what `fleet_describe_step` and every launcher select) is held to a recording made before the
single-step kernels learnt to skip a dead observation row (tests/golden/step_planner_pinned.json).  That skip is a run-time argument
of the launch: it must neither create an instance nor move a configuration to another one.  No GPU needed."""
import hashlib
import json
import os

import step_instances as si
from fleetrl_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_planner_pinned.json")


def _pinned():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_every_launch_of_every_case_takes_the_recorded_instance_and_grid():
    want = _pinned()["cases"]
    cases = si.cases()
    assert sorted(c.id for c in cases) == sorted(want)
    for c in cases:
        got = [[[int(x) for x in (ln.n_evs, ln.deg, ln.real_time, ln.log_data, ln.act_mode, ln.K, ln.has_done_count)],
                *ln.instance(c.num_envs)] for ln in c.launches()]
        assert got == want[c.id], c.id


def test_the_whole_sweep_of_the_planner_is_the_recorded_one():
    """Every (batch size, width, degradation model, real_time, data log, action mode, K, done_count) the reachable-set sweep of
    tests/step_instances.py visits, at a tiny and at the benchmark's batch size: names and grids, as one digest."""
    h = hashlib.sha256()
    names = set()
    n_max = 2 * int(_capi.load_library().fleet_max_evs_per_lane_group()) + 1
    for E in (7, 4096):
        for n in range(1, n_max + 1):
            for deg in range(3):
                for rt in (False, True):
                    for log in (False, True):
                        for act_mode in (_capi.ACT_F32, _capi.ACT_F64, *si.POLICIES.values()):
                            for K in (1, 2):
                                for hdc in (False, True):
                                    name, grid = _capi.step_instance(E, n, deg, rt, log, act_mode, K, hdc)
                                    names.add(name)
                                    h.update(f"{E},{n},{deg},{int(rt)},{int(log)},{act_mode},{K},{int(hdc)}:{name},{grid}\n".encode())
    assert h.hexdigest() == _pinned()["sweep_sha256"]
    assert not [n for n in names if "dead" in n]
