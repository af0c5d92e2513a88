"""The parameter sets of oracle/param_sets.py cover the scalar block: every float field of `FleetParams` that a config key can move
is off its default in at least one set, the twins the defaults make equal are unequal, and every set has its golden trace.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from fleetrl_amd import _capi
from fleetrl_amd.config import resolve_config
from fleetrl_amd.params import make_params
from golden_util import RT_TRACE_NAMES, TRACE_NAMES, load_trace, params_for
from oracle.param_sets import PARAM_SETS

# float fields no config scalar moves on its own:
#  - sized from the fleet type and the tables (evse_power, batt_cap_nominal, init_battery_cap, grid_connection and the table extrema;
#    tests/test_oracle_golden.py pins them to the reference per fleet type).  So the twins evse_power / obc_max_power are separated
#    from the on-board charger's side only: obc_max_power goes below the EVSE power of the fleet (3.7 < 4.6 kW, 11 < 22 kW);
#  - fixed by the reference's code (eps, max_laxity);
#  - init_soh: the rainflow model is refused off 1.0 (`validate_supported`, fleetrl_amd/params.py, "rainflow/SEI degradation with
#    init_soh != 1.0"; tests/test_host_logic.py test_unsupported_flag_combinations_are_rejected), and the q7 traces vary it under
#    the linear model
NOT_A_CONFIG_SCALAR = {"evse_power", "batt_cap_nominal", "init_battery_cap", "grid_connection", "max_time_left", "min_tariff",
                       "max_building", "max_pv", "max_laxity", "max_evse", "max_grid", "eps", "init_soh"}


def _params(overrides):
    import step_instances as si
    from fleetrl_amd.synth import synth_tables

    case = si.Case("", (), 0, 3, 2, "ct", "rainflow", False, False, True, True, True, True, False, 0)
    cfg = si.config_of(case)
    cfg.update(overrides)
    rc = resolve_config(cfg)
    if rc.minutes not in _params.tables:
        _params.tables[rc.minutes] = synth_tables("ct", 3, seed=1, minutes=rc.minutes)
    return make_params(rc, _params.tables[rc.minutes], 2)


_params.tables = {}


def unvaried_float_fields(sets):
    base = _params({})
    moved = set()
    for ov in sets.values():
        p = _params(ov)
        moved |= {f for f, t in _capi.FleetParams._fields_ if t is C.c_double and getattr(p, f) != getattr(base, f)}
    return {f for f, t in _capi.FleetParams._fields_ if t is C.c_double} - moved - NOT_A_CONFIG_SCALAR


def test_every_float_field_is_off_its_default_in_some_set():
    assert unvaried_float_fields(PARAM_SETS) == set()
    assert not NOT_A_CONFIG_SCALAR - {f for f, t in _capi.FleetParams._fields_ if t is C.c_double}, "stale exemption"


def test_the_check_sees_a_field_put_back_to_its_default():
    sets = {k: {q: v for q, v in ov.items() if q != "temperature"} for k, ov in PARAM_SETS.items()}
    assert unvaried_float_fields(sets) == {"temperature"}
    sets = {k: {q: v for q, v in ov.items() if q != "discharging_eff"} for k, ov in PARAM_SETS.items()}
    assert unvaried_float_fields(sets) == {"discharging_eff"}


@pytest.mark.parametrize("name", ["offdef", "offdef_norm"])
def test_twins_are_unequal_and_no_value_repeats(name):
    ov = PARAM_SETS[name]
    assert ov["charging_eff"] != ov["discharging_eff"] and ov["price_lookahead"] != ov["bl_pv_lookahead"]
    assert ov["penalty_invalid_action"] != ov["clip_overcharging"]
    vals = [abs(float(v)) for v in ov.values()]
    assert len(set(vals)) == len(vals), "two parameters share a value: a swap of the two would change no number"
    p = _params(ov)
    assert p.obc_max_power < p.evse_power or name == "offdef_norm"  # (sized for the utility EVSE, 22 kW, in the norm set)
    for k in ("price_lookahead", "bl_pv_lookahead", "charging_eff", "discharging_eff", "obc_max_power", "temperature"):
        assert getattr(p, k) == ov[k], k


def test_every_set_has_its_golden_trace():
    """The oracle is pinned to the reference under a set by the trace(s) made from it: the trace's stored config holds the set."""
    import json

    for name, ov in PARAM_SETS.items():
        hits = [n for n in TRACE_NAMES if n.endswith("_" + name) or (name == "offdef_norm" and n.endswith("norm_linear_offdef"))]
        assert hits, name
        for n in hits:
            g = load_trace(n)
            if name == "offdef" and "norm" in n:
                continue
            assert all(g.cfg[k] == v for k, v in ov.items()), (name, n)
            p = params_for(g)
            assert p.steps_per_hour == g.cfg.get("time_steps_per_hour", 4) and g.ep_steps == p.episode_steps
    assert "ct3_both_rainflow_offdef" in RT_TRACE_NAMES
    g = load_trace("ut3_both_rainflow_look12x14")
    assert int(g.sc_obs_dim) == 7 * g.N + 66


def test_coarse_step_traces_record_no_degradation():
    """What the reference did at 30 / 60 minutes with degradation configured: nothing (no row is 14:45)."""
    for n in ("ct3_both_rainflow_min30", "lmd3_both_linear_min60"):
        g = load_trace(n)
        assert not (np.asarray(g.tables.minute) == 45).any()
        assert (g.soh == 1.0).all() and not g.fd_cyc.any() and not g.sei_l.any()
    assert (load_trace("ct3_both_rainflow_min30").rf_len == 1).all()


def test_gpu_cases_reach_every_lane_group_and_use_under_every_set():
    """The case list of tests/test_param_space_gpu.py through the planner (no GPU needed): under every set a case on an instance of
    each lane group G = 8 ... 256 -- not the "G64w" instances the planner gives real_time and the data log beyond one wavefront --
    and every use; the 66-float tail on G = 64, 128 and 256."""
    import test_param_space_gpu as T

    cases = T.step_cases()
    for pset in T.STEP_SETS:
        mine = [c for s, c in cases if s == pset]
        groups = {c.instance.split(".")[0] for c in mine}
        assert groups == {"G8", "G16", "G32", "G64", "G128", "G256"}, (pset, groups)
        uses = {u for c in mine for u in c.uses}
        assert uses >= {"f32", "f64", "tape", "tape1", "rt", "uncontrolled", "distributed", "night"}, (pset, uses)
        assert any(c.log_data for c in mine) and any(c.real_time for c in mine)
        assert {c.f64 for c in mine} == {False, True}
    assert set(T.STEP_SETS) == {"offdef", "offdef_norm", "look0", "look12x14"} and set(T.STEP_SETS) < set(PARAM_SETS)
    rt_widths = {c.n_evs for s, c in cases if c.real_time}
    assert len(rt_widths) > 1 and max(rt_widths) <= 64
