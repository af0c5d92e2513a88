"""Host side of the benchmark policies: the night-charging window (`fleetrl_amd.policies.night_schedule`) against the
reference's own expressions evaluated on the reference's own `env.db` (benchmarking/night_charging.py:50-73 cannot be
called in isolation -- it sits inside `run_benchmark`, which needs SB3 -- so oracle/gen_night_schedule.py evaluated the same
pandas expressions on a reference FleetEnv and stored what they gave in tests/golden/night_schedule_reference.json), and the
rule restatement of the oracle against hand-checked cases."""
import json
import os

import numpy as np
import pytest

from fleetrl_amd.policies import night_schedule
from oracle.fleet_oracle import NightChargingRule


@pytest.mark.parametrize("use_case,sched", [("lmd", "lmd_sched_single.csv"), ("ct", "ct_sched_single.csv"), ("ut", "ut_sched_single.csv")])
def test_night_schedule_matches_reference_expressions(use_case, sched, reference_inputs):
    from fleetrl_amd.prestage import build_tables_from_config
    from golden_util import GOLDEN_DIR, reference_base_config

    with open(os.path.join(GOLDEN_DIR, "night_schedule_reference.json")) as f:
        want = json.load(f)[use_case]
    ov = dict(use_case=use_case, schedule_name=sched, include_building=False, include_pv=False, deg_emp=True)
    assert want["overrides"] == ov
    target_soc, cap, eff, evse = want["target_soc"], want["init_battery_cap"], want["charging_eff"], want["evse_power"]
    max_time_needed = want["max_time_needed"]
    assert max_time_needed == target_soc * cap / eff / evse

    cfg = reference_base_config(reference_inputs)
    cfg.update(ov)
    tb = build_tables_from_config(cfg)
    got = night_schedule(tb, target_soc=target_soc, init_battery_cap=cap, charging_eff=eff, evse_power=evse)
    assert got == (want["hour"], want["minute"], int(max_time_needed))
    lh = np.asarray(want["leave_hour"])
    lm = np.asarray(want["leave_minute"])
    ph, pm, pt = NightChargingRule.parameters(lh, lm, target_soc, cap, eff, evse)
    assert (ph, pm, int(pt)) == got


def _tables(there, hour, minute):
    from types import SimpleNamespace
    return SimpleNamespace(there=np.asarray(there, dtype=np.uint8), hour=np.asarray(hour), minute=np.asarray(minute))


def test_night_schedule_small_cases():
    # one EV, leaves at 06:30; 0.85 * 60 / 0.91 / 11 = 5.09 h -> window opens at 24 + 6.5 - 5.09 = 25.4 > 24 -> 23.99
    hour = np.repeat(np.arange(24), 4)
    minute = np.tile([0, 15, 30, 45], 24)
    there = np.ones((96, 1))
    there[26:40] = 0
    assert night_schedule(_tables(there, hour, minute), target_soc=0.85, init_battery_cap=60, charging_eff=0.91, evse_power=11) == (23, 45, 5)
    # slow charger: 0.85 * 60 / 0.91 / 3.7 = 15.1 h -> 24 + 6.5 - 15.15 = 15.35 -> hour 15, 21 min -> closest quarter 15
    assert night_schedule(_tables(there, hour, minute), target_soc=0.85, init_battery_cap=60, charging_eff=0.91, evse_power=3.7) == (15, 15, 15)
    # two EVs, ID-major frame: the second one is away on its first row while the first is home on its last row --
    # the reference's shift() counts that as a departure at 00:00
    there2 = np.ones((96, 2))
    there2[26:40, 0] = 0
    there2[0:4, 1] = 0
    h, m, mx = night_schedule(_tables(there2, hour, minute), target_soc=0.85, init_battery_cap=60, charging_eff=0.91, evse_power=11)
    assert (h, m, mx) == (18, 45, 5)  # 24 + 0 - 5.09 = 18.9 -> 18 h, int(54.3) = 54 min -> 45
    with pytest.raises(ValueError):
        night_schedule(_tables(np.ones((96, 1)), hour, minute), target_soc=0.85, init_battery_cap=60, charging_eff=0.91, evse_power=11)


def test_night_rule_state_machine():
    r = NightChargingRule(23, 45, 5.09, 15, is_ct=False)
    ones, zeros = np.ones(2), np.zeros(2)
    df = np.array([0.3, 1.7])
    assert np.array_equal(r.action(90, 22, 30, 2, df), zeros)
    assert np.array_equal(r.action(95, 23, 45, 2, df), ones) and r.charging and r.charging_start == 95
    # keeps charging until MORE than int(5.09) = 5 h have passed: 20 rows later is exactly 5 h -> still on
    for row in range(96, 116):
        assert np.array_equal(r.action(row, (row // 4) % 24, (row % 4) * 15, 2, df), ones)
    assert r.charging
    assert np.array_equal(r.action(116, 5, 0, 2, df), ones) and not r.charging  # 5.25 h: this step still charges, then off
    assert np.array_equal(r.action(117, 5, 15, 2, df), zeros)
    # the reference's clock test is not lexicographic: 23:30 does not open a 23:45 window, 23:45 does
    assert np.array_equal(r.action(190, 23, 30, 2, df), zeros)
    # caretaker lunch rows use the distributed rule and leave the state alone
    c = NightChargingRule(1, 30, 3.2, 15, is_ct=True)
    assert np.array_equal(c.action(50, 12, 30, 2, df), np.array([0.3, 1.0])) and not c.charging
    # hour >= 1 and minute >= 30 holds on many rows of the day (the reference's quirk): 16:45 opens the window
    assert np.array_equal(c.action(67, 16, 45, 2, df), ones) and c.charging_start == 67


@pytest.mark.parametrize("use_case", ["lmd", "ct", "ut"])
def test_night_rule_reproduces_the_reference_harness_action_for_action(use_case):
    """The oracle's restatement of the night-charging loop against the loop itself: `tests/golden/night_harness_*.npz` holds
    the clock, the table row, `get_dist_factor()` and the action vector of EVERY step the reference's unmodified
    `NightCharging.run_benchmark` took over three 72 h (ut: two 48 h) episodes (oracle/gen_night_harness.py; SB3's two entry
    points stood in for, in that process only).  Covers the non-lexicographic window test, `charging` surviving episode
    resets, the `> int(max_time_needed)` close, and the caretaker's lunch rows."""
    import os

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"night_harness_{use_case}.npz"))
    ch, cm, tmax = NightChargingRule.parameters(g["leave_hour"], g["leave_minute"], float(g["target_soc"]), float(g["cap"]),
                                                float(g["eff"]), float(g["evse"]))
    rule = NightChargingRule(ch, cm, tmax, int(g["minutes_per_step"]), is_ct=bool(g["is_ct"]))
    n = g["actions"].shape[1]
    assert len(g["row"]) >= 2 * int(g["episode_steps"])  # more than one episode: the loop state crosses a reset
    assert (np.diff(g["row"]) < 0).any()  # static start rows: the clock jumps back at every reset
    for k in range(len(g["row"])):
        a = rule.action(int(g["row"][k]), int(g["hour"][k]), int(g["minute"][k]), n, g["dist_factor"][k])
        np.testing.assert_array_equal(a, g["actions"][k], err_msg=f"step {k} at {g['hour'][k]}:{g['minute'][k]:02d}")
    assert (g["actions"] == 1).any() and (g["actions"] == 0).any()
    if use_case == "ct":
        part = (g["actions"] > 0) & (g["actions"] < 1)
        assert part.any() and set(g["hour"][part.any(axis=1)]) <= {11, 12, 13, 14}
