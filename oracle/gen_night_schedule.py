#!/usr/bin/env python3
"""The night-charging window as the reference's own expressions compute it on the reference's own `env.db`
(benchmarking/night_charging.py:50-73; TEST INFRASTRUCTURE, needs the reference sources).  `run_benchmark` cannot be called in
isolation (it needs SB3), so the same pandas expressions are evaluated on a reference FleetEnv built here.

    python oracle/gen_night_schedule.py      ->  tests/golden/night_schedule_reference.json

Per use case: the departures (hour, minute of every home -> driving row), the scalars the window is derived from, and the
window itself (hour, minute, max_time_needed).  Data only."""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

CASES = (("lmd", "lmd_sched_single.csv"), ("ct", "ct_sched_single.csv"), ("ut", "ut_sched_single.csv"))


def window(use_case: str, sched: str) -> dict:
    ov = dict(use_case=use_case, schedule_name=sched, include_building=False, include_pv=False, deg_emp=True)
    env = ref_harness.make_ref_env(ov)
    df = env.db
    # night_charging.py:52-73, verbatim semantics on the reference's frame
    df_leaving_home = df[(df["Location"].shift() == "home") & (df["Location"] == "driving")]
    earliest_dep_time = df_leaving_home["date"].dt.time.min()
    earliest_dep = earliest_dep_time.hour + earliest_dep_time.minute / 60
    evse, cap = env.load_calculation.evse_max_power, env.ev_config.init_battery_cap
    target_soc, eff = env.ev_config.target_soc, env.ev_config.charging_eff
    max_time_needed = target_soc * cap / eff / evse
    starting_time = 24 + (earliest_dep - max_time_needed)
    if starting_time > 24:
        starting_time = 23.99
    minutes = np.asarray([0, 15, 30, 45])
    return {"overrides": ov, "target_soc": float(target_soc), "init_battery_cap": float(cap), "charging_eff": float(eff),
            "evse_power": float(evse), "max_time_needed": float(max_time_needed),
            "hour": int(math.modf(starting_time)[1]),
            "minute": int(minutes[np.abs(minutes - int(math.modf(starting_time)[0] * 60)).argmin()]),
            "leave_hour": [int(x) for x in df_leaving_home["date"].dt.hour.values],
            "leave_minute": [int(x) for x in df_leaving_home["date"].dt.minute.values]}


def main():
    out = {uc: window(uc, sched) for uc, sched in CASES}
    path = os.path.join(ROOT, "tests", "golden", "night_schedule_reference.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(path, {uc: (v["hour"], v["minute"], v["max_time_needed"], len(v["leave_hour"])) for uc, v in out.items()})


if __name__ == "__main__":
    main()
