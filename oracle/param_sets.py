"""Named sets of scalar parameters away from the reference's defaults, kept in one place.

`oracle/gen_golden.py` merges them into the configurations of the golden traces that pin the CPU oracle off the
defaults (trace_*_offdef, *_look0, *_look12x14, *_min30, *_min60), and tests/test_param_space_gpu.py runs the HIP
kernels against the oracle under the same sets at the shapes the traces cannot reach.  tests/test_param_sets_cpu.py
fails when a float field of `FleetParams` keeps its default in every set.

Rules for the values: no two parameters that the defaults make equal (charging_eff / discharging_eff, price_lookahead /
bl_pv_lookahead, penalty_invalid_action / clip_overcharging, EVSE power / on-board charger power) are equal here, and no
value coincides with another parameter's value or default, so that a swapped pair always changes a number.
"""

# every scalar off its default at once; caretaker fleets (the lunch target only exists there); the on-board charger
# (3.7 kW) below the caretaker EVSE (4.6 kW), so that it is the binding power limit
OFFDEF = dict(
    price_lookahead=3, bl_pv_lookahead=6, charging_eff=0.95, discharging_eff=0.83, temperature=35.0,
    target_soc=0.8, target_soc_lunch=0.55, min_laxity=1.7, def_soc=0.4, spot_markup=7.3, spot_mul=1.3, feed_in_ded=0.1,
    price_multiplier=2.5, fully_charged_reward=1.75, penalty_invalid_action=-0.3, penalty_overcharging=-0.01,
    penalty_overloading=1.6, clip_overcharging=-0.5, obc_max_power=3.7,
)

# a second, disjoint choice for normalised observations: every normaliser constant that derives from a parameter
# (max_price, min_price, max_tariff, max_hours_needed, max_soc) moves; 11 kW on-board charger below the utility EVSE (22 kW)
OFFDEF_NORM = dict(
    price_lookahead=5, bl_pv_lookahead=2, charging_eff=0.88, discharging_eff=0.93, temperature=15.0,
    target_soc=0.75, target_soc_lunch=0.6, min_laxity=2.5, def_soc=0.45, spot_markup=12.5, spot_mul=1.2, feed_in_ded=0.35,
    price_multiplier=4.1, fully_charged_reward=0.65, penalty_invalid_action=-0.15, penalty_overcharging=-0.004,
    penalty_overloading=0.7, clip_overcharging=-0.32, obc_max_power=11.0,
)

# look-ahead edges: no look-ahead at all, and one that makes the env-level observation tail (2 (L + 1) + 2 (B + 1) + 10
# floats with load + pv + aux) 66 floats, longer than a 64-lane group
LOOK0 = dict(price_lookahead=0, bl_pv_lookahead=0)
LOOK12X14 = dict(price_lookahead=12, bl_pv_lookahead=14)

# other step lengths: the three keys are set together, as the reference expects
MIN30 = dict(freq="30T", minutes=30, time_steps_per_hour=2)
MIN60 = dict(freq="1H", minutes=60, time_steps_per_hour=1)

PARAM_SETS = {"offdef": OFFDEF, "offdef_norm": OFFDEF_NORM, "look0": LOOK0, "look12x14": LOOK12X14,
              "min30": MIN30, "min60": MIN60}
