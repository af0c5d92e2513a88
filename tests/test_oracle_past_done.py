"""Stepping an env without auto-reset past the end of its episode (the gymnasium.Env path): the CPU oracle against traces of
the unmodified reference (oracle/gen_golden.py pd).  In the reference `episode.done` stays True after the finish row
(fleet_environment.py:627-628, :702), LogDataDeg.soc_log keeps growing, and each 14:45 row past the finish runs the degradation
model on the whole log -- SoH, fd_cyc, rainflow_length and l move, and carry into the next episode (quirk Q6)."""
import numpy as np
import pytest

from golden_util import PD_RT_TRACE_NAMES, PD_TRACE_NAMES, load_pd_trace, params_for, replay_pd
from oracle.fleet_oracle import OracleBatch

CASES = [(n, False) for n in PD_TRACE_NAMES] + [(n, True) for n in PD_RT_TRACE_NAMES]


def test_the_past_done_fixtures_are_there():
    assert {"ct5_both_rainflow", "lmd3_price_linear_log"} <= set(PD_TRACE_NAMES) and "ct3_both_rainflow" in PD_RT_TRACE_NAMES


@pytest.mark.parametrize("name,rt", CASES)
def test_oracle_past_done_matches_reference(name, rt):
    g = load_pd_trace(name, rt)
    assert bool(g.rc.real_time) == rt
    # what the fixture pins: 14:45 rows past the finish (two without real_time), and a SOC log that kept growing there
    assert np.all(g.soc_log_len[:, 1] - g.soc_log_len[:, 0] >= g.seg_steps[:, 1])
    for e in range(g.E):
        rows = np.arange(g.time_idx[e, g.seg_steps[e, 0] - 1] + 1, g.time_idx[e, g.seg_steps[e, :2].sum() - 1] + 1)
        n_deg = np.count_nonzero((g.tables.hour[rows] == 14) & (g.tables.minute[rows] == 45))
        assert n_deg >= (1 if rt else 2), (e, n_deg)
    if g.rc.deg_mode == 2 and not rt:
        assert np.all(g.rf_len[:, 1] > g.rf_len[:, 0])  # the past-done evaluations counted new cycles
    for e in range(g.E):
        eng = OracleBatch(params_for(g, num_envs=1, auto_reset=False), g.tables, g.time_feat)
        worst = replay_pd(g, eng, e, float_rtol=1e-9, obs_exact=True, done_getter=lambda: eng.get("done")[0])
        assert worst["reward"] < 1e-9 and worst["soc"] < 1e-9 and worst["soh"] < 1e-12, worst


def test_oracle_raises_table_end_on_the_step_that_leaves_the_table():
    """An env stepped past done until `t + 1 > T - 1` gets FLEET_DEVERR_TABLE_END in exactly that step (the reference's
    `db.loc` lookup fails there too); every step before it is clean."""
    from fleetrl_amd import _capi

    g = load_pd_trace("ct5_both_rainflow")
    eng = OracleBatch(params_for(g, num_envs=1, auto_reset=False), g.tables, g.time_feat)
    T = g.tables.T
    eng.set_start_schedule(np.array([[T - 1 - g.ep_rows - 30]], dtype=np.int32))
    eng.reset()
    a = np.zeros((1, g.N), np.float32)
    while eng.get("time_idx")[0] < T - 1:
        eng.step(a)
        assert eng.get("error_bits")[0] == 0
    assert eng.get("done")[0] == 1
    eng.step(a)
    assert eng.get("error_bits")[0] & _capi.DEVERR_TABLE_END
