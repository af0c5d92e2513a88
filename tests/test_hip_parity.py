"""HIP product (libfleet_hip.so through the C ABI) against the golden traces from the unmodified reference and,
at larger batch sizes, against the CPU oracle on seeded inputs.  Needs a real MI355X (-m gpu).

Bar: indices / done flags / hours_left bit-exact; float32 observations bit-exact in practice (asserted at 1e-5
relative, the north-star tolerance, and the exact-match fraction is reported); float64 SOC / SoH / reward / cashflow
within 1e-9 relative (north star: 1e-5).
"""
import numpy as np
import pytest

from golden_util import TRACE_NAMES, load_trace, params_for, replay

pytestmark = pytest.mark.gpu


def _batch(g, num_envs=None):
    from fleetrl_amd.batch import FleetBatch

    return FleetBatch(params_for(g, num_envs=num_envs), g.tables, g.time_feat)


@pytest.mark.parametrize("name", TRACE_NAMES)
def test_hip_matches_reference_trace(name):
    g = load_trace(name)
    eng = _batch(g)
    assert eng.obs_dim == int(g.sc_obs_dim)
    worst = replay(g, eng, float_rtol=1e-9, obs_exact=False)
    frac = worst["obs_words_exact"] / max(worst["obs_words"], 1)
    print(name, worst, f"float32 observation words identical to the reference's: {100 * frac:.4f} %")
    assert worst["obs"] <= 1e-5 and worst["reward"] < 1e-9 and worst["soc"] < 1e-9 and worst["soh"] < 1e-9
    # the auxiliary slots are computed per lane with a reciprocal instead of two divisions (fleet_obs.h write_obs_ev): they are
    # tolerance-exact, not bit-exact -- a word may differ in its last bit when the float64 value sits on a float32 rounding boundary.
    # Measured (profiles/r05_obs_words_identical.txt): 100 % on 15 of the 17 traces, 99.996 % and 99.985 % on the other two
    assert frac >= 0.9998, frac


@pytest.mark.parametrize("name", ["ct5_both_rainflow", "lmd5_price_linear"])
def test_hip_batch_of_replicated_traces(name):
    """More envs than golden traces (several groups per wavefront, a partly filled last workgroup): env i replays
    golden env i % E_golden; every replica must reproduce the reference."""
    g = load_trace(name)
    eng = _batch(g, num_envs=77)
    replay(g, eng, float_rtol=1e-9, obs_exact=False)
