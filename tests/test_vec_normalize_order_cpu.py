"""The summation scheme of fleet_norm.hip, restated in NumPy (`vecnorm_model.device_order_moments`), against the two-pass model
that the GPU tests compare the device with -- on the very inputs of tests/test_vec_normalize_shapes_gpu.py.  No GPU.

What this proves: the scheme on its own (shift by row 0, slabs of 64 rows, four waves, fixed combine orders, the 64-lane tree of
the returns, `m2 > 0 ? m2 / n : 0`) stays within ONE QUARTER of every `check_stats` tolerance, so the tolerances the device is held
to are attainable, with room for what the restatement does not reproduce (the device's square root).  The device is compared with
the model, never bit-compared with the restatement.

Measured worst error over tolerance (1.0 = the `check_stats` limit, 0.25 = the limit here), this file's cases on x86-64 NumPy:
  hostile columns   E = 5: var 5.5e-6, mean 9.5e-5   E = 65: var 7.0e-5, mean 4.9e-4   E = 4161: var 9.2e-3, mean 6.1e-3
                    E = 65536: var 0.034, mean 0.011 -- but for ONE column at E = 65536, 0.5 +- 1e-3 with row 0 = 1e4, at 0.27:
                    its bound is derived from the shift in test_hostile_columns_within_a_quarter_of_the_tolerances
  ragged shapes     var 4.3e-5, mean 1.3e-4 (E = 16447 and E = 3)
  returns           var 5.6e-6, mean 1.1e-4
"""
from types import SimpleNamespace

import numpy as np
import pytest

from vecnorm_cases import (HOSTILE_COLUMNS, HOSTILE_D, HOSTILE_E, RAGGED_E, hostile_batch, hostile_dones, hostile_rewards, hostile_start,
                           ragged_step)
from vecnorm_model import (VecNormModel, batch_moments, check_stats, device_order_moments, device_order_return_moments,
                           stats_ratios)

QUARTER = 0.25
OUTLIER_COLUMN = HOSTILE_COLUMNS.index("0.5 +- 1e-3, row 0 = 1e4")


def pair(E, D, **kw):
    return VecNormModel(E, D, device_order=True, **kw), VecNormModel(E, D, **kw)


def step_both(order, model, *args):
    order.step(*args, outputs=False)
    model.step(*args, outputs=False)


def test_the_restatement_is_exact_where_the_sums_are():
    """Small integers: every sum is exact in any order, so the restatement equals the two-pass moments to the last few roundings
    -- at a ragged last slab, a slab count off the multiples of 4 and 64, and a row 0 far from the rest."""
    rng = np.random.default_rng(0)
    for E in (1, 2, 3, 5, 64, 65, 300, 4161):
        X = rng.integers(-50, 50, size=(E, 3)).astype(np.float64)
        X[0, 1] = 4096.0
        for got, want, K in ((device_order_moments(X), batch_moments(X), X[0]),
                             (device_order_return_moments(X[:, 1]), batch_moments(X[:, 1]), X[0, 1])):
            assert got[2] == want[2] == E
            # (S1, S2 and S1^2 are exact.  K + S1 / n rounds twice at the size of K; S1^2 / n rounds once at up to (n + 1) times
            # the size of m2 = n var, the row-0 outlier's price; the two-pass variance is good to a few ulps)
            assert np.all(np.abs(got[0] - want[0]) <= 4 * np.spacing(np.abs(K) + np.abs(want[0])))
            np.testing.assert_allclose(got[1], want[1], rtol=(E + 1) * 2.0 ** -53 + 4 * 2.0 ** -52, atol=0)


def test_every_row_and_slab_is_summed_once():
    """A one in a single row, zeros elsewhere (row 0 is zero: no shift): the mean is 1 / E whichever row, slab, wave or lane holds it."""
    for E in (2, 5, 65, 300, 4161):
        for r in sorted({1, E // 2, E - 2, E - 1} - {0}):
            X = np.zeros((E, 2))
            X[r, 0] = 1.0
            X[r, 1] = -3.0
            m, v, _ = device_order_moments(X)
            assert m[0] == 1.0 / E and m[1] == -3.0 / E, (E, r)
            rm, rv, _ = device_order_return_moments(X[:, 0])
            assert rm == 1.0 / E, (E, r)
            np.testing.assert_allclose([v[0], rv], [(1 - 1 / E) / E] * 2, rtol=1e-14)


def test_a_constant_batch_has_variance_exactly_zero():
    for E in HOSTILE_E:
        m, v, _ = device_order_moments(hostile_batch(E, 0)[:, :1])
        assert v[0] == 0.0 and m[0] == hostile_batch(E, 0)[0, 0]
        m, v, _ = device_order_return_moments(np.full(E, 0.1))
        assert v == 0.0 and m == 0.1


@pytest.mark.parametrize("E", HOSTILE_E)
def test_hostile_columns_within_a_quarter_of_the_tolerances(E):
    """The eight hostile columns over a reset and five steps with dones; the finite result of the +-3e38 column included (its
    squares overflow float32, not float64).  After the constant column's start at (its value, variance 0) its running variance
    stays exactly 0.0 in both.

    One column cannot hold the quarter at E = 65536: 0.5 +- 1e-3 with row 0 = 1e4, where the shift K is the outlier itself.  Its
    bound comes from the shift: (K - mean)^2 <= n var for any sample K of the batch, so S2 and S1^2 / n are at most (n + 1) times
    m2 = n var, and relative errors d2 of S2 and d1 of S1 leave (n + 1) (d2 - 2 d1) in the variance.  Every term x - K is the same
    to 1e-7 here, so each wave of norm_finalize adds m = slabs / 4 equal partials one after the other: roundings uniform in
    +- 2^-53 of the running sum give d a standard deviation of 2^-53 sqrt(m) / 3 per wave, half that for the four waves' mean
    (the 16 rows a wave adds inside a slab contribute 1 / 64 of it).  So sigma = (n + 1) 2^-53 sqrt(5 m) / 6 -- 4.3e-11 at
    n = 65536 (m = 256), 7e-13 at n = 4161 -- and the column is held to the larger of the quarter and 3 sigma.
    Measured on the CPU, running variance: 2.74e-11 (0.63 sigma, 0.27 of `check_stats`'s 1e-10, which stays as it is for the
    device) at E = 65536, where single batches reach 3.4e-11; 3.5e-13 at E = 4161, 8e-15 at E = 65, where the quarter (2.5e-11)
    decides.  Every other column holds the quarter at every E; worst
    ratios in the module docstring."""
    order, model = pair(E, HOSTILE_D)
    for m in (order, model):
        hostile_start(m)
        m.reset(hostile_batch(E, 0))
    sigma = (E + 1) * 2.0 ** -53 * np.sqrt(5 * -(-(-(-E // 64)) // 4)) / 6
    worst = np.zeros(4)
    worst_outlier = 0.0

    def check(tag):
        nonlocal worst, worst_outlier
        st = order.get_state()
        c = OUTLIER_COLUMN
        v, mean = model.obs_rms.var[c], model.obs_rms.mean[c]
        err = abs(st.obs_rms.var[c] - v)
        worst_outlier = max(worst_outlier, err / v)
        assert err <= max(QUARTER * max(1e-10 * v, 1e-14 * (1 + mean * mean)), 3 * sigma * v), (tag, err / v, sigma)
        st.obs_rms.var[c] = v  # (checked above; everything else, this column's mean included, to the quarter)
        worst = np.maximum(worst, stats_ratios(st, model))
        check_stats(SimpleNamespace(get_state=lambda: st), model, tag, fraction=QUARTER)

    check("reset")
    for k in range(1, 6):
        step_both(order, model, hostile_batch(E, k), hostile_rewards(E, k), hostile_dones(E, k))
        check(k)
        for m in (order, model):
            assert m.obs_rms.var[0] == 0.0 and m.obs_rms.mean[0] == hostile_batch(E, 0)[0, 0]
            assert np.all(np.isfinite(m.obs_rms.mean)) and np.all(np.isfinite(m.obs_rms.var))
    print(f"hostile E={E}: outlier column's worst relative variance error {worst_outlier:.2e} (sigma {sigma:.2e})")
    print(f"hostile E={E}: worst error / tolerance  mean {worst[0]:.1e}  var {worst[1]:.1e}  ret mean {worst[2]:.1e}  ret var {worst[3]:.1e}")


def test_hostile_returns_within_a_quarter_of_the_tolerances():
    """gamma = 1 with rewards near 1e6 over 50 steps without a done (returns near 5e7, their spread a few thousand); gamma = 0;
    a step where every env is done."""
    worst = np.zeros(4)
    for E in HOSTILE_E:
        order, model = pair(E, 1, gamma=1.0, norm_obs=False)
        for k in range(50):
            step_both(order, model, np.zeros((E, 1), np.float32), hostile_rewards(E, k, 1e3, 1e6), np.zeros(E, bool))
            worst = np.maximum(worst, stats_ratios(order.get_state(), model))
            check_stats(order, model, (E, k), fraction=QUARTER)
        order, model = pair(E, 1, gamma=0.0, norm_obs=False)
        for k in range(6):
            step_both(order, model, np.zeros((E, 1), np.float32), hostile_rewards(E, k), hostile_dones(E, k))
            worst = np.maximum(worst, stats_ratios(order.get_state(), model))
            check_stats(order, model, (E, k), fraction=QUARTER)
        order, model = pair(E, 1, norm_obs=False)
        for k in range(6):
            done = np.ones(E, bool) if k == 2 else hostile_dones(E, k)
            step_both(order, model, np.zeros((E, 1), np.float32), hostile_rewards(E, k), done)
            worst = np.maximum(worst, stats_ratios(order.get_state(), model))
            check_stats(order, model, (E, k), fraction=QUARTER)
            assert k != 2 or not model.returns.any()
    print(f"hostile returns: worst error / tolerance  ret mean {worst[2]:.1e}  ret var {worst[3]:.1e}")


@pytest.mark.parametrize("E", RAGGED_E)
def test_ragged_shapes_within_a_quarter_of_the_tolerances(E):
    """The GPU test's shape matrix reduced to D = 3 (the columns are independent): a reset and six steps with dones."""
    D = 3
    rng = np.random.default_rng([7, E, D])
    order, model = pair(E, D)
    x = ragged_step(rng, E, D)[0]
    order.reset(x)
    model.reset(x)
    worst = np.array(stats_ratios(order.get_state(), model))
    check_stats(order, model, "reset", fraction=QUARTER)
    for k in range(6):
        obs, rew, done, _ = ragged_step(rng, E, D)
        step_both(order, model, obs, rew, done)
        worst = np.maximum(worst, stats_ratios(order.get_state(), model))
        check_stats(order, model, k, fraction=QUARTER)
    print(f"ragged E={E}: worst error / tolerance  mean {worst[0]:.1e}  var {worst[1]:.1e}  ret mean {worst[2]:.1e}  ret var {worst[3]:.1e}")
