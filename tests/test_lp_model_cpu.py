"""The linear-optimisation benchmark's model (tests/lp_model.py) on the CPU: the slow NumPy solver of the
relaxation against scipy's HiGHS, hand-worked cases, and decision 2's realisation against the binary model."""
import numpy as np
import pytest

import lp_model as M


def _base(H, **kw):
    inst = dict(there=np.ones(H, bool), sor=np.zeros(H), price=np.full(H, 0.1), tariff=np.full(H, 0.05), pv=np.zeros(H),
                load=np.zeros(H), P=10.0, cap=10.0, eta_c=1.0, eta_d=1.0, dt=0.25, target=0.8, p_trafo=100.0, N=1, soc0=0.5)
    inst.update(kw)
    return inst


@pytest.mark.parametrize("seed", range(12))
def test_numpy_solver_equals_linprog(seed):
    rng = np.random.default_rng(seed)
    inst = M.random_instance(rng, int(rng.integers(6, 40)), pv=bool(seed % 2))
    want, _ = M.solve_scipy(inst)
    got, soc = M.solve_numpy(inst)
    assert got == pytest.approx(want, rel=1e-9, abs=1e-9)
    a, _ = M.realise(inst, soc)
    np.testing.assert_allclose(M.check_tape(inst, a), soc, atol=1e-12)


def test_departure_target_is_met_at_the_cheapest_rows():
    # k = P dt / cap = 0.25 per full-power row; 0.5 -> 0.8 needs 1.2 rows of charge before the departure row 3
    inst = _base(6, there=np.array([1, 1, 1, 1, 0, 0], bool), price=np.array([0.3, 0.1, 0.2, 0.4, 0.0, 0.0]), tariff=np.zeros(6))
    bound, soc = M.solve_numpy(inst)
    # row 1 full (0.25 SOC at 0.1 EUR/kWh * 10 kW * 0.25 h), the remaining 0.05 SOC on row 2 (0.2 of full power at 0.2 EUR/kWh)
    assert bound == pytest.approx(0.25 * 0.1 * 10 + 0.25 * 0.2 * 10 * 0.2, rel=1e-12)
    np.testing.assert_allclose(soc[:5], [0.5, 0.5, 0.75, 0.8, 0.0], atol=1e-12)
    assert M.solve_scipy(inst)[0] == pytest.approx(bound, rel=1e-9)


def test_arrival_fixes_the_soc_on_return():
    there = np.array([0, 0, 1, 1, 1, 1], bool)
    inst = _base(6, there=there, sor=np.array([0, 0, 0.3, 0.3, 0.3, 0.3]), price=np.full(6, 0.1), tariff=np.full(6, -0.01))
    bound, soc = M.solve_numpy(inst)
    assert soc[2] == 0.3 and bound == pytest.approx(0.0, abs=1e-15)  # open end, nothing pays: stay put
    np.testing.assert_allclose(soc, [0, 0, 0.3, 0.3, 0.3, 0.3, 0.3], atol=1e-15)


def test_unreachable_target_is_lowered_and_flagged():
    inst = _base(4, there=np.array([1, 1, 1, 0], bool), soc0=0.1)  # two charging rows reach 0.6 < 0.8
    start, tau, bits = M.sessions(inst)
    assert tau == {2: pytest.approx(0.6)} and bits & M.UNREACHABLE
    bound, soc = M.solve_numpy(inst)
    assert bound == pytest.approx(2 * 0.25 * 0.1 * 10, rel=1e-12)
    assert M.solve_scipy(inst)[0] == pytest.approx(bound, rel=1e-9)
    inst2 = _base(4, there=np.array([0, 1, 1, 0], bool), sor=np.array([0, -0.2, -0.2, 0]))
    assert M.sessions(inst2)[2] & M.NEG_RETURN and M.sessions(inst2)[1][2] == pytest.approx(0.25)


def test_grid_limit_binds():
    # 4 kW of headroom: a full-power row moves the SOC by 0.1 only
    inst = _base(5, there=np.array([1, 1, 1, 1, 0], bool), soc0=0.5, load=np.full(5, 6.0), p_trafo=10.0)
    bound, soc = M.solve_numpy(inst)
    np.testing.assert_allclose(soc[:4], [0.5, 0.6, 0.7, 0.8], atol=1e-12)
    assert bound == pytest.approx(3 * 0.25 * 0.1 * 4, rel=1e-12)
    assert M.solve_scipy(inst)[0] == pytest.approx(bound, rel=1e-9)


def test_pv_row_charges_for_free_and_the_relaxation_can_undercut_the_milp():
    # PV covers 4 kW on row 0 and the SOC must stay at the target: the relaxation charges 4 kW from PV and discharges 4 kW in
    # the same row (0.1 EUR/kWh * 4 kW * 0.25 h earned), which the binary b forbids
    inst = _base(3, there=np.array([1, 1, 0], bool), soc0=0.8, pv=np.array([4.0, 0.0, 0.0]), price=np.full(3, 0.2),
                 tariff=np.full(3, 0.1), target=0.8)
    bound, soc = M.solve_numpy(inst)
    lp, _ = M.solve_scipy(inst)
    ip, _ = M.solve_scipy(inst, binary=True)
    a, cost = M.realise(inst, soc)
    M.check_tape(inst, a)
    assert bound == pytest.approx(lp, rel=1e-9)
    assert soc[1] == pytest.approx(0.8) and bound == pytest.approx(-0.1, rel=1e-12)
    assert ip == pytest.approx(0.0, abs=1e-12) and cost == 0.0


@pytest.mark.parametrize("seed", range(8))
def test_relaxation_equals_milp_when_the_gap_condition_holds(seed):
    rng = np.random.default_rng(100 + seed)
    inst = M.random_instance(rng, int(rng.integers(6, 24)), pv=False, gap_zero=True)
    lp, _ = M.solve_scipy(inst)
    ip, _ = M.solve_scipy(inst, binary=True)
    bound, soc = M.solve_numpy(inst)
    a, cost = M.realise(inst, soc)
    assert ip == pytest.approx(lp, rel=1e-8, abs=1e-9)
    assert cost == pytest.approx(bound, rel=1e-9, abs=1e-12)


@pytest.mark.parametrize("seed", range(8))
def test_realised_tape_is_feasible_and_brackets_the_milp(seed):
    rng = np.random.default_rng(200 + seed)
    inst = M.random_instance(rng, int(rng.integers(6, 24)), pv=True)
    bound, soc = M.solve_numpy(inst)
    a, cost = M.realise(inst, soc)
    np.testing.assert_allclose(M.check_tape(inst, a), soc, atol=1e-12)
    ip, _ = M.solve_scipy(inst, binary=True)
    assert bound <= ip + 1e-9 and ip <= cost + 1e-9
