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


# ---- the adversarial families the GPU suite plans (tests/test_lp_plan_gpu.py) -------------------------------------------------
def _params(use_case, **kw):
    """What `instances_of` reads of a FleetParams, for the bench configuration of a use case."""
    from types import SimpleNamespace

    p = dict(include_building=1, include_pv=1, fixed_markup=10.0, variable_multiplier=1.5, feed_in_deduction=0.25,
             evse_power=M.EVSE_KW[use_case], init_battery_cap={"ct": 16.7, "lmd": 60.0}[use_case], charging_eff=0.91,
             discharging_eff=0.91, dt=0.25, target_soc=0.85, grid_connection=M.grid_kw(use_case))
    p.update(kw)
    return SimpleNamespace(**p)


_TABLES = {}


def _tables(use_case, N):
    if (use_case, N) not in _TABLES:
        _TABLES[use_case, N] = M.adversarial_tables(use_case, N, P=M.EVSE_KW[use_case], grid=M.grid_kw(use_case))
    return _TABLES[use_case, N]


def _family_instances(family, use_case, N, H, lanes, seed):
    rng = np.random.default_rng([seed, N, H])
    tables = _tables(use_case, N)
    E = 3
    starts = np.array([M.block_start(family, k) + int(rng.integers(0, 96)) for k in rng.integers(0, 6, size=E)])
    assert all(M.family_of_row(t) == family == M.family_of_row(t + H - 1) for t in starts)
    insts = M.instances_of(tables, _params(use_case), starts, rng.uniform(-0.05, 1.0, size=(E, N)), H)
    keys = sorted(insts)
    return [insts[keys[i]] for i in rng.choice(len(keys), size=min(lanes, len(keys)), replace=False)]


@pytest.mark.parametrize("family", M.FAMILIES)
def test_adversarial_family_numpy_solver_trajectory_and_tape(family):
    """On every family, at 1, 3 and 50 EVs and whole horizons of 192 and 95 rows: the NumPy solver equals linprog, the relaxed
    cost of its trajectory is its bound, and the realised tape is feasible and keeps the trajectory.  (Measured on these 84
    instances: NumPy against HiGHS within 4.3e-15 of max(1, |bound|), the trajectory identity within 1.9e-14.)"""
    worst = [0.0, 0.0]
    for use_case, N, H in (("ct", 1, 192), ("lmd", 3, 95), ("lmd", 50, 192)):
        for inst in _family_instances(family, use_case, N, H, lanes=4, seed=7):
            want, _ = M.solve_scipy(inst)
            got, soc = M.solve_numpy(inst)
            assert got == pytest.approx(want, rel=1e-9, abs=1e-9)
            traj = M.relaxed_cost_of_trajectory(inst, soc)
            assert traj == pytest.approx(got, rel=1e-9, abs=1e-9)
            a, cost = M.realise(inst, soc)
            np.testing.assert_allclose(M.check_tape(inst, a), soc, atol=1e-12)
            assert cost >= got - 1e-9
            if family == "gap_zero":
                assert cost == pytest.approx(got, rel=1e-9, abs=1e-9)
            worst = [max(worst[0], abs(got - want) / max(1, abs(want))), max(worst[1], abs(traj - got) / max(1, abs(got)))]
    print(f"{family}: numpy vs HiGHS {worst[0]:.2e}, trajectory identity {worst[1]:.2e}")


def test_trajectory_cost_exceeds_the_bound_off_the_optimum():
    """`relaxed_cost_of_trajectory` is what makes a feasible but dearer plan visible: charging one row earlier than the cheapest
    row costs the price difference."""
    inst = _base(6, there=np.array([1, 1, 1, 1, 0, 0], bool), price=np.array([0.3, 0.1, 0.2, 0.4, 0.0, 0.0]), tariff=np.zeros(6))
    bound, soc = M.solve_numpy(inst)
    assert M.relaxed_cost_of_trajectory(inst, soc) == pytest.approx(bound, rel=1e-12)
    dearer = np.array([0.5, 0.55, 0.8, 0.8, 0.0, 0.0, 0.0])  # 0.05 on the 0.3 row instead of the 0.2 row
    assert M.relaxed_cost_of_trajectory(inst, dearer) == pytest.approx(bound + 0.25 * 10 * 0.2 * (0.3 - 0.2), rel=1e-12)
    with pytest.raises(AssertionError):
        M.relaxed_cost_of_trajectory(inst, np.array([0.5, 0.8, 0.8, 0.8, 0.0, 0.0, 0.0]))  # 0.3 in one row: more than full power


def test_row_cost_has_at_most_four_pieces():
    """The kernel allows FLEET_LP_MAX_PIECES = 5 (six candidate points); the hull never has more than four pieces, and only the
    G < s < (P + G) / 2 rows have four.

    The image (delta, cost) of the polygon is linear on x <= s and on x >= s, so the hull is the lower hull of the images of two
    convex polygons that share the edge x = s, and a vertex of it lies on the lower chain of every polygon it belongs to.
      * No bend (price <= 0, s = 0 or s >= P): one polygon (0,0), (min(P,G),0), [corner], (0,P), whose ends in delta, (0,P) and
        (min(P,G),0), are opposite vertices: a lower chain of at most 2 pieces.
      * 0 < s < G < P, the six-point case: x <= s is the quadrilateral (0,0), (s,0), (s,P-s), (0,P) with the ends (0,P), (s,0)
        opposite, so (0,0) and (s,P-s) lie on opposite chains and only one of them is on the lower one; x >= s is (s,0), (G,0),
        corner, (s,P-s) with the ends (s,P-s), (G,0) opposite, so only one of (s,0) and the corner is: 4 points, 3 pieces.
      * s < P <= G: the same with the triangle (s,0), (P,0), (s,P-s): 3 pieces.
      * G < s < (P + G) / 2: x <= s is the pentagon (0,0), (G,0), (s,s-G), (s,P-s), (0,P) with the ends (0,P), (G,0): its chains
        have 2 and 3 pieces; x >= s is the triangle (s,P-s), corner, (s,s-G), which can put the corner between them: (0,P),
        (s,P-s), corner, (s,s-G), (G,0), 4 pieces (constructed below).
      * s >= (P + G) / 2: x <= s holds the whole polygon: 2 pieces.
    The search below is the check of that argument, not a substitute for it."""
    rng = np.random.default_rng(5)
    seen = {}
    for _ in range(20000):
        P = 10.0
        G = rng.uniform(-0.2 * P, 1.5 * P)
        s = rng.choice([0.0, rng.uniform(0, 1.3 * P)])
        inst = dict(price=[rng.normal(0.05, 0.1)], tariff=[rng.normal(0.05, 0.2)], pv=[s], N=1, P=P, dt=0.25, cap=10.0,
                    eta_c=rng.uniform(0.5, 1.0), eta_d=rng.uniform(0.5, 1.0))
        Gc = max(G, 0.0)
        m = len(M.row_cost(inst, 0, Gc)[0]) - 1
        seen[m] = seen.get(m, 0) + 1
        assert m <= 4
        if m == 4:
            assert inst["price"][0] > 0 and Gc < s < 0.5 * (P + Gc)
    assert set(seen) == {1, 2, 3, 4}, seen
    # four pieces by construction: G = 2 < s = 4 < (P + G) / 2 = 6, selling pays more than buying
    inst = dict(price=[0.1], tariff=[0.3], pv=[4.0], N=1, P=10.0, dt=0.25, cap=10.0, eta_c=0.9, eta_d=1.0)
    bx, by = M.row_cost(inst, 0, 2.0)
    k = 0.25 / 10.0
    np.testing.assert_allclose(bx, np.array([-10.0, 0.9 * 4 - 6, 0.9 * 6 - 4, 0.9 * 4 - 2, 0.9 * 2]) * k, atol=1e-15)
    np.testing.assert_allclose(by, np.array([-3.0, -1.8, 0.2 - 1.2, -0.6, 0.0]) * 0.25, atol=1e-15)


def test_adversarial_tables_keep_the_schedule_and_replace_the_series():
    from fleetrl_amd.synth import synth_tables

    t = _tables("ct", 3)
    base = synth_tables("ct", 3, seed=1234, include_building=True, include_pv=True)
    for col in ("there", "time_left", "consumption", "hour", "minute", "weekday", "dates"):
        assert np.array_equal(getattr(t, col), getattr(base, col)), col
    assert t.soc_on_return.shape == base.soc_on_return.shape and t.soc_on_return.dtype == np.float64
    r = slice(M.block_start("hourly"), M.block_start("hourly") + M.BLOCK)
    assert np.all(t.delu[r].reshape(-1, 4) == t.delu[r].reshape(-1, 4)[:, :1]) and not t.pv[r].any()
    r = slice(M.block_start("negative", 2), M.block_start("negative", 2) + M.BLOCK)
    price = (t.delu[r] + 10.0) * 1.5 / 1000
    assert (price == 0).any() and (price < 0).any() and (price > 0).any()
    assert (t.delu[r] / 1000.0 + 10.0 / 1000 == 0).sum() == (price == 0).sum()  # the library's order of the same factors
    r = slice(M.block_start("returns"), M.block_start("returns") + M.BLOCK)
    assert t.soc_on_return[r].min() < 0 and t.soc_on_return[r].max() > 0.85
    r = slice(M.block_start("gap_zero", 1), M.block_start("gap_zero", 1) + M.BLOCK)
    price, tar = (t.delu[r] + 10.0) * 1.5 / 1000, t.tariff[r] * 0.75 / 1000
    assert np.all(tar * 0.91 <= price / 0.91) and not t.pv[r].any() and (4.6 * 2.5 - t.load[r] < 4.6).any()


def test_the_gpu_suites_cases_cover_every_category():
    """The instance set of tests/test_lp_plan_gpu.py::test_every_lane_matches_the_model_on_adversarial_tables (the reset SOC
    replaced by 0.5), summarised by the model alone: every category the kernel branches on occurs."""
    total = None
    for E, N, H, use_case, seed in M.ADVERSARIAL_SHAPES:
        starts, fams = M.adversarial_starts(E, H, seed)
        assert all(M.family_of_row(t) == f == M.family_of_row(t + H - 1) for t, f in zip(starts, fams))
        insts = M.instances_of(_tables(use_case, N), _params(use_case), starts, np.full((E, N), 0.5), H)
        cov = M.coverage(insts)
        assert cov["lanes"] == E * N
        if N >= 64:
            assert cov["rows"]["G<P"] and cov["rows"]["s>G"] and cov["pieces"].get(4), (N, cov)
        total = M.merge_coverage(total, cov)
    M.assert_covered(total)
    assert total["whole_horizon_session"] and max(total["pieces"]) == 4
