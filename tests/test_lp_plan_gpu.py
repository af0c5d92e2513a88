"""The linear-optimisation benchmark on the GPU (`fleet_lp_plan_dev`, fleetrl_amd/lp_benchmark.py): every (env, EV) plan
against the model restated in tests/lp_model.py (scipy HiGHS, or the NumPy solver where scipy is missing), the replayed
tape against the plan and the CPU oracle, status bits, the horizon guard, determinism and the bench-size call: on two golden
tables, and on the adversarial tables of tests/lp_model.py (grid-bound rows, prices <= 0, PV shares up to above the charger's
power, returns outside [0, target]) over ragged shapes, from live states mid-episode and at the bench size.  Needs an MI355X."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import lp_model as M
from golden_util import load_trace, params_for
from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, H = 8, 192

try:
    import scipy.optimize  # noqa: F401

    def relaxed_opt(inst):
        return M.solve_scipy(inst)[0]
except ImportError:  # never skip: the NumPy solver is exact too (tests/test_lp_model_cpu.py checks it against scipy)
    def relaxed_opt(inst):
        return M.solve_numpy(inst)[0]


def _setup(name, tables=None, log=False, seed=3, no_deg=False):
    from fleetrl_amd.batch import FleetBatch

    g = load_trace(name)
    tables = g.tables if tables is None else tables
    p = params_for(g, num_envs=E)
    p.init_soh = 1.0  # fresh batteries: the env's sticky 0.9 target at SoH <= 0.9 is not in the model (nor in the reference's)
    if log:
        p.log_data = 1
    if no_deg:  # the env's capacity shrinks with the state of health; the model's is the nominal one (as in the reference)
        p.deg_mode = _capi.DEG_NONE
    rng = np.random.default_rng(seed)
    starts = rng.integers(0, tables.T - g.ep_steps - 1, size=(1, E)).astype(np.int32)
    hip = FleetBatch(p, tables, g.time_feat)
    hip.set_start_schedule(starts)
    hip.reset()
    return g, p, tables, starts, hip


def _instances(p, tables, hip):
    """lp_model instances of every (env, EV) from the batch's live state."""
    t0, soc = hip.get("time_idx"), hip.get("soc")
    N = hip.N
    delu, tariff = np.asarray(tables.delu, float), np.asarray(tables.tariff, float)
    load = np.asarray(tables.load, float) if p.include_building else np.zeros(tables.T)
    pv = np.asarray(tables.pv, float) if p.include_pv else np.zeros(tables.T)
    out = {}
    for e in range(hip.E):
        r = slice(int(t0[e]), int(t0[e]) + H)
        for c in range(N):
            out[e, c] = dict(there=np.asarray(tables.there)[r, c] != 0, sor=np.asarray(tables.soc_on_return)[r, c],
                             price=(delu[r] + p.fixed_markup) * p.variable_multiplier / 1000,
                             tariff=tariff[r] * (1 - p.feed_in_deduction) / 1000, pv=pv[r], load=load[r], P=p.evse_power,
                             cap=p.init_battery_cap, eta_c=p.charging_eff, eta_d=p.discharging_eff, dt=p.dt, target=p.target_soc,
                             p_trafo=p.grid_connection, N=N, soc0=float(soc[e, c]))
    return out


def _check_plan(plan, insts, E_, N_, H_, gap_zero_envs=()):
    """Every lane of `plan` against the model's instances: status; the tape is feasible and yields `soc_plan`; `plan_cost` is the
    tape's cost; the per-env bound is the sum of the relaxed optima; the relaxed cost of `soc_plan`'s trajectories is that sum
    too (the forward pass recovered an OPTIMAL trajectory, not just a feasible one); where the relaxation equals the MILP
    (`gap_zero_envs`), `plan_cost` is the bound.  The reference of the trajectory identity and of the gap-zero check is the
    model's optimum, not the kernel's bound; tolerance rtol = atol = 1e-9 as for the bound (HiGHS and the NumPy solver differ
    by 5e-15 of max(1, |bound|) on these families, tests/test_lp_model_cpu.py; a per-env sum has up to 130 terms)."""
    want_bound, want_cost, traj = np.zeros(E_), np.zeros(E_), np.zeros(E_)
    for (e, c), inst in insts.items():
        want_bound[e] += relaxed_opt(inst)
        a = plan["actions"][:, e, c]
        soc = M.check_tape(inst, a)
        np.testing.assert_allclose(soc, np.where(np.r_[inst["there"], True], plan["soc_plan"][:, e, c], 0.0), atol=1e-10,
                                   err_msg=f"lane {(e, c)}")
        want_cost[e] += sum(M.action_cost(inst, i, a[i]) for i in range(H_))
        traj[e] += M.relaxed_cost_of_trajectory(inst, plan["soc_plan"][:, e, c])
        assert plan["status"][e, c] == M.sessions(inst)[2], (e, c)
    assert len(insts) == E_ * N_ == plan["status"].size
    scale = np.maximum(1.0, np.abs(want_bound))
    print(f"{E_} x {N_} x {H_}: bound {np.max(np.abs(plan['bound'] - want_bound) / scale):.2e}, trajectory "
          f"{np.max(np.abs(traj - want_bound) / scale):.2e}, cost {np.max(np.abs(plan['plan_cost'] - want_cost)):.2e}, "
          f"gap in [{plan['gap'].min():.3e}, {plan['gap'].max():.3e}]")
    np.testing.assert_allclose(plan["bound"], want_bound, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(traj, want_bound, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(plan["plan_cost"], want_cost, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(plan["gap"], want_cost - plan["bound"], rtol=1e-12, atol=1e-12)
    assert (plan["gap"] >= -1e-9).all()
    for e in gap_zero_envs:
        np.testing.assert_allclose(plan["plan_cost"][e], want_bound[e], rtol=1e-9, atol=1e-9, err_msg=f"gap-zero env {e}")


_ADV_TABLES = {}


def _adv_tables(use_case, N_):
    if (use_case, N_) not in _ADV_TABLES:
        _ADV_TABLES[use_case, N_] = M.adversarial_tables(use_case, N_, P=M.EVSE_KW[use_case], grid=M.grid_kw(use_case))
    return _ADV_TABLES[use_case, N_]


def _adv_setup(E_, N_, H_, use_case, seed, *, episode_hours=168, deg="rainflow", move_start=None):
    """A batch of E_ envs x N_ EVs on the adversarial tables (tests/lp_model.py), env e reset to a row of its family's block
    (`move_start(tables, starts, fams)` may move start rows inside their blocks)."""
    from bench import bench_config
    from fleetrl_amd.batch import FleetBatch
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params, time_features

    tables = _adv_tables(use_case, N_)
    cfg = bench_config(E_, N_, use_case, True, True, deg)
    cfg["episode_length"] = episode_hours
    p = make_params(resolve_config(cfg), tables, E_, auto_reset=True, seed=0)
    assert p.evse_power == M.EVSE_KW[use_case] and p.init_soh == 1.0 and p.episode_steps == 4 * episode_hours >= H_
    p.grid_connection = M.grid_kw(use_case)  # (sized from the load otherwise: it would never bind)
    starts, fams = M.adversarial_starts(E_, H_, seed)
    if move_start is not None:
        move_start(tables, starts, fams)
        assert all(M.family_of_row(t) == f == M.family_of_row(t + H_ - 1) for t, f in zip(starts, fams))
    tf = time_features(tables)
    hip = FleetBatch(p, tables, tf)
    hip.set_start_schedule(starts[None, :])
    hip.reset()
    assert np.array_equal(hip.get("time_idx"), starts)
    return p, tables, tf, starts, fams, hip


@pytest.mark.parametrize("E_,N_,H_,use_case,seed", M.ADVERSARIAL_SHAPES, ids=lambda v: str(v))
def test_every_lane_matches_the_model_on_adversarial_tables(E_, N_, H_, use_case, seed):
    """Every (env, EV) lane at ragged shapes: one lane, horizons of 1, 2 and 3 rows, 64 and 130 EVs, 900 lanes (four workgroups,
    the last partly filled; the scratch is strided by E * N), 95 rows and a 7-day episode; env e plans the family
    FAMILIES[(e + seed) % 7] of tests/lp_model.py."""
    from fleetrl_amd.lp_benchmark import plan_linear_optimization

    p, tables, _, starts, fams, hip = _adv_setup(E_, N_, H_, use_case, seed)
    plan = plan_linear_optimization(hip, H_)
    insts = M.instances_of(tables, p, hip.get("time_idx"), hip.get("soc"), H_)
    _check_plan(plan, insts, E_, N_, H_, gap_zero_envs=[e for e, f in enumerate(fams) if f == "gap_zero"])


def test_adversarial_shapes_cover_every_category():
    """What test_every_lane_matches_the_model_on_adversarial_tables plans, summarised by the model alone from the same live
    states (nothing of the kernel's output): rows with G < P, G < 0, price < 0, price == 0, s >= P, 0 < s < G < P, s > G; row
    costs of 1 to 4 pieces (5 cannot occur, tests/test_lp_model_cpu.py); every status bit set and clear; EVs away at row 0 and
    present on the last row.  A generator that drifts out of a category fails here instead of testing nothing."""
    total = None
    for E_, N_, H_, use_case, seed in M.ADVERSARIAL_SHAPES:
        p, tables, _, _, _, hip = _adv_setup(E_, N_, H_, use_case, seed)
        cov = M.coverage(M.instances_of(tables, p, hip.get("time_idx"), hip.get("soc"), H_))
        assert cov["lanes"] == E_ * N_
        if N_ >= 64:
            assert cov["rows"]["G<P"] and cov["rows"]["s>G"] and cov["pieces"].get(4), (N_, cov)
        total = M.merge_coverage(total, cov)
    print(total)
    M.assert_covered(total)
    assert total["whole_horizon_session"] and max(total["pieces"]) == 4 and total["lanes"] > 256


def _step_rows(hip, actions):
    """Step the batch once per row of `actions` [K, E, N] (float64)."""
    import torch

    dev = torch.device("cuda", 0)
    obs = torch.zeros((hip.E, hip.obs_dim), device=dev)
    rew = torch.zeros(hip.E, device=dev, dtype=torch.float64)
    done = torch.zeros(hip.E, device=dev, dtype=torch.uint8)
    tape = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.float64)).to(dev)
    for i in range(tape.shape[0]):
        hip.step_dev(tape[i].data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), act_dtype=_capi.ACT_F64)
        assert not done.any().item(), i
    hip.check_errors()


def test_plans_from_live_states_mid_episode():
    """Plans of exactly the rows left after K steps of a 192-row episode, K = 5, 60, 131 and 190 (a launch steps every env of a
    batch, so each K has a batch of its own): a third of the envs driven with +1, a third with -1, the rest with random actions.
    The env caps every charge at the target (ev_charger.py:100-114: an action >= 0 even brings a higher SOC down to it), so
    a live SOC above the target is one that arrived with it on the very row the plan starts from: the envs of the "returns"
    family start K rows before such an arrival, and FLEET_LP_ABOVE_TARGET is then set on a STARTING SOC."""
    from fleetrl_amd.lp_benchmark import plan_linear_optimization

    total = None
    above_bit_from_start = 0
    for K in (5, 60, 131, 190):
        E_, N_, H_ = 14, 5, 192 - K

        def before_a_high_arrival(tables, starts, fams, K=K):
            there, sor = np.asarray(tables.there) != 0, np.asarray(tables.soc_on_return)
            for e, f in enumerate(fams):
                if f != "returns":
                    continue
                b0 = (int(starts[e]) // M.BLOCK) * M.BLOCK
                rows = np.arange(b0 + K, b0 + M.BLOCK - 192 + K)  # plan rows whose episode stays inside the block
                hit = (there[rows] & ~there[rows - 1] & (sor[rows] > 0.85)).any(axis=1)
                starts[e] = rows[np.nonzero(hit)[0][e % hit.sum()]] - K

        p, tables, _, starts, fams, hip = _adv_setup(E_, N_, 192, "lmd", K % 7, episode_hours=48, deg="none",
                                                     move_start=before_a_high_arrival)
        rng = np.random.default_rng(K)
        act = rng.uniform(-1.0, 1.0, size=(K, E_, N_))
        act[:, 0::3] = 1.0
        act[:, 1::3] = -1.0
        _step_rows(hip, act)
        t0, soc = hip.get("time_idx"), hip.get("soc")
        assert np.array_equal(t0, starts + K)
        plan = plan_linear_optimization(hip, H_)
        insts = M.instances_of(tables, p, t0, soc, H_)
        cov = M.coverage(insts)
        total = M.merge_coverage(total, cov)
        for (e, c), inst in insts.items():
            if inst["there"][0] and inst["soc0"] > inst["target"]:
                assert plan["status"][e, c] & _capi.LP_ABOVE_TARGET and plan["soc_plan"][0, e, c] == inst["target"]
                above_bit_from_start += 1
        _check_plan(plan, insts, E_, N_, H_, gap_zero_envs=[e for e, f in enumerate(fams) if f == "gap_zero"])
    print(total)
    assert above_bit_from_start > 0 and total["start_above_target"] == above_bit_from_start
    assert total["rows"]["G<P"] and total["rows"]["s>G"] and total["rows"]["price<0"] and total["away_at_row_0"]


def test_replay_on_adversarial_tables_follows_the_plan_and_the_oracle():
    """The tape of a whole 192-row episode per family, replayed: the rewards are the CPU oracle's at every row, and the env's SOC
    is `soc_plan` while an EV is present, for the lanes whose status has neither clamp bit.  (A SOC_on_return below 0 or above
    the target is clamped in the model and not in the env: there the model is knowingly not the env.)  On grid-bound rows the SOC
    still follows the plan because the env never curtails a charger for the grid: it moves the SOC by the action alone and only
    PENALISES the fleet's overload (fleet_environment.py:480-502), and the tape keeps (c + d) P <= G per EV by itself."""
    import torch

    from fleetrl_amd.batch import FleetBatch
    from fleetrl_amd.lp_benchmark import plan_linear_optimization, run_linear_optimization
    from oracle.fleet_oracle import OracleBatch

    E_, N_, H_ = 14, 10, 192
    p, tables, tf, starts, fams, hip = _adv_setup(E_, N_, H_, "lmd", 0, episode_hours=48, deg="none")
    assert set(fams) == set(M.FAMILIES)
    plan = plan_linear_optimization(hip, H_)
    tape = plan["actions"]
    cpu = OracleBatch(p, tables, tf)
    cpu.set_start_schedule(starts[None, :])
    cpu.reset()
    dev = torch.device("cuda", 0)
    tape_d = torch.from_numpy(tape).to(dev)
    obs = torch.zeros((E_, hip.obs_dim), device=dev)
    rew = torch.zeros(E_, device=dev, dtype=torch.float64)
    done = torch.zeros(E_, device=dev, dtype=torch.uint8)
    rsum = np.zeros(E_)
    there = np.asarray(tables.there) != 0
    unclamped = (plan["status"] & (_capi.LP_NEG_RETURN | _capi.LP_ABOVE_TARGET)) == 0
    assert unclamped.any(axis=1).all() and not unclamped.all()
    G = p.grid_connection - np.asarray(tables.load) + np.asarray(tables.pv)
    grid_bound_rows_charged = 0
    for i in range(H_):
        hip.step_dev(tape_d[i].data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), act_dtype=_capi.ACT_F64)
        _o, r_cpu, _d, _t = cpu.step(tape[i])
        r = rew.cpu().numpy()
        np.testing.assert_allclose(r, r_cpu, rtol=1e-9, atol=1e-9, err_msg=f"row {i}")
        rsum += r
        grid_bound_rows_charged += int(((G[starts + i] < p.evse_power)[:, None] & (tape[i] > 0) & unclamped).sum())
        if i + 1 < H_:
            pres = there[starts + i + 1] & unclamped
            np.testing.assert_allclose(np.where(pres, hip.get("soc"), 0.0), np.where(pres, plan["soc_plan"][i + 1], 0.0), rtol=0,
                                       atol=1e-10, err_msg=f"row {i + 1}")
    hip.check_errors()
    assert grid_bound_rows_charged > 0
    hip2 = FleetBatch(hip.params, tables, tf)
    hip2.set_start_schedule(starts[None, :])
    hip2.reset()
    _obs, rs, dc = run_linear_optimization(hip2, H_)
    np.testing.assert_allclose(rs, rsum, rtol=1e-9, atol=1e-9)
    assert (dc == 1).all()  # the plan spans the whole episode


def test_scratch_is_reused_across_horizons():
    """The handle's scratch grows on demand, is never cleared, and its layout depends on H: plans of 192, 50 and 192 rows on
    one handle; the first and the third are bit-identical, the second is a fresh handle's, bit for bit."""
    from fleetrl_amd.lp_benchmark import plan_linear_optimization

    _, _, _, _, _, hip = _adv_setup(9, 7, 192, "ct", 0)
    a, b, c = (plan_linear_optimization(hip, h) for h in (192, 50, 192))
    _, _, _, _, _, fresh = _adv_setup(9, 7, 192, "ct", 0)
    d = plan_linear_optimization(fresh, 50)
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k
        assert b[k].tobytes() == d[k].tobytes(), k
    assert b["actions"].shape == (50, 9, 7) and np.isfinite(b["bound"]).all()


@pytest.mark.parametrize("name", ["lmd5_price_linear", "ct5_both_rainflow"])
def test_plan_matches_the_model(name):
    from fleetrl_amd.lp_benchmark import plan_linear_optimization

    g, p, tables, _, hip = _setup(name)
    if name.startswith("ct"):
        assert np.asarray(tables.pv).max() > 0 and p.include_pv
    plan = plan_linear_optimization(hip, H)
    insts = _instances(p, tables, hip)
    want_bound = np.zeros(E)
    want_cost = np.zeros(E)
    for (e, c), inst in insts.items():
        want_bound[e] += relaxed_opt(inst)
        a = plan["actions"][:, e, c]
        soc = M.check_tape(inst, a)
        np.testing.assert_allclose(soc, np.where(np.r_[inst["there"], True], plan["soc_plan"][:, e, c], 0.0), atol=1e-10)
        want_cost[e] += sum(M.action_cost(inst, i, a[i]) for i in range(H))
        assert plan["status"][e, c] == M.sessions(inst)[2], (e, c)
    np.testing.assert_allclose(plan["bound"], want_bound, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(plan["plan_cost"], want_cost, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(plan["gap"], want_cost - plan["bound"], rtol=1e-12, atol=1e-12)
    assert (plan["gap"] >= -1e-9).all()


@pytest.mark.parametrize("name", ["lmd5_price_linear", "ct5_both_rainflow"])
def test_replay_follows_the_plan_and_the_oracle(name):
    import torch

    from fleetrl_amd.batch import FleetBatch
    from fleetrl_amd.lp_benchmark import plan_linear_optimization, run_linear_optimization
    from oracle.fleet_oracle import OracleBatch

    g, p, tables, starts, hip = _setup(name, log=True, no_deg=True)
    plan = plan_linear_optimization(hip, H)
    tape = plan["actions"]
    p_cpu = params_for(g, num_envs=E)
    p_cpu.init_soh = 1.0
    p_cpu.deg_mode = _capi.DEG_NONE
    cpu = OracleBatch(p_cpu, tables, g.time_feat)
    cpu.set_start_schedule(starts)
    cpu.reset()
    dev = torch.device("cuda", 0)
    tape_d = torch.from_numpy(tape).to(dev)
    obs = torch.zeros((E, hip.obs_dim), device=dev)
    rew = torch.zeros(E, device=dev, dtype=torch.float64)
    done = torch.zeros(E, device=dev, dtype=torch.uint8)
    rsum = np.zeros(E)
    there = np.asarray(tables.there) != 0
    t0 = hip.get("time_idx")
    for i in range(H):
        hip.step_dev(tape_d[i].data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), act_dtype=_capi.ACT_F64)
        _o, r_cpu, _d, _t = cpu.step(tape[i])
        r = rew.cpu().numpy()
        np.testing.assert_allclose(r, r_cpu, rtol=1e-9, atol=1e-9)
        rsum += r
        if i + 1 < H:
            pres = there[t0 + i + 1]
            np.testing.assert_allclose(np.where(pres, hip.get("soc"), 0.0), np.where(pres, plan["soc_plan"][i + 1], 0.0), rtol=0,
                                       atol=1e-10, err_msg=f"row {i + 1}")
    hip.check_errors()
    # no SOC-violation penalty in the envs whose EVs all have a clear status
    lg = hip.log_read(with_obs=False)
    clear = (plan["status"] == 0).all(axis=1)
    assert clear.any() or name.startswith("ct")  # (the caretakers' short lunch sessions often cannot reach the target)
    pos = lg["pos"]
    for e in np.nonzero(clear)[0]:
        rows = np.arange(max(0, pos[e] - lg["capacity"]), pos[e]) % lg["capacity"]
        assert np.all(lg["env"][rows, e, 3] == 0.0), e
    # run_linear_optimization from the same start: the same rewards
    hip2 = FleetBatch(hip.params, tables, g.time_feat)
    hip2.set_start_schedule(starts)
    hip2.reset()
    _obs, rs, dc = run_linear_optimization(hip2, H)
    np.testing.assert_allclose(rs, rsum, rtol=1e-9, atol=1e-9)
    assert (dc == 1).all()  # the plan spans the whole episode


def test_status_bits_on_constructed_cases():
    from fleetrl_amd.lp_benchmark import plan_linear_optimization

    g = load_trace("ct5_both_rainflow")
    t = copy.copy(g.tables)
    sor = np.array(t.soc_on_return, dtype=np.float64, copy=True)
    sor[:, 0] = -np.abs(sor[:, 0]) - 0.05 * (np.asarray(t.there)[:, 0] != 0)  # EV 0 always returns below 0
    sor[:, 1] = np.where(np.asarray(t.there)[:, 1] != 0, 0.0, 0.0)         # EV 1 returns empty: short sessions cannot reach the target
    t.soc_on_return = sor
    _, p, tables, _, hip = _setup("ct5_both_rainflow", tables=t)
    plan = plan_linear_optimization(hip, H)
    insts = _instances(p, tables, hip)
    want = np.array([[M.sessions(insts[e, c])[2] for c in range(hip.N)] for e in range(E)])
    np.testing.assert_array_equal(plan["status"], want)
    assert (want[:, 0] & _capi.LP_NEG_RETURN).any() and (want & _capi.LP_UNREACHABLE).any()
    assert not (want[:, 2:] & _capi.LP_NEG_RETURN).any()


def test_horizon_past_the_episode_end_is_refused():
    import torch

    from fleetrl_amd.batch import FleetHipError
    from fleetrl_amd.lp_benchmark import plan_linear_optimization

    g, p, tables, _, hip = _setup("lmd5_price_linear")
    with pytest.raises(FleetHipError) as ei:
        plan_linear_optimization(hip, g.ep_steps + 1)
    assert ei.value.status == _capi.ERR_INVALID
    a = torch.zeros((E, hip.N), device="cuda:0")
    obs = torch.zeros((E, hip.obs_dim), device="cuda:0")
    rew = torch.zeros(E, device="cuda:0", dtype=torch.float64)
    done = torch.zeros(E, device="cuda:0", dtype=torch.uint8)
    hip.step_dev(a.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr())
    with pytest.raises(FleetHipError):
        plan_linear_optimization(hip, g.ep_steps)
    assert plan_linear_optimization(hip, g.ep_steps - 1)["actions"].shape == (g.ep_steps - 1, E, hip.N)


def test_two_calls_are_bit_identical():
    from fleetrl_amd.lp_benchmark import plan_linear_optimization

    _, _, _, _, hip = _setup("ct5_both_rainflow")
    a, b = plan_linear_optimization(hip, H), plan_linear_optimization(hip, H)
    c = plan_linear_optimization(hip, H, act_dtype="f32")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert c["actions"].dtype == np.float32 and np.array_equal(c["actions"], a["actions"].astype(np.float32))
    assert c["bound"].tobytes() == a["bound"].tobytes()


BENCH_ENVS = sorted({0, 4095, *np.random.default_rng(11).choice(np.arange(1, 4095), size=6, replace=False).tolist()})


def test_bench_size_plan(tmp_path):
    """4096 x 50 x 192 on the bench's synthetic caretaker tables with rainflow degradation, in a child process under its own time
    limit: finite, two calls bit-identical, and env 0, env 4095 and six seeded envs in between (all 50 EVs each, so the first and
    the last of the 204800 lanes) against the model, from the state the tool wrote out with the plan.  Eight of 4096 envs is the
    limit of this check."""
    import json

    from bench import bench_config
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params
    from fleetrl_amd.synth import synth_tables

    Eb, Nb, Hb = 4096, 50, 192
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lp_plan_bench.py"), "--reps", "1", "--dump", str(tmp_path),
                        "--dump-envs", ",".join(map(str, BENCH_ENVS))], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["finite"] and res["bit_identical"] and (res["envs"], res["evs"], res["horizon"]) == (Eb, Nb, Hb)
    z = np.load(os.path.join(str(tmp_path), "lp_plan_dump.npz"))
    assert z["envs"].tolist() == BENCH_ENVS and len(BENCH_ENVS) == 8
    tables = synth_tables("ct", Nb, seed=1234, include_building=True, include_pv=True, price_year="2020", feed_in="spot")
    p = make_params(resolve_config(bench_config(Eb, Nb, "ct", True, True, "rainflow")), tables, Eb, auto_reset=True, seed=0)
    insts = M.instances_of(tables, p, z["time_idx"], z["soc"], Hb)
    plan = {k: z[k] for k in ("actions", "soc_plan", "bound", "plan_cost", "status")}
    plan["gap"] = plan["plan_cost"] - plan["bound"]
    assert plan["actions"].shape == (Hb, 8, Nb)
    _check_plan(plan, insts, 8, Nb, Hb)
