"""The linear-optimisation benchmark on the GPU (`fleet_lp_plan_dev`, fleetrl_amd/lp_benchmark.py): every (env, EV) plan
against the model restated in tests/lp_model.py (scipy HiGHS, or the NumPy solver where scipy is missing), the replayed
tape against the plan and the CPU oracle, status bits, the horizon guard, determinism and the bench-size call.  Needs an
MI355X."""
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


def test_bench_size_plan():
    """4096 x 50 x 192 on the bench's synthetic caretaker tables with rainflow degradation, in a child process under its own time
    limit."""
    import json

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lp_plan_bench.py"), "--reps", "1"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["finite"] and res["bit_identical"] and (res["envs"], res["evs"], res["horizon"]) == (4096, 50, 192)
