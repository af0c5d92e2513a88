"""The scalar parameters off their defaults, HIP against the CPU oracle on every step, at the shapes the golden traces cannot reach.

The parameter sets are those of oracle/param_sets.py: the golden traces made from them (trace_*_offdef, *_look0, *_look12x14, *_min30,
*_min60, rttrace_*_offdef) pin the ORACLE to the unmodified reference under each set (tests/test_oracle_golden.py), so that the
comparisons here are against a pinned oracle.  Plumbing and bounds are those of tests/test_step_instances_gpu.py (`Pair`), nothing
new: flags, indices and counters bit-exact, float32 observations rtol 1e-5 / atol 1e-6, float64 state rtol 1e-9 (fd_cyc 1e-8).

Per set: one case per lane-group width the planner selects (G = 8 ... 256), the uses (float32 / float64 single steps, 61-step tapes
with the hand-over, 1-step tapes, real_time, the data log with all three policies) rotated over the widths so that every set meets
every use and every lane group (real_time and the log on the widths up to 64 only: `uses_of_set`;
tests/test_param_sets_cpu.py checks the coverage through the planner), each over at least two auto-resets.  look12x14 makes the env-level tail 66 floats: longer than the group
at G = 8 ... 64, shorter at G = 128 / 256 -- the instance each case takes is read back from the planner, not assumed.
Needs an MI355X."""
import dataclasses

import numpy as np
import pytest

import step_instances as si
import test_step_instances_gpu as tsi
from fleetrl_amd import _capi
from fleetrl_amd.config import resolve_config
from fleetrl_amd.params import make_params, time_features
from fleetrl_amd.synth import synth_tables
from oracle.param_sets import PARAM_SETS

pytestmark = pytest.mark.gpu

WIDTHS = {7: 8, 13: 16, 31: 32, 50: 64, 100: 128, 130: 256}  # EVs per env -> lanes per env of the instances it selects
USES = ("f32", "f64", "tape", "tape1", "rt", "log")
LOG_USES = ("f32", "f64", "tape1", "tape", "uncontrolled", "distributed", "night")
# set -> (fleet type, degradation, normalise): caretakers where the lunch target matters, normalised utility fleets for the derived
# normaliser constants; building load + PV + auxiliary observations everywhere (the 66-float tail needs all three)
STEP_SETS = {"offdef": ("ct", "rainflow", False), "offdef_norm": ("ut", "linear", True), "look0": ("lmd", "rainflow", False),
             "look12x14": ("ct", "rainflow", False)}
_TABLES = {}


def config_for(pset, uc, deg, norm, *, real_time=False, log_data=False, episode_length=24, drop=()):
    case = si.Case("", (), 0, 0, 0, uc, deg, real_time, log_data, norm, True, True, True, False, 0)
    cfg = si.config_of(case)
    cfg["episode_length"] = episode_length
    cfg.update({k: v for k, v in PARAM_SETS[pset].items() if k not in drop})
    return cfg


def tables_for(rc, uc, n, minutes=15):
    """Synthetic tables drawn for the resolved configuration: the target SOCs and the markups enter the pre-staged columns."""
    key = (uc, n, minutes, rc.target_soc, rc.target_soc_lunch, rc.fixed_markup, rc.variable_multiplier, rc.feed_in_deduction)
    if key not in _TABLES:
        tb = synth_tables(uc, n, seed=100 + n, target_soc=rc.target_soc, target_soc_lunch=rc.target_soc_lunch,
                          fixed_markup=rc.fixed_markup, variable_multiplier=rc.variable_multiplier,
                          feed_in_deduction=rc.feed_in_deduction, minutes=minutes)
        _TABLES[key] = (tb, time_features(tb))
    return _TABLES[key]


SMALL, BIG = (7, 13, 31, 50), (100, 130)  # widths up to one wavefront per env; beyond it (G = 128, 256)
PLAIN = ("f32", "f64", "tape", "tape1")


def uses_of_set(i):
    """{width: use} of the i-th set.  real_time and the data log stay on the widths up to 64: beyond one wavefront the planner
    gives them the instances whose lanes walk several EVs ("G64w", tests/step_instances.py), so a case there would not run the
    G = 128 / 256 instances at all.  The two big widths take two of the plain uses, the small ones real_time, the log and the
    other two, all rotated with i: every set meets every use and every lane group, and no use sits on one width in all sets."""
    pl = PLAIN[i % 4:] + PLAIN[:i % 4]
    small = ("rt", "log", pl[2], pl[3])
    small = small[i % 4:] + small[:i % 4]
    return {**dict(zip(SMALL, small)), **dict(zip(BIG, pl[:2]))}


def make_case(pset, n_evs, use, seed):
    uc, deg, norm = STEP_SETS[pset]
    rt, log = use == "rt", use == "log"
    uses = LOG_USES if log else (use,)
    lanes = WIDTHS[n_evs]
    epb = si.K_BLOCK // lanes
    E = 2 * epb + 3 if epb > 1 else 4  # whole workgroups and a partly filled last one
    f64 = bool(seed % 2)
    probe = si.Case("", uses, lanes, n_evs, E, uc, deg, rt, log, norm, True, True, True, f64, seed)
    names = {ln.instance(E)[0] for ln in probe.launches()}  # what the planner itself selects, not an assumption
    assert len(names) == 1, names
    (name,) = names
    assert name.startswith(f"G{lanes}.{deg}."), (name, n_evs, use)
    return dataclasses.replace(probe, instance=name)


def step_cases():
    out = []
    for i, pset in enumerate(STEP_SETS):
        for n, use in uses_of_set(i).items():
            out.append((pset, make_case(pset, n, use, seed=len(out))))
    return out


def param_pair(case, pset, log_rows=0, episode_length=24, drop=()):
    """tests/test_step_instances_gpu.py `Pair` under a parameter set: its config and tables drawn for the set."""
    cfg = config_for(pset, case.uc, case.deg, case.norm, real_time=case.real_time, log_data=case.log_data,
                     episode_length=episode_length, drop=drop)
    rc = resolve_config(cfg)
    pair = tsi.Pair(case, log_rows=log_rows, cfg=cfg, tables=tables_for(rc, case.uc, case.n_evs, rc.minutes))
    p = pair.p
    for k, v in PARAM_SETS[pset].items():  # the set really reached the scalar block
        if k in ("price_lookahead", "bl_pv_lookahead", "charging_eff", "discharging_eff", "temperature", "obc_max_power") and k not in drop:
            assert getattr(p, k) == v, k
    assert p.steps_per_hour * rc.minutes == 60 and p.episode_steps == episode_length * p.steps_per_hour
    assert pair.hip.obs_dim == pair.cpu.obs_dim
    return pair


@pytest.mark.parametrize("pset,case", step_cases(), ids=lambda v: v if isinstance(v, str) else v.id)
def test_steps_under_a_parameter_set_match_the_oracle(pset, case):
    """The runs of tests/test_step_instances_gpu.py `_run`, 24 h episodes, every env through at least two auto-resets."""
    def make_pair(c, log_rows=0):
        pair = param_pair(c, pset, log_rows=log_rows)
        if pset == "look12x14":
            assert pair.hip.obs_dim == 7 * c.n_evs + 66
        return pair

    if pset == "look12x14":
        L, B = PARAM_SETS[pset]["price_lookahead"], PARAM_SETS[pset]["bl_pv_lookahead"]
        tail = 2 * (L + 1) + 2 * (B + 1) + 10
        assert tail == 66 and (tail > case.lanes) == (case.lanes <= 64)
    tsi._run(case, make_pair)


@pytest.mark.parametrize("use", ["uncontrolled", "distributed", "night"])
def test_policies_under_the_off_default_set(use):
    """The device-side policies on a caretaker fleet with charging_eff 0.95 != discharging_eff 0.83, target 0.8 and a lunch target
    of 0.55.  The night window is derived from the handle's own parameters and must be the one the reference's expressions give
    (`NightChargingRule.parameters`, pinned to the reference by tests/test_policies_cpu.py) for THIS charging_eff and target."""
    from fleetrl_amd.policies import night_schedule
    from oracle.fleet_oracle import NightChargingRule

    case = si.Case("", (use,), 64, 50, 11, "ct", "rainflow", False, False, False, True, True, True, False, 40)
    case = dataclasses.replace(case, instance=case.launches()[0].instance(11)[0])
    pair = param_pair(case, "offdef")
    try:
        if use == "night":
            p, tb = pair.p, pair.tb
            assert (p.charging_eff, p.target_soc) == (0.95, 0.8)
            kw = dict(init_battery_cap=p.init_battery_cap, evse_power=p.evse_power)
            got = night_schedule(tb, target_soc=p.target_soc, charging_eff=p.charging_eff, **kw)
            there = (np.asarray(tb.there) != 0).T.reshape(-1)  # ID-major, like the reference's frame
            rows = (np.nonzero(there[:-1] & ~there[1:])[0] + 1) % tb.T
            ph, pm, pt = NightChargingRule.parameters(np.asarray(tb.hour)[rows], np.asarray(tb.minute)[rows], p.target_soc,
                                                      p.init_battery_cap, p.charging_eff, p.evse_power)
            assert (ph, pm, int(pt)) == got and pt == 0.8 * p.init_battery_cap / 0.95 / p.evse_power
            # the window the defaults would give is another one: the derived window really depends on the two parameters
            assert got[:2] != night_schedule(tb, target_soc=0.85, charging_eff=0.91, **kw)[:2]
            pair.night(case.policy_chunks(), (si.K_TAPE, 40))
        else:
            pair.policy(use, case.policy_chunks())
        pair.finish()
    finally:
        pair.close()


# ---- 30- and 60-minute steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset,uc,n_evs,use", [("min30", "ct", 50, "f32"), ("min30", "lmd", 7, "tape"), ("min30", "ut", 100, "f64"),
                                               ("min60", "ct", 13, "f32"), ("min60", "lmd", 50, "tape"), ("min60", "ct", 130, "f64")])
def test_coarser_steps_match_the_oracle(pset, uc, n_evs, use):
    """Tables resampled to 30 / 60 minutes, rainflow configured, 48 h episodes (96 / 48 rows), over two episode ends.  No row reads
    14:45, so the degradation model never runs (what the reference itself recorded: trace_ct3_both_rainflow_min30): SoH stays at 1,
    rainflow_length at its initial 1, and no episode has a last degradation row (rf_until = -1)."""
    lanes = WIDTHS[n_evs]
    E = 2 * (si.K_BLOCK // lanes) + 3 if lanes < si.K_BLOCK else 4
    case = si.Case("", (use,), lanes, n_evs, E, uc, "rainflow", False, False, False, True, True, True, use == "f64", 60 + n_evs)
    name = case.launches()[0].instance(E)[0]
    assert name.startswith(f"G{lanes}.rainflow.")
    pair = param_pair(dataclasses.replace(case, instance=name), pset, episode_length=48)
    try:
        sph = 60 // PARAM_SETS[pset]["minutes"]
        assert pair.p.steps_per_hour == sph and pair.p.dt == 1 / sph and not (np.asarray(pair.tb.minute) == 45).any()
        steps = 2 * 48 * sph + 10
        if use == "tape":
            pair.tape(si.K_TAPE, -(-steps // si.K_TAPE), case.f64)
            pair.single_steps(20, False, what="single step after the launches")
        else:
            pair.single_steps(steps, use == "f64")
        pair.finish()
        assert (pair.hip.get("soh") == 1.0).all() and (pair.hip.get("rf_len") == 1).all() and not pair.hip.get("fd_cyc").any()
        assert (pair.hip.get("rf_until") == -1).all()
    finally:
        pair.close()


def test_counting_to_the_end_changes_nothing_without_a_degradation_row():
    """tests/test_rf_tail_gpu.py's comparison on 30-minute tables: no episode holds a degradation row, so the default batch counts
    nothing at all (rf_until = -1) while `set_rainflow_count_all` counts every sample -- and everything the reference can see is
    identical after every step, over two episode ends."""
    from fleetrl_amd.batch import FleetBatch
    from test_rf_tail_gpu import VISIBLE

    E, N = 37, 5
    rc = resolve_config(config_for("min30", "ct", "rainflow", False, episode_length=24))
    tb, tf = tables_for(rc, "ct", N, 30)
    p = make_params(rc, tb, E, seed=3)
    a, b = FleetBatch(p, tb, tf), FleetBatch(p, tb, tf)
    b.set_rainflow_count_all(True)
    np.testing.assert_array_equal(a.reset(), b.reset())
    rng = np.random.default_rng(8)
    differed = 0
    for k in range(2 * p.episode_steps + 9):
        act = rng.uniform(-1, 1, size=(E, N)).astype(np.float32)
        act[rng.random((E, N)) < 0.15] = 0.0
        ra, rb = a.step(act), b.step(act)
        for x, y, what in zip(ra[:3], rb[:3], ("obs", "reward", "done")):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}, step {k}")
        for f in VISIBLE:
            np.testing.assert_array_equal(a.get(f), b.get(f), err_msg=f"{f}, step {k}")
        ca, cb = a.get("rf_cycles"), b.get("rf_cycles")
        assert (ca <= cb).all()
        differed += int((ca != cb).any())
    assert differed > 0 and (a.get("rf_until") == -1).all() and (b.get("rf_until") == np.iinfo(np.int32).max).all()
    assert a.get("episodes").min() >= 2
    a.check_errors(); b.check_errors()
    a.close(); b.close()


# ---- the linear-optimisation benchmark --------------------------------------------------------------------------------------------
# obc_max_power stays at its default here: tests/lp_model.py (like the reference's model) knows one charging power, the EVSE's
_LP_DROP = ("obc_max_power",)


def _lp_batch(cfg, tables, E, starts):
    from fleetrl_amd.batch import FleetBatch

    p = make_params(resolve_config(cfg), tables, E, auto_reset=True, seed=0)
    hip = FleetBatch(p, tables, time_features(tables))
    hip.set_start_schedule(np.asarray(starts, np.int32)[None, :])
    hip.reset()
    assert np.array_equal(hip.get("time_idx"), starts)
    return p, hip


def test_lp_plan_with_unequal_efficiencies_on_adversarial_tables():
    """tests/test_lp_plan_gpu.py's per-lane checks at a ragged shape (3 envs x 7 EVs x 95 rows) with eta_c = 0.95 != eta_d = 0.83,
    target 0.8, markups 7.3 / 1.3 and a feed-in deduction of 0.1, on adversarial tables drawn for these values; then the replay."""
    import lp_model as M
    from fleetrl_amd.lp_benchmark import plan_linear_optimization, run_linear_optimization
    from test_lp_plan_gpu import _check_plan

    E, N, H, uc, seed = 3, 7, 95, "ct", 3
    cfg = config_for("offdef", uc, "rainflow", False, episode_length=168, drop=_LP_DROP)
    rc = resolve_config(cfg)
    tables = M.adversarial_tables(uc, N, P=M.EVSE_KW[uc], grid=M.grid_kw(uc), eta_c=rc.charging_eff, eta_d=rc.discharging_eff,
                                  fixed_markup=rc.fixed_markup, variable_multiplier=rc.variable_multiplier,
                                  feed_in_deduction=rc.feed_in_deduction)
    starts, fams = M.adversarial_starts(E, H, seed)
    p, hip = _lp_batch(cfg, tables, E, starts)
    assert (p.charging_eff, p.discharging_eff, p.target_soc) == (0.95, 0.83, 0.8)
    p.grid_connection = M.grid_kw(uc)
    hip.close()
    from fleetrl_amd.batch import FleetBatch

    hip = FleetBatch(p, tables, time_features(tables))  # (the grid connection of the adversarial cases, as in `_adv_setup`)
    hip.set_start_schedule(np.asarray(starts, np.int32)[None, :])
    hip.reset()
    plan = plan_linear_optimization(hip, H)
    insts = M.instances_of(tables, p, hip.get("time_idx"), hip.get("soc"), H)
    assert all(i["eta_c"] == 0.95 and i["eta_d"] == 0.83 and i["target"] == 0.8 for i in insts.values())
    _check_plan(plan, insts, E, N, H, gap_zero_envs=[e for e, f in enumerate(fams) if f == "gap_zero"])
    # the replay (`run_linear_optimization`: plan, then step the float64 tape) against the oracle stepping the same tape
    from oracle.fleet_oracle import OracleBatch

    cpu = OracleBatch(p, tables, time_features(tables))
    cpu.set_start_schedule(np.asarray(starts, np.int32)[None, :])
    cpu.reset()
    rsum = np.zeros(E)
    for a in plan["actions"]:
        oc, r, d, _t = cpu.step(a)
        rsum += r
        assert not d.any()
    obs, rs, dc = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in run_linear_optimization(hip, H))
    np.testing.assert_allclose(rs, rsum, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(obs, oc, rtol=1e-5, atol=1e-6)
    assert (dc == 0).all()
    np.testing.assert_allclose(hip.get("soc"), cpu.get("soc"), rtol=1e-9, atol=1e-12)
    assert not cpu.get("error_bits").any()
    cpu.close()
    hip.check_errors()
    hip.close()


def test_lp_plan_at_half_hour_steps():
    """dt = 0.5: the same per-lane checks on 30-minute synthetic tables (5 envs x 5 EVs x 48 rows = 24 h)."""
    import lp_model as M
    from fleetrl_amd.lp_benchmark import plan_linear_optimization
    from test_lp_plan_gpu import _check_plan

    E, N, H, uc = 5, 5, 48, "lmd"
    cfg = config_for("min30", uc, "none", False, episode_length=48)
    cfg.update({k: v for k, v in PARAM_SETS["offdef"].items() if k not in _LP_DROP + ("price_lookahead", "bl_pv_lookahead")})
    rc = resolve_config(cfg)
    tables, _ = tables_for(rc, uc, N, 30)
    starts = np.random.default_rng(4).integers(0, tables.T - 200, size=E).astype(np.int32)
    p, hip = _lp_batch(cfg, tables, E, starts)
    assert p.dt == 0.5 and p.episode_steps == 96
    plan = plan_linear_optimization(hip, H)
    insts = M.instances_of(tables, p, hip.get("time_idx"), hip.get("soc"), H)
    assert all(i["dt"] == 0.5 for i in insts.values())
    _check_plan(plan, insts, E, N, H)
    hip.check_errors()
    hip.close()


# ---- env state ---------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_and_fingerprint_with_other_lookaheads():
    """tests/test_state_gpu.py's rewind with L = 3, B = 6 (the observation rows in the blob have another width), a fork between two
    such handles, and a load refused between two handles that differ ONLY in bl_pv_lookahead."""
    from fleetrl_amd.batch import FleetBatch
    from test_state_gpu import _assert_same, _refused, _run, _tape

    E, N = 13, 5
    cfg = config_for("offdef", "ct", "rainflow", False)
    rc = resolve_config(cfg)
    tb, tf = tables_for(rc, "ct", N)
    p = make_params(rc, tb, E, seed=1)
    b = FleetBatch(p, tb, tf)
    assert b.obs_dim == 7 * N + 2 * 4 + 2 * 7 + 10
    rng = np.random.default_rng(5)
    b.reset()
    tape = _tape(rng, 40 + 200, E, N)
    _run(b, tape[:40], with_fields=False)
    blob = b.save_state()
    first = _run(b, tape[40:])
    b.load_state(blob)
    _assert_same(_run(b, tape[40:]), first, "second pass after load")
    assert np.array([r["done"] for r in first]).any()
    twin = FleetBatch(p, tb, tf)
    twin.reset()
    twin.load_state(blob)
    twin.fork_envs([0, 1], [2, 3], source=b)
    for f in ("soc", "soh", "time_idx", "rf_len", "fd_cyc"):
        np.testing.assert_array_equal(twin.get(f)[[2, 3]], b.get(f)[[0, 1]], err_msg=f)
    cfg2 = dict(cfg, bl_pv_lookahead=cfg["bl_pv_lookahead"] + 1)
    p2 = make_params(resolve_config(cfg2), tb, E, seed=1)
    diff = [f for f, _ in _capi.FleetParams._fields_ if getattr(p, f) != getattr(p2, f)]
    assert diff == ["bl_pv_lookahead"], diff
    other = FleetBatch(p2, tb, tf)
    other.reset()
    before = other.save_state()
    _refused(lambda: other.load_state(blob), _capi.ERR_INVALID, "bl_pv_lookahead")
    _refused(lambda: other.fork_envs([0], [1], source=b), _capi.ERR_INVALID, "bl_pv_lookahead")
    assert other.save_state().tobytes() == before.tobytes()
    for x in (b, twin, other):
        x.check_errors()
        x.close()
