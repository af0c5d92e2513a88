"""The data log summarised on the device (fleet_log_summary_dev, fleetrl_amd.evaluation) on the GPU: the three golden logs
replayed and summarised against the reference's arithmetic on the fixtures, and every output bit for bit against the NumPy
restatement (tests/logsum_model.py) on the device's own ring -- at the shapes where the reduction can go wrong: one EV, a
partial chunk, exactly one chunk, a carry across the 64-lane boundary, three chunks; one row, a full block, a block and one row,
three blocks; wrapped rings; envs whose rings differ in length; an empty window.  Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

import logsum_model as lm
from golden_util import load_rt_trace

pytestmark = pytest.mark.gpu

OUTPUTS = ("scal", "deg_sum", "soh_last", "prof_sum", "prof_cnt", "hist")
_TABLES = {}


def _tables(n):
    from fleetrl_amd.synth import synth_tables

    if n not in _TABLES:
        _TABLES[n] = synth_tables("ct", n, seed=100 + n)
    return _TABLES[n]


def _outputs(s) -> dict:
    return {k: getattr(s, k) for k in OUTPUTS}


def _model(core, **kw):
    lg = core.batch.log_read(with_obs=False)
    regular = "irregular" not in core.tables.meta
    return lm.summarize(lg, core.tables.hour, core.tables.minute, minutes_per_step=int(core.rc.minutes) if regular else 0,
                        price_multiplier=core.rc.price_multiplier, calc_deg=core.rc.calc_deg, **kw), lg


def _assert_equals_model(env, drop_last=0, bins=50, range=(-1.0, 1.0), hist_ev=0):
    """summarize_log against the model on the device's own log_read arrays: every output, bit for bit."""
    from fleetrl_amd import summarize_log
    from fleetrl_amd.evaluation import _core_of

    got = summarize_log(env, drop_last=drop_last, bins=bins, range=range, hist_ev=hist_ev)
    want, lg = _model(_core_of(env), drop_last=drop_last, bins=bins, lo=range[0], hi=range[1], hist_ev=hist_ev)
    for k in OUTPUTS:
        g = getattr(got, k)
        assert g.shape == want[k].shape and g.dtype == want[k].dtype, k
        np.testing.assert_array_equal(g, want[k], err_msg=k)
    np.testing.assert_array_equal(got.hist_edges, lm.hist_edges(bins, *range))
    return got, lg


# ---- the golden logs ---------------------------------------------------------------------------------------------------------------
def test_golden_replay_two_episodes_of_single_steps():
    """trace custom3_both_overload_log, as tests/test_vec_env_gpu.py replays it: the vec env has auto-reset into a third episode,
    so drop_last = 1 leaves the reference's rows, and 3 the rows its evaluation keeps (`iloc[0:-2]`)."""
    from fleetrl_amd import FleetVecEnv

    g = lm.load_fixture("custom3_both_overload_log", "trace_")
    venv = FleetVecEnv(g.cfg, g.E, tables=g.tables, start_rows=g.starts, extrema=g.extrema, start_range=(0, 0))
    venv.reset()
    for k in range(g.total):
        venv.step(g.actions[:, k])
    for drop, hist_ev in ((0, 0), (2, -1)):
        got, _ = _assert_equals_model(venv, drop_last=1 + drop, hist_ev=hist_ev)
        for e in range(g.E):
            lm.assert_meets_reference(_outputs(got), e, lm.reference_aggregates(g, e, drop, hist_ev=hist_ev), f"env {e} drop {drop}")
    venv.close()


def test_golden_replay_real_time_rows():
    """trace rttrace_ct3_both_rainflow_log (real_time: a row per table row passed, the envs' rings differ in length).  An env that
    has finished its recorded steps goes on stepping, so the rows past the reference's differ per env: one call per env."""
    from fleetrl_amd import FleetVecEnv

    g = lm.load_fixture("ct3_both_rainflow_log", "rttrace_")
    g.ep_rows = g.rc.episode_length * (60 // g.rc.minutes)
    cfg = dict(g.cfg)
    cfg["log_capacity"] = int(g.log_rows.max()) + 2 * g.ep_rows
    venv = FleetVecEnv(cfg, g.E, tables=g.tables, start_rows=g.starts, extrema=g.extrema, start_range=(0, 0))
    venv.reset()
    for k in range(int(g.n_steps.sum(axis=1).max())):
        venv.step(g.actions[:, k])
    pos = venv.core.batch.log_read(with_obs=False)["pos"]
    for e in range(g.E):
        extra = int(pos[e]) - int(g.log_rows[e])
        assert extra >= 0
        got, _ = _assert_equals_model(venv, drop_last=extra)
        lm.assert_meets_reference(_outputs(got), e, lm.reference_aggregates(g, e, 0), f"env {e}")
    venv.close()


def test_golden_replay_single_env_without_auto_reset():
    """trace pdtrace_lmd3_price_linear_log on a FleetEnv (reset, an episode, steps past done that log nothing, reset, an episode):
    the ring holds exactly the reference's rows."""
    from fleetrl_amd import FleetEnv

    g = lm.load_fixture("lmd3_price_linear_log", "pdtrace_")
    for e in range(g.E):
        env = FleetEnv(g.cfg, tables=g.tables, start_rows=g.starts[:, [e]], extrema=g.extrema, start_range=(0, 0))
        seg_end, k = np.cumsum(g.seg_steps[e]), 0
        for seg in range(3):
            if seg != 1:
                env.reset()
            while k < seg_end[seg]:
                env.step(g.actions[e, k])
                k += 1
        for drop in (0, 2):
            got, _ = _assert_equals_model(env, drop_last=drop)
            lm.assert_meets_reference(_outputs(got), 0, lm.reference_aggregates(g, e, drop), f"env {e} drop {drop}")
        env.close()


# ---- shapes --------------------------------------------------------------------------------------------------------------------
def _run(E, N, steps, how, *, log_capacity=0, real_time=False, seed=5):
    """A FleetVecEnv with the log on after reset() and `steps` steps: `how` = "uncontrolled" / "distributed" (the device-side
    rules, one launch) or "random" (host steps with uniform actions in [-1, 1], both signs and both Q8 carries)."""
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv
    from fleetrl_amd.policies import run_policy

    cfg = dict(bench_config(E, N, "ct"), log_data=True, real_time=real_time)
    if log_capacity:
        cfg["log_capacity"] = log_capacity
    venv = FleetVecEnv(cfg, E, tables=_tables(N), seed=seed)
    venv.reset()
    if how == "random":
        rng = np.random.default_rng(seed)
        for _ in range(steps):
            a = rng.uniform(-1.0, 1.0, size=(E, N)).astype(np.float32)
            a[rng.random((E, N)) < 0.15] = 0.0  # (a bin edge, and the charging side of the carry)
            venv.step(a)
    elif steps:
        run_policy(venv.core.batch, how, steps, chunk=96)
    return venv


SHAPES = [
    # E, N, steps, how, log_capacity, summary keywords; window rows = steps + 1 (the reset row) unless the ring has wrapped
    pytest.param(1, 1, 0, "uncontrolled", 0, {}, id="E1-N1-1row"),
    pytest.param(3, 3, 62, "distributed", 0, dict(hist_ev=-1), id="E3-N3-63rows-every-ev"),
    pytest.param(3, 64, 63, "random", 0, dict(hist_ev=63), id="E3-N64-64rows-last-ev"),
    pytest.param(130, 3, 64, "uncontrolled", 0, dict(range=(-0.5, 0.5), bins=7), id="E130-N3-65rows-narrow-range"),
    pytest.param(3, 65, 130, "random", 0, dict(drop_last=2, hist_ev=64, bins=256), id="E3-N65-129rows-drop2"),
    pytest.param(3, 65, 120, "random", 50, dict(hist_ev=-1, range=(-0.25, 1.0)), id="E3-N65-cap50-wrapped"),
    pytest.param(2, 130, 150, "random", 100, dict(hist_ev=129), id="E2-N130-cap100-wrapped"),
    pytest.param(130, 130, 70, "distributed", 0, dict(hist_ev=-1, drop_last=1), id="E130-N130-71rows"),
]


@pytest.mark.parametrize("E,N,steps,how,cap,kw", SHAPES)
def test_summary_equals_the_model_bit_for_bit(E, N, steps, how, cap, kw):
    venv = _run(E, N, steps, how, log_capacity=cap)
    got, lg = _assert_equals_model(venv, **kw)
    ring = cap or venv.core.batch.log_capacity()
    want_rows = max(min(steps + 1, ring) - kw.get("drop_last", 0), 0)
    assert (lg["pos"] == steps + 1).all() and (got.rows == want_rows).all()
    if cap:
        assert steps + 1 > cap and cap % 64  # wrapped, and no multiple of the block
    if how == "random":
        act = lg["ev"][:, :, 0]
        assert (act < 0).any() and (act > 0).any() and (act == 0).any()
        if "range" in kw:
            assert got.hist.sum() < (got.rows * (N if kw.get("hist_ev", 0) < 0 else 1)).sum()  # some actions are left out
    if want_rows >= 97:
        assert (got.deg_rows >= 1).all() and np.abs(got.deg_sum).sum() > 0  # a day's rows hold a 14:45 row
    venv.close()


def test_real_time_rings_of_different_length():
    venv = _run(3, 3, 12, "random", real_time=True)
    got, lg = _assert_equals_model(venv, hist_ev=-1)
    # every table row passed is logged: an env that skipped rows has more rows than the reset row and its 12 steps
    assert len(set(lg["pos"].tolist())) > 1 and (lg["pos"] >= 13).all() and lg["pos"].max() > 13
    _assert_equals_model(venv, drop_last=int(lg["pos"].min()), hist_ev=1)  # one env's window is empty, the others' are not
    venv.close()


def test_empty_windows():
    venv = _run(3, 65, 9, "random")
    got, _ = _assert_equals_model(venv, drop_last=11)  # more than pos = 10
    assert not got.scal.any() and np.isnan(got.soh_last).all() and not got.hist.any() and not got.prof_cnt.any()
    venv.core.clear_log()
    got, lg = _assert_equals_model(venv, hist_ev=-1)
    assert not lg["pos"].any() and not got.scal.any() and np.isnan(got.soh_last).all()
    assert not got.deg_sum.any() and not got.prof_sum.any() and not got.prof_cnt.any() and not got.hist.any()
    venv.step(np.zeros((3, 65), dtype=np.float32))  # the ring goes on from row 0
    got, _ = _assert_equals_model(venv)
    assert (got.rows == 1).all()
    venv.close()


def test_against_get_log_across_the_lane_boundary():
    """N = 65: the last EV's charging energy carries over from the first 64.  Aggregates of get_log()'s DataFrames -- the host
    route the reference's logger pins -- at the per-row tolerances of tests/test_vec_env_gpu.py."""
    venv = _run(3, 65, 128, "random")
    got, _ = _assert_equals_model(venv, hist_ev=64)
    frames = venv.env_method("get_log")
    mps, S = int(venv.core.rc.minutes), 1440 // int(venv.core.rc.minutes)
    for e, f in enumerate(frames):
        n = len(f)
        assert got.rows[e] == n == 129
        for name, col in (("reward", "Reward"), ("cashflow", "Cashflow"), ("penalty", "Penalties"), ("overload", "Grid overloading"),
                          ("soc_violation", "SOC violation")):
            np.testing.assert_allclose(getattr(got, name)[e], f[col].values.astype(float).sum(), rtol=lm.RTOL, atol=lm.ATOL[name] * n,
                                       err_msg=col)
        assert got.violations[e] == int((f["SOC violation"].values.astype(float) > 0).sum())
        deg = np.stack([np.broadcast_to(np.asarray(x, dtype=np.float64), (65,)) for x in f["Degradation"]])
        np.testing.assert_allclose(got.deg_sum[e], deg.sum(axis=0), rtol=lm.RTOL_DEG, atol=lm.ATOL["deg"] * n)
        np.testing.assert_allclose(got.soh_last[e], np.asarray(f["SOH"].iloc[-1], dtype=np.float64), rtol=lm.RTOL, atol=0)
        energy = np.stack([np.asarray(x, dtype=np.float64) for x in f["Charging energy"]])
        assert np.abs(energy[:, 64]).sum() > 0
        t = f["Time"].dt.hour.values * 60 + f["Time"].dt.minute.values
        slot = t // mps
        for s in range(S):
            rows = slot == s
            assert got.prof_cnt[e, s] == rows.sum()
            np.testing.assert_allclose(got.prof_sum[e, s], energy[rows].mean(axis=1).sum(), rtol=lm.RTOL,
                                       atol=lm.ATOL["charge"] * max(int(rows.sum()), 1))
        act = np.stack([np.asarray(x, dtype=np.float64) for x in f["Action"]])[:, 64]
        np.testing.assert_array_equal(got.hist[e], np.histogram(act, bins=50, range=(-1.0, 1.0))[0])
    venv.close()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_leave_the_outputs_untouched():
    import torch

    from bench import bench_config
    from fleetrl_amd import FleetVecEnv, _capi
    from fleetrl_amd.batch import FleetHipError

    E, N = 3, 3
    venv = _run(E, N, 5, "uncontrolled")
    b = venv.core.batch
    dev = torch.device("cuda", 0)
    bufs = {"scal": torch.full((E, 8), -7.0, device=dev, dtype=torch.float64), "deg_sum": torch.full((E, N), -7.0, device=dev, dtype=torch.float64),
            "soh_last": torch.full((E, N), -7.0, device=dev, dtype=torch.float64), "prof_sum": torch.full((E, 96), -7.0, device=dev, dtype=torch.float64),
            "prof_cnt": torch.full((E, 96), -7, device=dev, dtype=torch.int32), "hist": torch.full((E, 256), -7, device=dev, dtype=torch.int32)}
    torch.cuda.synchronize()

    def args(**kw):
        a = _capi.FleetLogSummaryArgs()
        a.drop_last, a.bins, a.hist_ev, a.lo, a.hi = 0, 50, 0, -1.0, 1.0
        for k, t in bufs.items():
            setattr(a, k, t.data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(handle, a, size=None):
        rc = b.lib.fleet_log_summary_dev(handle, None if a is None else C.byref(a), C.sizeof(_capi.FleetLogSummaryArgs) if size is None else size)
        assert rc == _capi.ERR_INVALID
        b.synchronize()
        torch.cuda.synchronize()
        for k, t in bufs.items():
            assert bool((t == -7).all()), k

    refused(b.h, None)
    refused(b.h, args(), size=C.sizeof(_capi.FleetLogSummaryArgs) - 8)
    refused(b.h, args(), size=C.sizeof(_capi.FleetLogSummaryArgs) + 8)
    refused(b.h, args(scal=None))
    refused(b.h, args(drop_last=-1))
    for bins in (0, -3, 257):
        refused(b.h, args(bins=bins))
    for lo, hi in ((1.0, 1.0), (1.0, -1.0), (float("nan"), 1.0), (-1.0, float("nan"))):
        refused(b.h, args(lo=lo, hi=hi))
    for ev in (-2, N, N + 64):
        refused(b.h, args(hist_ev=ev))
    assert "hist_ev" in b.lib.fleet_last_error(b.h).decode()
    with pytest.raises(FleetHipError):
        b.log_summary(bufs["scal"].data_ptr(), drop_last=-1)
    # the log being off
    off = FleetVecEnv(bench_config(E, N, "ct"), E, tables=_tables(N), seed=5)
    off.reset()
    refused(off.core.batch.h, args())
    off.close()
    # bins is only read with a histogram: a call without one is served, and the refused ones before it left no trace
    a = args(bins=0, hist=None)
    assert b.lib.fleet_log_summary_dev(b.h, C.byref(a), C.sizeof(a)) == _capi.OK
    b.synchronize()
    assert bool((bufs["scal"][:, 0] == 6).all()) and bool((bufs["hist"] == -7).all())
    venv.close()


def test_time_of_day_profile_is_refused_on_an_irregular_grid():
    """Trace rttrace_lmd1_both_irregular (7- and 8-minute rows): the time-of-day slot is not defined there, so prof_* is refused
    and the rest is served (summarize_log passes no profile then)."""
    import torch

    from fleetrl_amd import FleetVecEnv, _capi, summarize_log

    g = load_rt_trace("lmd1_both_irregular")
    cfg = dict(g.cfg, log_data=True)
    venv = FleetVecEnv(cfg, g.E, tables=g.tables, start_rows=g.starts, extrema=g.extrema, start_range=(0, 0))
    venv.reset()
    for k in range(5):
        venv.step(g.actions[:, k])
    b = venv.core.batch
    dev = torch.device("cuda", 0)
    scal = torch.full((g.E, 8), -7.0, device=dev, dtype=torch.float64)
    prof = torch.full((g.E, 1440), -7.0, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    a = _capi.FleetLogSummaryArgs()
    a.bins, a.hist_ev, a.lo, a.hi, a.scal, a.prof_sum = 1, -1, -1.0, 1.0, scal.data_ptr(), prof.data_ptr()
    assert b.lib.fleet_log_summary_dev(b.h, C.byref(a), C.sizeof(a)) == _capi.ERR_INVALID
    b.synchronize()
    assert bool((scal == -7).all()) and bool((prof == -7).all())
    s = summarize_log(venv)
    assert s.prof_sum is None and s.prof_cnt is None and (s.rows > 5).all()
    _assert_equals_model_without_profile(venv, s)
    venv.close()


def _assert_equals_model_without_profile(venv, got):
    want, _ = _model(venv.core, hist_ev=0)
    for k in ("scal", "deg_sum", "soh_last", "hist"):
        np.testing.assert_array_equal(getattr(got, k), want[k], err_msg=k)


# ---- evaluate_strategies -----------------------------------------------------------------------------------------------------------
def test_evaluate_strategies_same_episodes_and_the_seven_rows():
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv, compare, evaluate_strategies
    from fleetrl_amd.evaluation import TABLE_ROWS
    from fleetrl_amd.policies import run_policy

    E, N, steps = 4, 3, 95  # one 24-hour episode: the reset row and every step but the one that ends it
    cfg = dict(bench_config(E, N, "ct"), episode_length=24)
    names = ("uncontrolled", "distributed", "night", "lp")
    out = evaluate_strategies(cfg, names, E, steps, tables=_tables(N), seed=11)
    assert tuple(out) == names
    for s in out.values():
        assert (s.rows == steps + 1).all() and s.steps_per_hour == 4.0
        assert s.prof_cnt.sum() == E * (steps + 1) and s.hist.sum() <= E * (steps + 1)
    assert out["uncontrolled"].hist.sum() == E * (steps + 1)
    # the uncontrolled rule's own reward sum, from a twin env built the same way (the reset row adds nothing)
    twin = FleetVecEnv(dict(cfg, log_data=True), E, tables=_tables(N), seed=11)
    twin.reset()
    starts = twin.core.batch.get("start_idx").copy()
    _o, rsum, _d = run_policy(twin.core.batch, "uncontrolled", steps)
    np.testing.assert_allclose(out["uncontrolled"].reward, rsum, rtol=1e-9, atol=0)
    twin.close()
    assert len(set(starts.tolist())) > 1  # the envs' episodes differ; every strategy saw the same ones
    first_slot = (np.asarray(_tables(N).hour)[starts].astype(int) * 60 + np.asarray(_tables(N).minute)[starts]) // 15
    # (96 rows fill every slot of the day once, whenever they begin: the first rows alone show where each env's episode began)
    first = evaluate_strategies(cfg, names, E, steps, tables=_tables(N), seed=11, drop_last=steps)
    onehot = np.zeros((E, 96), dtype=np.int32)
    onehot[np.arange(E), first_slot] = 1
    for s in first.values():
        assert (s.rows == 1).all() and not s.reward.any()  # the reset row
        np.testing.assert_array_equal(s.prof_cnt, onehot)
    res = compare(out["lp"], out["uncontrolled"], env=2)
    assert tuple(res["table"]) == TABLE_ROWS and len(TABLE_ROWS) == 7
    assert res["table"]["Reward"] == (out["lp"].reward[2], out["uncontrolled"].reward[2])
    assert res["table"]["# Violations"][1] == int(out["uncontrolled"].violations[2])
    assert res["table"]["SOH"][0] == float(np.round(out["lp"].soh_last[2].mean(), 5))
    assert res["power"]["RL"].shape == (96,) and np.isfinite(res["power"]["benchmark charging"]).all()
    np.testing.assert_array_equal(res["power"]["RL"], out["lp"].prof_sum[2] / out["lp"].prof_cnt[2] * 4.0)
    if res["frame"] is not None:
        assert list(res["frame"]["Category"]) == list(TABLE_ROWS) and list(res["frame"].columns) == ["Category", "RL-based charging",
                                                                                                      "benchmark charging"]
    mean = compare(out["lp"], out["uncontrolled"], env="mean")
    np.testing.assert_allclose(mean["table"]["Cashflow"][0], out["lp"].cashflow.mean(), rtol=1e-15)


def test_evaluate_strategies_runs_the_committed_agent():
    """The shipped PPO agent (tests/golden/ppo_lmd_arbitrage_policy.npz, 45 observations -> 1 action) beside the uncontrolled rule."""
    from bench import bench_config
    from fleetrl_amd import DevicePolicy, evaluate_strategies
    from fleetrl_amd.synth import synth_tables

    with np.load(os.path.join(lm.ROOT, "tests", "golden", "ppo_lmd_arbitrage_policy.npz")) as z:
        policy = DevicePolicy.from_state_dict({k: z[k] for k in z.files})
    E, steps = 4, 40
    cfg = dict(bench_config(E, 1, "lmd"), episode_length=24)
    out = evaluate_strategies(cfg, ("uncontrolled", policy), E, steps, tables=synth_tables("lmd", 1), seed=2)
    assert tuple(out) == ("uncontrolled", "policy")
    for s in out.values():
        assert (s.rows == steps + 1).all()
    np.testing.assert_array_equal(out["policy"].prof_cnt, out["uncontrolled"].prof_cnt)
    assert np.isfinite(out["policy"].scal).all() and out["policy"].hist.sum() == E * (steps + 1)
    policy.close()
