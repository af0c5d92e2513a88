"""The last stage of the reference's workflow, `agent_eval/basic_evaluation.py`, at fleet scale: the numbers of
`BasicEvaluation.compare` and `plot_action_dist` from the device-side data log, reduced ON THE DEVICE.

`FleetCore.get_log()` copies the whole ring to the host and builds one DataFrame per env -- right for three envs, hopeless for
thousands.  `summarize_log` runs `fleet_log_summary_dev` (fleetrl_amd/csrc/fleet_logsum.hip: two launches over the ring) and reads
back a few kilobytes per env: the sums of reward, cashflow, penalties, overloading and SOC violation, the violation count, the
degradation per EV, the last SoH, the mean charging power per time of day and the action histogram.  `compare` lays two such
summaries side by side as the reference's `total_results` table; `evaluate_strategies` is the reference's `evaluate_agent` plus
its benchmark runs, every strategy on its own env over the same episodes.  The plots of agent_eval/ stay out.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _capi

__all__ = ["LogSummary", "summarize_log", "compare", "evaluate_strategies", "TABLE_ROWS"]

TABLE_ROWS = ("Reward", "Cashflow", "Average degradation per EV", "Overloading", "SOC violation", "# Violations", "SOH")


@dataclass
class LogSummary:
    """What `fleet_log_summary_dev` writes, per env: NumPy arrays, or torch tensors on the env's device (`as_torch=True`).
    scal [E,8]: the columns of `_capi.LOG_SUMMARY_SCALARS` (also as properties); deg_sum, soh_last [E,N]; prof_sum f64 /
    prof_cnt i32 [E,S] over the S = 1440 / minutes_per_step time-of-day slots (None on an irregular time grid); hist i32
    [E,bins] with `hist_edges` [bins + 1]."""
    scal: object
    deg_sum: object
    soh_last: object
    prof_sum: object
    prof_cnt: object
    hist: object
    hist_edges: np.ndarray
    steps_per_hour: float
    price_multiplier: float
    drop_last: int = 0
    hist_ev: int = 0

    def _col(self, name):
        return self.scal[:, _capi.LOG_SUMMARY_SCALARS.index(name)]

    rows = property(lambda self: self._col("rows"))
    reward = property(lambda self: self._col("reward"))
    cashflow = property(lambda self: self._col("cashflow"))
    penalty = property(lambda self: self._col("penalty"))
    overload = property(lambda self: self._col("overload"))
    soc_violation = property(lambda self: self._col("soc_violation"))
    violations = property(lambda self: self._col("violations"))
    deg_rows = property(lambda self: self._col("deg_rows"))

    def numpy(self) -> "LogSummary":
        """The same summary in NumPy arrays (a device synchronisation when it holds tensors)."""
        conv = lambda x: x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()  # noqa: E731
        return LogSummary(conv(self.scal), conv(self.deg_sum), conv(self.soh_last), conv(self.prof_sum), conv(self.prof_cnt),
                          conv(self.hist), self.hist_edges, self.steps_per_hour, self.price_multiplier, self.drop_last, self.hist_ev)

    def power_profile(self):
        """[E,S] mean charging power per time of day in kW: prof_sum / prof_cnt * steps_per_hour (NaN where a slot has no row)."""
        s = self.numpy()
        if s.prof_sum is None:
            raise ValueError("no time-of-day profile: the env's tables are an irregular time grid")
        with np.errstate(invalid="ignore", divide="ignore"):
            return s.prof_sum / s.prof_cnt * s.steps_per_hour


def _core_of(env):
    """The FleetCore behind a FleetCore, FleetVecEnv, FleetVectorEnv, FleetEnv or FleetVecNormalize."""
    for obj in (env, getattr(env, "core", None), getattr(getattr(env, "venv", None), "core", None)):
        if obj is not None and hasattr(obj, "batch") and hasattr(obj, "rc"):
            return obj
    raise TypeError(f"no FleetCore behind {type(env).__name__}")


def summarize_log(env, *, drop_last: int = 0, bins: int = 50, range=(-1.0, 1.0), hist_ev: int = 0, as_torch: bool = False) -> LogSummary:
    """The env's data log (`log_data` on) reduced on the device.  `env`: a FleetCore, FleetVecEnv, FleetEnv or FleetVecNormalize.
    The window of an env is its kept rows without the newest `drop_last` (the reference evaluates `log_RL.iloc[0:-2]`; an
    auto-resetting vec env has logged the reset row of the episode after the last one, which the reference never has).  The
    histogram is `plot_action_dist`'s: `bins` = 50 bins over `range`, of the actions of EV `hist_ev` (the reference's `x[0]`; -1:
    every EV).  Ordered behind everything the env has enqueued; `as_torch=True` leaves the tensors on the device and does not
    synchronise."""
    import torch

    core = _core_of(env)
    batch = core.batch
    if not core.log_data:
        raise _capi.FleetHipError(_capi.ERR_INVALID, "summarize_log: the data log is off (log_data = False)")
    E, N = batch.E, batch.N
    dev = torch.device("cuda", batch.device)
    batch.use_torch_stream(dev)
    regular = "irregular" not in getattr(core.tables, "meta", {})
    mps = int(core.rc.minutes)
    S = 1440 // mps if regular else 0
    f64 = dict(device=dev, dtype=torch.float64)
    scal, deg, soh = torch.empty((E, 8), **f64), torch.empty((E, N), **f64), torch.empty((E, N), **f64)
    psum = torch.empty((E, S), **f64) if S else None
    pcnt = torch.empty((E, S), device=dev, dtype=torch.int32) if S else None
    hist = torch.empty((E, int(bins)), device=dev, dtype=torch.int32)
    lo, hi = float(range[0]), float(range[1])
    batch.log_summary(scal.data_ptr(), deg_sum_ptr=deg.data_ptr(), soh_last_ptr=soh.data_ptr(),
                      prof_sum_ptr=None if psum is None else psum.data_ptr(), prof_cnt_ptr=None if pcnt is None else pcnt.data_ptr(),
                      hist_ptr=hist.data_ptr(), drop_last=drop_last, bins=bins, lo=lo, hi=hi, hist_ev=hist_ev)
    edges = np.empty(int(bins) + 1)
    edges[:-1] = lo + np.arange(int(bins)) * ((hi - lo) / int(bins))
    edges[-1] = hi
    out = LogSummary(scal, deg, soh, psum, pcnt, hist, edges, 60.0 / mps, float(core.rc.price_multiplier), int(drop_last), int(hist_ev))
    return out if as_torch else out.numpy()


def _table_column(s: LogSummary, env):
    s = s.numpy()
    cols = [s.reward, s.cashflow, s.deg_sum.mean(axis=1), s.overload, s.soc_violation, s.violations, s.soh_last.mean(axis=1)]
    if isinstance(env, str):
        if env != "mean":
            raise ValueError("env: an env index or 'mean'")
        vals = [float(np.mean(c)) for c in cols]
    else:
        vals = [float(c[int(env)]) for c in cols]
        vals[5] = int(vals[5])
    vals[2], vals[6] = float(np.round(vals[2], 5)), float(np.round(vals[6], 5))
    return vals


def compare(rl: LogSummary, benchmark: LogSummary, env=0) -> dict:
    """`BasicEvaluation.compare` (agent_eval/basic_evaluation.py:94-155) without its plot, for env `env` of both summaries
    (`env="mean"`: the table's entries averaged over the envs).
      "table"    {row: (rl, benchmark)} for the rows of TABLE_ROWS: the sums of Reward, Cashflow, Grid overloading and SOC
                 violation, `round(mean over the EVs of the summed degradation, 5)`, the number of rows with a SOC violation,
                 `round(mean over the EVs of the last SoH, 5)`
      "frame"    the same as the reference's `total_results` DataFrame (columns Category, RL-based charging, benchmark charging),
                 or None without pandas
      "power"    {"RL": [S], "benchmark charging": [S]}: the mean charging power per time of day in kW, prof_sum / prof_cnt *
                 steps_per_hour.  The reference multiplies the mean energy per step by a hard-coded 4, which is steps_per_hour at
                 its 15-minute resolution; here the factor follows the env's resolution."""
    a, b = _table_column(rl, env), _table_column(benchmark, env)
    table = {name: (x, y) for name, x, y in zip(TABLE_ROWS, a, b)}
    try:
        import pandas as pd

        frame = pd.DataFrame({"Category": list(TABLE_ROWS), "RL-based charging": a, "benchmark charging": b})
    except ImportError:  # pragma: no cover - depends on the installation
        frame = None

    def curve(s):
        p = s.power_profile()
        if not isinstance(env, str):
            return p[int(env)]
        filled = ~np.isnan(p)  # the mean over the envs that have a row in the slot; NaN where none has
        with np.errstate(invalid="ignore"):
            return np.where(filled, p, 0.0).sum(axis=0) / filled.sum(axis=0)

    power = None
    if rl.prof_sum is not None and benchmark.prof_sum is not None:
        power = {"RL": curve(rl), "benchmark charging": curve(benchmark)}
    return {"table": table, "frame": frame, "power": power}


STRATEGIES = ("uncontrolled", "distributed", "night", "lp", "policy")


def _run_agent(venv, agent, normalizer, n_steps: int):
    """The policy loop on the device: forward, step, nothing read back.  Returns what has to be closed afterwards."""
    import torch

    from .vec_normalize import FleetVecNormalize

    batch = venv.core.batch
    dev = torch.device("cuda", batch.device)
    E = batch.E
    obs = torch.empty((E, agent.obs_dim), device=dev, dtype=torch.float32)
    act = torch.empty((E, agent.act_dim), device=dev, dtype=torch.float32)
    if normalizer is not None:  # statistics frozen, rewards raw: the log holds the env's own rewards either way
        stepper = FleetVecNormalize.load(normalizer, venv)
        stepper.training = False
        stepper.norm_reward = False
        stepper.reset_torch(obs_out=obs)
    else:
        stepper = venv
        batch.use_torch_stream(dev)
        venv._torch_stream = torch.cuda.current_stream(dev).cuda_stream
        venv.core.clear_start_overrides()
        batch.reset_dev(obs.data_ptr())
    for _ in range(n_steps):
        agent.act(obs, out=act)
        stepper.step_torch(act, obs_out=obs)
    batch.check_errors()
    return stepper


def evaluate_strategies(env_config, strategies, n_envs: int, n_steps: int, *, policy=None, normalizer=None, seed: int = 0, tables=None,
                        start_rows=None, drop_last: int = 0, bins: int = 50, range=(-1.0, 1.0), hist_ev: int = 0, device: int = 0,
                        **env_kw) -> dict:
    """The reference's `evaluate_agent` and its benchmark runs (benchmarking/*.py) over `n_envs` fleets at once: every strategy runs
    `n_steps` steps on an env of its own with `log_data` on and a ring that loses no row, all built from the same config, seed and
    start schedule -- so all see the same episodes -- and its log is summarised on the device.  -> {name: LogSummary}.
    strategies: any of "uncontrolled", "distributed", "night" (fleetrl_amd.policies.run_policy), "lp" (run_linear_optimization:
    perfect foresight over the `n_steps` rows, which must lie within one episode) and "policy" or a DevicePolicy itself (`policy=`
    gives the agent for the name; `normalizer=` the path of a FleetVecNormalize.save file whose frozen statistics the observations
    go through, None: raw observations).  `tables`, `start_rows` and further keywords go to FleetVecEnv.  A real_time config needs
    its own `log_capacity` (an agent step logs every table row it passes)."""
    from .config import resolve_config
    from .lp_benchmark import run_linear_optimization
    from .policies import night_schedule, run_policy
    from .vec_env import FleetVecEnv

    cfg = dict(env_config)
    cfg["log_data"] = True
    n_steps = int(n_steps)
    if not cfg.get("log_capacity"):
        if cfg.get("real_time"):
            raise ValueError("evaluate_strategies: a real_time config needs log_capacity (rows per env the run may log)")
        rc = resolve_config(cfg)
        ep = max(int(rc.episode_length) * (60 // int(rc.minutes)), 1)
        cfg["log_capacity"] = n_steps + n_steps // ep + 2  # a row per step and a reset row per episode begun
    out = {}
    for strat in strategies:
        name = strat if isinstance(strat, str) else "policy"
        agent = policy if isinstance(strat, str) else strat
        if name not in STRATEGIES:
            raise ValueError(f"unknown strategy {strat!r}: one of {STRATEGIES} or a DevicePolicy")
        if name == "policy" and agent is None:
            raise ValueError("the 'policy' strategy needs policy=")
        venv = FleetVecEnv(cfg, int(n_envs), tables=tables, seed=seed, start_rows=start_rows, device=device, **env_kw)
        closer = venv
        try:
            batch = venv.core.batch
            if name == "policy":
                closer = _run_agent(venv, agent, normalizer, n_steps)
            else:
                batch.reset()
                if name == "lp":
                    run_linear_optimization(venv, n_steps)
                elif name == "night":
                    p = venv.core.params
                    run_policy(batch, "night", n_steps, night=night_schedule(
                        venv.core.tables, target_soc=p.target_soc, init_battery_cap=p.init_battery_cap, charging_eff=p.charging_eff,
                        evse_power=p.evse_power))
                else:
                    run_policy(batch, name, n_steps)
            if batch.log_dropped():
                raise _capi.FleetHipError(_capi.ERR_STATE, f"evaluate_strategies: the log ring of strategy {name!r} has lost rows")
            out[name] = summarize_log(venv, drop_last=drop_last, bins=bins, range=range, hist_ev=hist_ev)
        finally:
            closer.close()  # (a FleetVecNormalize closes the env under it)
    return out


