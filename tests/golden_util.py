"""Shared helpers for the parity tests: load a committed golden trace (tests/golden/trace_*.npz, produced from
the unmodified reference by oracle/gen_golden.py) and replay it on an engine.

An "engine" is anything with reset() / step(actions) / get(name) / set_start_schedule(starts) -- the CPU oracle
(oracle.fleet_oracle.OracleBatch) or the HIP product (fleetrl_amd.batch.FleetBatch).
"""
from __future__ import annotations

import glob
import json
import os
from types import SimpleNamespace

import numpy as np

from fleetrl_amd.config import resolve_config
from fleetrl_amd.params import make_params, time_features
from fleetrl_amd.prestage import FleetTables

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRACE_NAMES = sorted(os.path.basename(p)[len("trace_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN_DIR, "trace_*.npz")))


RT_TRACE_NAMES = sorted(os.path.basename(p)[len("rttrace_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN_DIR, "rttrace_*.npz")))

# The reference's input CSVs the pre-stager tests read, stored xz-compressed (byte-identical once unpacked), and its config.json.
# The reference ships each single-EV schedule under two names; the copies are made from the one stored file.
INPUTS_DIR = os.path.join(GOLDEN_DIR, "inputs")
_INPUT_ALIASES = {"ct_sched_single.csv": "1_ct.csv", "lmd_sched_single.csv": "1_lmd.csv", "ut_sched_single.csv": "1_ut.csv"}


def unpack_reference_inputs(dest: str) -> str:
    """Write the stored input CSVs into `dest` under the reference's file names; returns `dest` (a `data_path`)."""
    import lzma
    import shutil

    for f in sorted(os.listdir(INPUTS_DIR)):
        if f.endswith(".csv.xz"):
            with lzma.open(os.path.join(INPUTS_DIR, f)) as src, open(os.path.join(dest, f[:-len(".xz")]), "wb") as dst:
                shutil.copyfileobj(src, dst)
    for alias, f in _INPUT_ALIASES.items():
        shutil.copyfile(os.path.join(dest, f), os.path.join(dest, alias))
    return dest


def reference_base_config(data_path: str) -> dict:
    """oracle.ref_harness.base_config() on the stored config.json, reading its inputs from `data_path`."""
    from oracle import ref_harness

    return ref_harness.base_config(os.path.join(INPUTS_DIR, "config.json"), data_path)


def load_trace(name: str, prefix: str = "trace_") -> SimpleNamespace:
    z = np.load(os.path.join(GOLDEN_DIR, f"{prefix}{name}.npz"), allow_pickle=False)
    g = SimpleNamespace(**{k: z[k] for k in z.files})
    g.name = name
    g.cfg = json.loads(str(z["cfg_json"]))
    g.rc = resolve_config(g.cfg)
    dates = z["tab_dates"].astype("datetime64[s]")
    day = dates.astype("datetime64[D]")
    hours = ((dates - day) // np.timedelta64(3600, "s")).astype(np.int64)
    minute = ((dates - dates.astype("datetime64[h]")) // np.timedelta64(60, "s")).astype(np.int64)
    month = dates.astype("datetime64[M]").astype(np.int64) % 12 + 1
    weekday = (day.astype(np.int64) + 3) % 7
    g.tables = FleetTables(
        dates=dates, there=z["tab_there"], time_left=z["tab_time_left"].astype(np.float32),
        soc_on_return=z["tab_soc_on_return"], consumption=np.zeros_like(z["tab_soc_on_return"]),
        delu=z["tab_delu"], tariff=z["tab_tariff"], prc=z["tab_prc"], trc=z["tab_trc"], load=z["tab_load"], pv=z["tab_pv"],
        hour=hours.astype(np.uint8), minute=minute.astype(np.uint8), month=month.astype(np.uint8),
        weekday=weekday.astype(np.uint8), minutes_per_step=g.rc.minutes,
    )
    g.extrema = {k[len("sc_ext_"):]: float(z[k]) for k in z.files if k.startswith("sc_ext_")}
    g.E, g.total, g.N = g.actions.shape
    g.episodes = g.starts.shape[0]
    g.ep_steps = g.total // g.episodes
    g.time_feat = time_features(g.tables)
    return g


def params_for(g, num_envs=None, auto_reset=True):
    return make_params(g.rc, g.tables, g.E if num_envs is None else num_envs, auto_reset=auto_reset,
                       extrema=g.extrema, start_range=(0, 0))


def rel_err(a, b):
    """max |a-b| / max(|b|, 1e-3): relative error with an absolute floor, so that a float64 residue of 1e-17 where the
    reference has an exact 0 (e.g. SOC after a full discharge) does not read as a huge relative error."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3))) if a.size else 0.0


def replay(g, engine, *, float_rtol=1e-9, obs_exact=True, check_sei=True, env_map=None):
    """Drive `engine` (E_engine envs) with the golden actions/starts; env i of the engine replays golden env
    env_map[i] (default i % g.E).  Asserts bit-exact flags/indices, float32 obs (exact or 1e-5 rel), and
    float64 state within `float_rtol` relative.  Returns the largest relative errors seen."""
    Ee = engine.E
    env_map = np.arange(Ee) % g.E if env_map is None else np.asarray(env_map)
    engine.set_start_schedule(g.starts[:, env_map])
    worst = dict(obs=0.0, reward=0.0, soc=0.0, soh=0.0, cashflow=0.0, obs_words=0, obs_words_exact=0)
    obs = engine.reset()
    np.testing.assert_array_equal(engine.get("start_idx"), g.starts[0, env_map])

    def cmp_obs(got, want, what):
        if obs_exact:
            np.testing.assert_array_equal(got, want, err_msg=what)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=what)
        worst["obs"] = max(worst["obs"], rel_err(got, want))
        worst["obs_words"] += int(np.size(want))  # how many float32 observation words are the reference's, bit for bit
        worst["obs_words_exact"] += int(np.count_nonzero(np.asarray(got, dtype=np.float32).view(np.uint32) ==
                                                         np.asarray(want, dtype=np.float32).view(np.uint32)))

    cmp_obs(obs, g.reset_obs[env_map, 0], "reset obs, episode 0")
    np.testing.assert_allclose(engine.get("soc"), g.reset_soc[env_map, 0], rtol=float_rtol, atol=0)
    k = 0
    for ep in range(g.episodes):
        for s in range(g.ep_steps):
            obs, rew, done, term = engine.step(g.actions[env_map, k])
            last = s == g.ep_steps - 1
            np.testing.assert_array_equal(done, g.done[env_map, k], err_msg=f"done flag, step {k}")
            np.testing.assert_allclose(rew, g.reward[env_map, k], rtol=float_rtol, atol=1e-12, err_msg=f"reward, step {k}")
            worst["reward"] = max(worst["reward"], rel_err(rew, g.reward[env_map, k]))
            np.testing.assert_allclose(engine.get("cashflow"), g.cashflow[env_map, k], rtol=float_rtol, atol=1e-13,
                                       err_msg=f"cashflow, step {k}")
            if not last:
                cmp_obs(obs, g.obs[env_map, k], f"obs, step {k}")
                np.testing.assert_array_equal(engine.get("time_idx"), g.time_idx[env_map, k], err_msg=f"time row, step {k}")
                np.testing.assert_array_equal(engine.get("hours_left").astype(np.float64), g.hours_left[env_map, k],
                                              err_msg=f"hours_left, step {k}")
                np.testing.assert_allclose(engine.get("soc"), g.soc[env_map, k], rtol=float_rtol, atol=1e-15, err_msg=f"soc, step {k}")
                np.testing.assert_allclose(engine.get("soh"), g.soh[env_map, k], rtol=float_rtol, atol=0, err_msg=f"soh, step {k}")
                np.testing.assert_allclose(engine.get("soc_deg"), g.soc_deg[env_map, k], rtol=float_rtol, atol=1e-15)
                np.testing.assert_array_equal(engine.get("target_soc"), g.target_soc[env_map, k])
                worst["soc"] = max(worst["soc"], rel_err(engine.get("soc"), g.soc[env_map, k]))
                worst["soh"] = max(worst["soh"], rel_err(engine.get("soh"), g.soh[env_map, k]))
            else:
                # vec-env semantics: terminal observation is reported separately, obs is the next episode's reset obs
                cmp_obs(term, g.terminal_obs[env_map, ep], f"terminal obs, episode {ep}")
                if check_sei and g.rc.deg_mode == 2:
                    np.testing.assert_array_equal(engine.get("rf_len"), g.rf_len[env_map, ep], err_msg=f"rainflow_length, episode {ep}")
                    np.testing.assert_allclose(engine.get("fd_cyc"), g.fd_cyc[env_map, ep], rtol=1e-9, atol=1e-18)
                    np.testing.assert_allclose(engine.get("fd_cal"), g.fd_cal[env_map, ep], rtol=1e-9, atol=1e-18)
                    np.testing.assert_allclose(engine.get("sei_l"), g.sei_l[env_map, ep], rtol=1e-9, atol=1e-18)
                if ep + 1 < g.episodes:
                    cmp_obs(obs, g.reset_obs[env_map, ep + 1], f"reset obs, episode {ep + 1}")
                    np.testing.assert_array_equal(engine.get("start_idx"), g.starts[ep + 1, env_map])
                    np.testing.assert_allclose(engine.get("soc"), g.reset_soc[env_map, ep + 1], rtol=float_rtol, atol=0)
                    if g.rc.aux:
                        np.testing.assert_allclose(engine.dist_factor(), g.dist_factor[env_map, ep + 1], rtol=1e-12, atol=0)
            k += 1
    assert not np.any(engine.get("error_bits")), "device/oracle error bits set"
    return worst


def load_rt_trace(name: str) -> SimpleNamespace:
    """real_time (event-skipping) trace, oracle/gen_golden.py `run_config_rt`: per env a variable number of agent steps
    per episode (`n_steps[E, episodes]`), arrays indexed by the env's running agent-step count."""
    g = load_trace(name, prefix="rttrace_")
    g.ep_rows = g.rc.episode_length * (60 // g.rc.minutes)
    g.total_e = g.n_steps.sum(axis=1)  # agent steps recorded per env
    return g


def replay_rt(g, engine, *, float_rtol=1e-9, obs_exact=True):
    """Lock-step replay of a real_time trace on an auto-resetting engine with E == g.E envs: env e is compared while its
    running step count is below g.total_e[e]; afterwards it keeps stepping (next schedule entry) and is ignored."""
    E = g.E
    assert engine.E == E
    engine.set_start_schedule(g.starts)
    obs = engine.reset()
    cmp = (lambda a, b, m: np.testing.assert_array_equal(a, b, err_msg=m)) if obs_exact else \
          (lambda a, b, m: np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=m))
    cmp(obs, g.reset_obs[:, 0], "reset obs, episode 0")
    ep_end = np.cumsum(g.n_steps, axis=1)  # [E, episodes] running index after each episode's last step
    episode = np.zeros(E, dtype=np.int64)
    worst = dict(reward=0.0, soc=0.0, soh=0.0)
    rows_seen = 0
    for k in range(int(g.total_e.max())):
        live = k < g.total_e
        obs, rew, done, term = engine.step(g.actions[:, k])
        t_idx, soc, soh, hl, cash = (engine.get(n) for n in ("time_idx", "soc", "soh", "hours_left", "cashflow"))
        for e in np.nonzero(live)[0]:
            what = f"env {e}, agent step {k}"
            assert bool(done[e]) == bool(g.done[e, k]), f"done flag, {what}"
            np.testing.assert_allclose(rew[e], g.reward[e, k], rtol=float_rtol, atol=1e-12, err_msg=f"reward, {what}")
            np.testing.assert_allclose(cash[e], g.cashflow[e, k], rtol=float_rtol, atol=1e-13, err_msg=f"cashflow, {what}")
            worst["reward"] = max(worst["reward"], rel_err(rew[e], g.reward[e, k]))
            if g.done[e, k]:
                assert k + 1 == ep_end[e, episode[e]], what
                cmp(term[e], g.obs[e, k], f"terminal obs, {what}")
                if g.rc.deg_mode == 2:
                    np.testing.assert_array_equal(engine.get("rf_len")[e], g.rf_len[e, episode[e]], err_msg=what)
                    np.testing.assert_allclose(engine.get("fd_cyc")[e], g.fd_cyc[e, episode[e]], rtol=1e-9, atol=1e-18)
                    np.testing.assert_allclose(engine.get("sei_l")[e], g.sei_l[e, episode[e]], rtol=1e-9, atol=1e-18)
                episode[e] += 1
                if episode[e] < g.episodes:
                    cmp(obs[e], g.reset_obs[e, episode[e]], f"reset obs after {what}")
            else:
                cmp(obs[e], g.obs[e, k], f"obs, {what}")
                assert t_idx[e] == g.time_idx[e, k], f"time row, {what}"
                if "irregular" in g.tables.meta:  # 7- and 8-minute steps: hours_left is not a float32-exact multiple of dt
                    np.testing.assert_allclose(hl[e].astype(np.float64), g.hours_left[e, k], rtol=1e-6, atol=1e-6, err_msg=what)
                else:
                    np.testing.assert_array_equal(hl[e].astype(np.float64), g.hours_left[e, k], err_msg=what)
                np.testing.assert_allclose(soc[e], g.soc[e, k], rtol=float_rtol, atol=1e-15, err_msg=f"soc, {what}")
                np.testing.assert_allclose(soh[e], g.soh[e, k], rtol=float_rtol, atol=0, err_msg=f"soh, {what}")
                np.testing.assert_allclose(engine.get("ep_return")[e], g.ep_return[e, k], rtol=float_rtol, atol=1e-11,
                                           err_msg=f"episode return (sums the skipped rows too), {what}")
                worst["soc"] = max(worst["soc"], rel_err(soc[e], g.soc[e, k]))
                worst["soh"] = max(worst["soh"], rel_err(soh[e], g.soh[e, k]))
        rows_seen += 1
    assert not np.any(engine.get("error_bits")), "device/oracle error bits set"
    assert np.all(g.n_steps < g.ep_rows + 1), "the trace must actually skip rows"
    return worst


# past-done traces (oracle/gen_golden.py `run_config_pd`): no auto-reset; per env reset(), one episode, `seg_steps[e, 1]` steps
# past done, reset(), one more episode.  Their own prefixes: replay() above assumes auto-reset.
PD_TRACE_NAMES = sorted(os.path.basename(p)[len("pdtrace_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN_DIR, "pdtrace_*.npz")))
PD_RT_TRACE_NAMES = sorted(os.path.basename(p)[len("pdrttrace_"):-len(".npz")]
                           for p in glob.glob(os.path.join(GOLDEN_DIR, "pdrttrace_*.npz")))


def load_pd_trace(name: str, rt: bool = False) -> SimpleNamespace:
    g = load_trace(name, prefix="pdrttrace_" if rt else "pdtrace_")
    g.ep_rows = g.rc.episode_length * (60 // g.rc.minutes)
    return g


def replay_pd(g, engine, e, *, float_rtol=1e-9, obs_exact=True, done_getter=None):
    """Replay golden env `e` of a past-done trace on a one-env engine without auto-reset (its start schedule is set here).
    At every step: done (and `done_getter()`, the engine's own episode.done, when given), time row and hours_left bit-exact,
    obs exact or within 1e-5, reward / cashflow / SOC / SoH within `float_rtol`; the rainflow state (rainflow_length exact,
    fd_cyc / fd_cal / l) at the end of each of the three segments.  Returns the largest relative errors seen."""
    assert engine.E == 1
    engine.set_start_schedule(g.starts[:, [e]])
    worst = dict(reward=0.0, soc=0.0, soh=0.0)
    cmp = (lambda a, b, m: np.testing.assert_array_equal(a, b, err_msg=m)) if obs_exact else \
          (lambda a, b, m: np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=m))
    seg_end = np.cumsum(g.seg_steps[e])
    k = 0
    for seg in range(3):
        if seg != 1:
            obs = engine.reset()
            cmp(obs[0], g.reset_obs[e, seg // 2], f"reset obs, episode {seg // 2}")
            np.testing.assert_array_equal(engine.get("start_idx"), g.starts[seg // 2, [e]])
        while k < seg_end[seg]:
            obs, rew, done, _ = engine.step(g.actions[e, k][None])
            what = f"env {e}, segment {seg}, step {k}"
            assert bool(done[0]) == bool(g.done[e, k]), f"done flag, {what}"
            if done_getter is not None:
                assert bool(done_getter()) == bool(g.done[e, k]), f"episode.done / is_done(), {what}"
            cmp(obs[0], g.obs[e, k], f"obs, {what}")
            np.testing.assert_allclose(rew[0], g.reward[e, k], rtol=float_rtol, atol=1e-12, err_msg=f"reward, {what}")
            np.testing.assert_allclose(engine.get("cashflow")[0], g.cashflow[e, k], rtol=float_rtol, atol=1e-13, err_msg=what)
            np.testing.assert_array_equal(engine.get("time_idx")[0], g.time_idx[e, k], err_msg=f"time row, {what}")
            np.testing.assert_array_equal(engine.get("hours_left")[0].astype(np.float64), g.hours_left[e, k], err_msg=what)
            np.testing.assert_allclose(engine.get("soc")[0], g.soc[e, k], rtol=float_rtol, atol=1e-15, err_msg=f"soc, {what}")
            np.testing.assert_allclose(engine.get("soh")[0], g.soh[e, k], rtol=float_rtol, atol=0, err_msg=f"soh, {what}")
            np.testing.assert_allclose(engine.get("soc_deg")[0], g.soc_deg[e, k], rtol=float_rtol, atol=1e-15, err_msg=what)
            np.testing.assert_array_equal(engine.get("target_soc")[0], g.target_soc[e, k], err_msg=what)
            worst["reward"] = max(worst["reward"], rel_err(rew[0], g.reward[e, k]))
            worst["soc"] = max(worst["soc"], rel_err(engine.get("soc")[0], g.soc[e, k]))
            worst["soh"] = max(worst["soh"], rel_err(engine.get("soh")[0], g.soh[e, k]))
            k += 1
        assert g.done[e, k - 1], f"segment {seg} of env {e} must end done"
        if g.rc.deg_mode == 2:
            what = f"rainflow state after segment {seg}, env {e}"
            np.testing.assert_array_equal(engine.get("rf_len")[0], g.rf_len[e, seg], err_msg=what)
            np.testing.assert_allclose(engine.get("fd_cyc")[0], g.fd_cyc[e, seg], rtol=1e-9, atol=1e-18, err_msg=what)
            np.testing.assert_allclose(engine.get("fd_cal")[0], g.fd_cal[e, seg], rtol=1e-9, atol=1e-18, err_msg=what)
            np.testing.assert_allclose(engine.get("sei_l")[0], g.sei_l[e, seg], rtol=1e-9, atol=1e-18, err_msg=what)
    assert not np.any(engine.get("error_bits")), "device/oracle error bits set"
    return worst
