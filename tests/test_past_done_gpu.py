"""Stepping an env without auto-reset past the end of its episode (the gymnasium.Env path, `FleetEnv`, `auto_reset = 0`) on the
GPU.  The reference allows it: `episode.done` stays True (fleet_environment.py:627-628, :702), LogDataDeg.soc_log keeps growing,
every 14:45 row past the finish runs the degradation model on the whole log, and the DataLogger writes nothing (:679).
Reads only tests/golden/ and the CPU oracle.  Needs an MI355X.  Bar: done, time row, hours_left and rainflow_length bit-exact,
float32 obs <= 1e-5 rel, float64 state <= 1e-9 rel."""
import numpy as np
import pytest

from fleetrl_amd import _capi
from golden_util import PD_RT_TRACE_NAMES, PD_TRACE_NAMES, load_pd_trace, replay_pd

pytestmark = pytest.mark.gpu

CASES = [(n, False) for n in PD_TRACE_NAMES] + [(n, True) for n in PD_RT_TRACE_NAMES]


class _EnvEngine:
    """FleetEnv behind the one-env engine interface of golden_util.replay_pd, through its public step()/reset()."""

    E = 1

    def __init__(self, env):
        self.env = env

    def set_start_schedule(self, starts):
        self.env.core.batch.set_start_schedule(starts)

    def reset(self):
        obs, info = self.env.reset()
        assert info == {}
        return obs[None]

    def step(self, a):
        obs, rew, done, trunc, info = self.env.step(a[0])
        assert isinstance(done, bool) and trunc is False and info == {}
        return obs[None], np.array([rew]), np.array([done]), None

    def get(self, name):
        return self.env.core.batch.get(name)


@pytest.mark.parametrize("name,rt", CASES)
def test_fleet_env_past_done_matches_reference(name, rt):
    """step() and is_done() both report the reference's sticky done at every step; the past-done 14:45 rows move SoH, fd_cyc,
    rainflow_length and l as the reference's do, and the next episode starts from that state (quirk Q6)."""
    from fleetrl_amd import FleetEnv

    g = load_pd_trace(name, rt)
    for e in range(g.E):
        env = FleetEnv(g.cfg, tables=g.tables, start_rows=g.starts[:, [e]], extrema=g.extrema, start_range=(0, 0))
        worst = replay_pd(g, _EnvEngine(env), e, float_rtol=1e-9, obs_exact=False, done_getter=env.is_done)
        print(name, e, worst)
        if g.rc.raw.get("log_data"):
            _assert_log_equals_reference(g, e, env.get_log())
        env.close()


def _assert_log_equals_reference(g, e, lg):
    """The DataLogger rows of the whole schedule: two episodes (reset row + every step but the last), nothing past done."""
    rows = int(g.log_rows[e])
    lg = lg.reset_index(drop=True)
    assert len(lg) == rows
    np.testing.assert_array_equal(lg["Episode"].values.astype(int), g.log_episode[e, :rows])
    np.testing.assert_array_equal(lg["Time"].values.astype("datetime64[s]").astype(np.int64), g.log_time[e, :rows])
    np.testing.assert_allclose(lg["Reward"].values.astype(float), g.log_reward[e, :rows], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(lg["Cashflow"].values.astype(float), g.log_cashflow[e, :rows], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(lg["Penalties"].values.astype(float), g.log_penalty[e, :rows], rtol=1e-9, atol=1e-8)
    for k in range(rows):
        np.testing.assert_allclose(np.broadcast_to(lg["Degradation"].iloc[k], (g.N,)), g.log_deg[e, k], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(lg["SOH"].iloc[k], g.log_soh[e, k], rtol=1e-9)
        np.testing.assert_allclose(lg["Observation"].iloc[k], g.log_obs[e, k], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------
# batches against the oracle (itself pinned by tests/test_oracle_past_done.py): synthetic tables, every group geometry
# ---------------------------------------------------------------------------------------------------------------------------
def _cfg(deg, episode_length=24):
    from test_hip_shapes import _cfg as shapes_cfg

    return shapes_cfg("lmd", deg, False, episode_length=episode_length)


def _pair(n_evs, num_envs, deg, episode_length=24, seed=0):
    from fleetrl_amd.batch import FleetBatch
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params, time_features
    from fleetrl_amd.synth import synth_tables
    from oracle.fleet_oracle import OracleBatch

    tb = synth_tables("lmd", n_evs, seed=100 + n_evs)
    p = make_params(resolve_config(_cfg(deg, episode_length)), tb, num_envs, auto_reset=False, seed=seed + 1)
    tf = time_features(tb)
    return tb, FleetBatch(p, tb, tf), OracleBatch(p, tb, tf, threads=4)


def _assert_state_equal(hip, cpu, deg, what, agree=None):
    """`agree`: [E, N] the EVs whose cycle bookkeeping agrees with the oracle's (default all).  The others -- attributed to an exact
    tie of the reversal extraction, see test_batch_past_done_matches_oracle_step_by_step -- are held to SOC / SoH 1e-4 and their
    bookkeeping to the recount of the kernels' own samples."""
    np.testing.assert_array_equal(hip.get("time_idx"), cpu.get("time_idx"), err_msg=what)
    np.testing.assert_array_equal(hip.get("hours_left"), cpu.get("hours_left"), err_msg=what)
    np.testing.assert_array_equal(hip.get("done"), cpu.get("done"), err_msg=f"episode.done, {what}")
    ok = np.ones(hip.get("soc").shape, bool) if agree is None else agree
    np.testing.assert_allclose(hip.get("soc")[ok], cpu.get("soc")[ok], rtol=1e-9, atol=1e-12, err_msg=what)
    np.testing.assert_allclose(hip.get("soh")[ok], cpu.get("soh")[ok], rtol=1e-9, atol=0, err_msg=f"soh, {what}")
    # (one cycle counted otherwise moves SoH by that cycle's degradation -- measured 3.2e-5 at N = 65 -- and the capacity with it,
    # so the SOC charged afterwards: 1.2e-5)
    np.testing.assert_allclose(hip.get("soc")[~ok], cpu.get("soc")[~ok], rtol=1e-4, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(hip.get("soh")[~ok], cpu.get("soh")[~ok], rtol=1e-4, atol=0, err_msg=f"soh, {what}")
    if deg == "rainflow":
        np.testing.assert_array_equal(hip.get("rf_len")[ok], cpu.get("rf_len")[ok], err_msg=f"rainflow_length, {what}")
        np.testing.assert_allclose(hip.get("fd_cyc")[ok], cpu.get("fd_cyc")[ok], rtol=1e-8, atol=1e-18, err_msg=f"fd_cyc, {what}")
        np.testing.assert_allclose(hip.get("sei_l")[ok], cpu.get("sei_l")[ok], rtol=1e-9, atol=1e-18, err_msg=f"l, {what}")


@pytest.mark.parametrize("n_evs,deg", [(1, "rainflow"), (5, "rainflow"), (50, "rainflow"), (64, "rainflow"), (65, "rainflow"),
                                       (130, "rainflow"), (200, "rainflow"), (5, "linear"), (65, "linear")])
def test_batch_past_done_matches_oracle_step_by_step(n_evs, deg):
    """Envs on staggered start rows, so that some are past done while others are mid-episode; then half of them reset while the
    others run on past done.  done and the degradation state compared at every step (every 14:45 row among them), and every
    EV's bookkeeping against the recount of the kernels' own samples (tests/degradation_model.py).  An EV whose bookkeeping
    differs from the oracle's must be an exact tie of the reversal extraction on one side (degradation_model.attribute, on a
    re-run of its env alone); it stays compared (obs 1e-5, SoH 1e-4)."""
    from degradation_model import Recount, RecountCheck, attribute_by_rerun, book_mismatch
    from fleetrl_amd.batch import FleetBatch
    from oracle.fleet_oracle import OracleBatch

    E = 5
    tb, hip, cpu = _pair(n_evs, E, deg)
    ep = 96
    rng = np.random.default_rng(n_evs)
    base = int(rng.integers(0, tb.T - 8 * ep))
    starts = (base + np.array([0, 17, 40, 71, 95]) + 100 * np.arange(3)[:, None]).astype(np.int32)  # [episode, env]
    hip.set_start_schedule(starts)
    cpu.set_start_schedule(starts)
    np.testing.assert_array_equal(hip.reset(), cpu.reset())
    p = hip.params
    chk = RecountCheck(Recount(E, n_evs, deg, init_soh=p.init_soh, temp=p.temperature, dt=p.dt, evse_power=p.evse_power), tb)
    chk.reset(hip.get)
    # explicit resets: two envs restart 20 steps in, one 50 steps in (so the finishes are staggered: some envs are past done
    # while others are mid-episode); at 3 episodes' length half of the envs start their next episode, the others go on
    resets = {20: [0, 1, 0, 1, 0], 50: [0, 0, 0, 0, 1], 3 * ep: [1, 0, 1, 0, 1]}
    n_deg_past = np.zeros(E, dtype=np.int64)
    off = np.zeros((E, n_evs), bool)  # EVs whose cycle bookkeeping differs from the oracle's
    tape = []
    steps = 3 * ep + 60
    for s in range(steps):
        if s in resets:
            mask = np.array(resets[s], np.uint8)
            np.testing.assert_array_equal(hip.reset(mask)[mask == 1], cpu.reset(mask)[mask == 1])
            chk.reset(hip.get, mask.astype(bool))
        a = rng.uniform(-1, 1, size=(E, n_evs))
        a[rng.random(a.shape) < 0.2] = 0.0
        a = a.astype(np.float32)
        tape.append(a)
        oh, rh, dh, _ = hip.step(a)
        oc, rc, dc, _ = cpu.step(a)
        what = f"step {s}"
        chk.step(hip.get, what)
        np.testing.assert_array_equal(dh, dc, err_msg=f"done, {what}")
        if deg == "rainflow":
            book = ("rf_len", "fd_cyc", "fd_cal", "sei_l")
            off |= book_mismatch({f: hip.get(f) for f in book}, {f: cpu.get(f) for f in book})
        env_ok = ~off.any(axis=1)
        np.testing.assert_allclose(oh, oc, rtol=1e-5, atol=1e-6, err_msg=f"obs, {what}")
        np.testing.assert_allclose(rh[env_ok], rc[env_ok], rtol=1e-9, atol=1e-9, err_msg=f"reward, {what}")
        np.testing.assert_allclose(rh[~env_ok], rc[~env_ok], rtol=1e-5, atol=1e-6, err_msg=f"reward, {what}")
        _assert_state_equal(hip, cpu, deg, what, ~off)
        t = cpu.get("time_idx")
        n_deg_past += dc.astype(bool) & (tb.hour[t] == 14) & (tb.minute[t] == 45)
        if s == 100:
            assert dc.any() and not dc.all()  # some envs past done, others mid-episode
    hip.check_errors()
    assert not cpu.get("error_bits").any()
    assert np.all(n_deg_past >= 1) and n_deg_past.max() >= 2, n_deg_past  # model evaluations past done
    np.testing.assert_array_equal(hip.get("episodes"), cpu.get("episodes"))
    if deg == "rainflow":  # the count did not stop at the episode's last 14:45 row
        assert np.all(hip.get("rf_until") == np.iinfo(np.int32).max)
    print(chk.report(f"past done {E}x{n_evs} {deg}"))
    for e in np.flatnonzero(off.any(axis=1)):
        from fleetrl_amd.params import time_features

        tf = time_features(tb)
        p1 = _pair(n_evs, 1, deg)[1].params
        recs = attribute_by_rerun(lambda: _sched(FleetBatch(p1, tb, tf), starts[:, [e]]),
                                  lambda: _sched(OracleBatch(p1, tb, tf), starts[:, [e]]), tb,
                                  lambda k: tape[k][[e]], steps, lambda k, d: k + 1 in resets and resets[k + 1][e] == 1, int(e),
                                  np.flatnonzero(off[e]), init_soh=p.init_soh, temp=p.temperature, dt=p.dt,
                                  final_gpu={f: hip.get(f)[e] for f in ("rf_len", "fd_cyc", "sei_l", "soh")}, what=f"past done {n_evs}")
        print(f"env {e}: bookkeeping differs from the oracle's through an exact tie: {recs}")
    hip.close()
    cpu.close()


def _sched(x, starts):
    x.set_start_schedule(starts)
    return x


def test_past_done_tape_is_bit_identical_in_every_launch_mode():
    """The same past-done tape through fleet_step_host, fleet_step_dev and every launch mode of fleet_run_tape_dev: bit-identical
    state.  The K-step entries that need auto-reset still refuse a handle without it."""
    import torch

    from fleetrl_amd.batch import FleetBatch, FleetHipError
    from golden_util import params_for

    g = load_pd_trace("ct5_both_rainflow")
    E = 96
    rng = np.random.default_rng(5)
    starts = rng.integers(0, g.tables.T - 4 * g.ep_rows - 60, size=(2, E)).astype(np.int32)
    p = params_for(g, num_envs=E, auto_reset=False)
    tape_len, steps = 37, 2 * g.ep_rows + 40
    acts = rng.uniform(-1, 1, size=(tape_len, E, g.N)).astype(np.float32)
    dev = torch.device("cuda", 0)
    tape = torch.from_numpy(acts).to(dev)
    fields = ("time_idx", "soc", "soh", "hours_left", "rf_len", "fd_cyc", "fd_cal", "sei_l", "done", "ep_return", "episodes")

    def make():
        b = FleetBatch(p, g.tables, g.time_feat)
        b.set_start_schedule(starts)
        bufs = (torch.zeros((E, b.obs_dim), device=dev), torch.zeros(E, device=dev, dtype=torch.float64),
                torch.zeros(E, device=dev, dtype=torch.uint8))
        b.reset_dev(bufs[0].data_ptr())
        return b, bufs

    chunks = (50, steps - 50)  # two runs back to back; each walks the tape from its first row
    rows = [j % tape_len for n in chunks for j in range(n)]
    ref, rbufs = make()  # one fleet_step_dev launch per step
    host = FleetBatch(p, g.tables, g.time_feat)
    host.set_start_schedule(starts)
    host.reset()
    for r in rows:
        ref.step_dev(tape[r].data_ptr(), *(t.data_ptr() for t in rbufs))
        oh, rh, dh, _ = host.step(acts[r])
    ref.synchronize()
    assert rbufs[2].cpu().numpy().all()  # every env is past done at the end
    np.testing.assert_array_equal(oh, rbufs[0].cpu().numpy())
    np.testing.assert_array_equal(rh, rbufs[1].cpu().numpy())
    np.testing.assert_array_equal(dh, rbufs[2].cpu().numpy())
    for f in fields:
        np.testing.assert_array_equal(host.get(f), ref.get(f), err_msg=f"fleet_step_host: {f}")
    for mode in (_capi.LAUNCH_EAGER, _capi.LAUNCH_GRAPH, _capi.LAUNCH_DIRECT):
        b, bufs = make()
        for n in chunks:
            b.run_tape_dev(n, tape.data_ptr(), tape_len, *(t.data_ptr() for t in bufs), use_graph=mode)
        b.synchronize()
        b.check_errors()
        for k, what in enumerate(("obs", "reward", "done")):
            np.testing.assert_array_equal(bufs[k].cpu().numpy(), rbufs[k].cpu().numpy(), err_msg=f"launch mode {mode}: {what}")
        for f in fields:
            np.testing.assert_array_equal(b.get(f), ref.get(f), err_msg=f"launch mode {mode}: {f}")
        b.close()
    ref.check_errors()
    rs = torch.zeros(E, device=dev, dtype=torch.float64)
    with pytest.raises(FleetHipError, match="fleet_step_many_dev needs auto_reset = 1"):
        ref.step_many_dev(4, tape.data_ptr(), rbufs[0].data_ptr(), rs.data_ptr())
    with pytest.raises(FleetHipError, match="fleet_rollout_policy_dev needs auto_reset = 1"):
        ref.rollout_policy_dev(_capi.POLICY_UNCONTROLLED, 4, rbufs[0].data_ptr(), rs.data_ptr())
    ref.close()
    host.close()


def test_rainflow_stack_overflow_past_done_is_an_error_not_a_wrong_result():
    """The rainflow stack workspace is sized for one episode (episode_steps + 3 rows).  Past the finish the samples keep coming;
    an alternating tape of ever smaller swings (each range below the previous one: nothing closes) grows the stack by one entry
    per step until it no longer fits.  The step that gets there raises FLEET_DEVERR_TABLE_END; every step before equals the
    oracle, which has no such bound."""
    tb, hip, cpu = _pair(1, 1, "rainflow", episode_length=1)
    t = tb.time_left[:, 0]
    # a row where the EV has just arrived and stays plugged in for 40 rows
    start = int(next(r for r in range(1, tb.T - 50) if t[r - 1] == 0 and np.all(t[r:r + 40] > 0) and tb.there[r, 0] == 1))
    for x in (hip, cpu):
        x.set_start_schedule(np.array([[start]], np.int32))
    np.testing.assert_array_equal(hip.reset(), cpu.reset())
    ep_steps = 4
    tape = [0.0] * ep_steps + [(1.0 if k % 2 == 0 else -1.0) * 0.95 * 0.85 ** k for k in range(30)]
    raised_at = None
    for s, v in enumerate(tape):
        a = np.full((1, 1), v, np.float32)
        oc, rc, dc, _ = cpu.step(a)
        try:
            oh, rh, dh, _ = hip.step(a)
        except IndexError as exc:
            assert exc.error_bits & _capi.DEVERR_TABLE_END
            raised_at = s
            break
        np.testing.assert_array_equal(dh, dc, err_msg=f"done, step {s}")
        np.testing.assert_allclose(oh, oc, rtol=1e-5, atol=1e-6, err_msg=f"obs, step {s}")
        _assert_state_equal(hip, cpu, "rainflow", f"step {s}")
    assert raised_at is not None and raised_at > ep_steps + 3, raised_at  # past done, once the stack outgrew the workspace
    assert not cpu.get("error_bits").any()
    hip.close()
    cpu.close()
