"""The float64 degradation model of tests/degradation_model.py, pinned before the GPU tests trust it:
  * against every step-wise rainflow golden and every linear one (the unmodified reference's own values): per-step SoH and
    each episode's rainflow_length / fd_cyc / fd_cal / l, fed with the golden's reset sample and per-step `soc_deg`;
  * against the CPU oracle stepping saturating tapes (auto-reset and past done), at every degradation row.
No GPU."""
import numpy as np
import pytest

from degradation_model import BOOK, Recount, RecountCheck, SeiModel, deg_rows, rainflow_decisions, rel, starts_avoiding_deg_finish
from golden_util import GOLDEN_DIR, PD_TRACE_NAMES, TRACE_NAMES, load_pd_trace, load_trace, params_for

RAINFLOW = [n for n in TRACE_NAMES if "rainflow" in n]
LINEAR = [n for n in TRACE_NAMES if "linear" in n]
PD = [n for n in PD_TRACE_NAMES if "rainflow" in n or "linear" in n]


def _recount(g, E):
    p = params_for(g, num_envs=E)
    deg = {1: "linear", 2: "rainflow"}[g.rc.deg_mode]
    return Recount(E, g.N, deg, init_soh=p.init_soh, temp=p.temperature, dt=p.dt, evse_power=p.evse_power)


def _assert_book(rc, e, want, what):
    """want: {field: [N]} of the reference.  rainflow_length exact; the floats <= 1e-15 relative, room for a summation order
    other than numpy's pairwise one.  (The model sums each EV's own slice with np.sum, as Series.sum / .mean do: every golden
    is met bit for bit, the test prints the worst.)"""
    np.testing.assert_array_equal(rc.get("rf_len")[e], want["rf_len"], err_msg=f"rainflow_length, {what}")
    for f in BOOK[1:]:
        r = rel(rc.get(f)[e], want[f])
        assert (r <= 1e-15).all(), f"{f}, {what}: {rc.get(f)[e]!r} vs {want[f]!r}"
    return max(float(rel(rc.get(f)[e], want[f]).max()) for f in BOOK[1:])


@pytest.mark.parametrize("name", RAINFLOW + LINEAR)
def test_model_reproduces_the_reference_golden(name):
    g = load_trace(name)
    rc = _recount(g, g.E)
    def_soc = g.rc.def_soc
    worst_soh, worst_book, k = 0.0, 0.0, 0
    for ep in range(g.episodes):
        reset = np.where(g.reset_soc[:, ep] == 0, def_soc, g.reset_soc[:, ep])  # fleet_environment.py:395-399
        rc.reset(np.ones(g.E, bool), reset)
        for s in range(g.ep_steps):
            rc.step(np.ones(g.E, bool), g.soc_deg[:, k], deg_rows(g.tables, g.time_idx[:, k]))
            worst_soh = max(worst_soh, float(np.abs(rc.soh - g.soh[:, k]).max()))
            np.testing.assert_array_equal(rc.soh, g.soh[:, k], err_msg=f"soh, step {k}")
            k += 1
        if rc.deg == "rainflow":
            for e in range(g.E):
                want = {f: getattr(g, f)[e, ep] for f in BOOK}
                worst_book = max(worst_book, _assert_book(rc, e, want, f"env {e}, episode {ep}"))
    assert not rc.get("error_bits").any()
    if 45 % g.rc.minutes == 0:
        assert deg_rows(g.tables, g.time_idx).any()
    else:
        # 30- and 60-minute steps: no row reads 14:45 (fleet_environment.py:665), and this is what the reference recorded --
        # its model was never called: SoH stays at init_soh, rainflow_length at its initial 1, fd_cyc / fd_cal / l at 0
        assert not deg_rows(g.tables, g.time_idx).any()
        assert (g.soh == g.rc.init_soh).all()
        if rc.deg == "rainflow":
            assert (g.rf_len == 1).all() and not g.fd_cyc.any() and not g.fd_cal.any() and not g.sei_l.any()
    print(name, "soh exact; bookkeeping worst rel", worst_book)


@pytest.mark.parametrize("name", PD)
def test_model_reproduces_the_reference_past_done_golden(name):
    """No auto-reset: the log keeps growing past done and its 14:45 rows evaluate it whole; the model's state carries into the
    next episode (quirk Q6).  The reset sample is the CPU oracle's (its reset is pinned to this golden by
    tests/test_oracle_past_done.py)."""
    from oracle.fleet_oracle import OracleBatch

    g = load_pd_trace(name)
    for e in range(g.E):
        rc = _recount(g, 1)
        p = params_for(g, num_envs=1, auto_reset=False)
        cpu = OracleBatch(p, g.tables, g.time_feat)
        cpu.set_start_schedule(g.starts[:, [e]])
        seg_end = np.cumsum(g.seg_steps[e])
        k = 0
        for seg in range(3):
            if seg != 1:
                cpu.reset()
                rc.reset(np.ones(1, bool), cpu.get("soc_deg"))
            while k < seg_end[seg]:
                rc.step(np.ones(1, bool), g.soc_deg[e, k][None], deg_rows(g.tables, g.time_idx[e, k][None]))
                np.testing.assert_array_equal(rc.soh[0], g.soh[e, k], err_msg=f"soh, env {e}, step {k}")
                k += 1
            if rc.deg == "rainflow":
                _assert_book(rc, 0, {f: getattr(g, f)[e, seg] for f in BOOK}, f"env {e}, segment {seg}")
        cpu.close()


def _oracle_run(E, N, auto_reset, steps, seed, deg="rainflow"):
    """OracleBatch at bench.py's workload (caretaker fleet, 48 h episodes) on a saturating tape, its own soc_deg recounted."""
    from bench import bench_config
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params, time_features
    from fleetrl_amd.synth import synth_tables
    from oracle.fleet_oracle import OracleBatch

    tb = synth_tables("ct", N)
    p = make_params(resolve_config(bench_config(E, N, "ct", deg=deg)), tb, E, auto_reset=auto_reset, seed=seed)
    rng = np.random.default_rng(seed)
    cpu = OracleBatch(p, tb, time_features(tb), threads=4)
    n_ep = steps // p.episode_steps + 2
    if auto_reset:
        starts = starts_avoiding_deg_finish(rng, tb, p.start_lo, p.start_hi, p.episode_steps, (n_ep, E))
    else:  # any start, finishing rows at 14:45 included
        starts = rng.integers(p.start_lo, p.start_hi + 1, size=(3 * n_ep, E)).astype(np.int32)
        starts[0, :4] = (starts[0, :4] // 96) * 96 + 58  # finishes on 14:45 (2-day episodes end on their start's clock)
    cpu.set_start_schedule(starts)
    chk = RecountCheck(Recount(E, N, deg, init_soh=p.init_soh, temp=p.temperature, dt=p.dt, evse_power=p.evse_power), tb,
                       rtol=1e-11, soh_atol=1e-15)
    cpu.reset()
    chk.reset(cpu.get)
    ep_prev = cpu.get("episodes")
    past = 0
    for k in range(steps):
        a = rng.uniform(-1, 1, size=(E, N))
        a[rng.random(a.shape) < 0.15] = 0.0
        a[:, : N // 2] = np.sign(a[:, : N // 2])  # half of the EVs driven into their limits: saturated, equal samples
        _, _, done, _ = cpu.step(a.astype(np.float32))
        eps = cpu.get("episodes")
        if auto_reset:
            chk.step(cpu.get, f"step {k}", finished=eps != ep_prev)
        else:
            chk.step(cpu.get, f"step {k}")
            past += int(done.sum())
            # envs whose episode has ended: a third restart at once, the others run on past done for a while
            m = done.astype(bool) & ((np.arange(E) % 3 == 0) | (rng.random(E) < 0.01))
            if m.any():
                cpu.reset(m.astype(np.uint8))
                chk.reset(cpu.get, m)
        ep_prev = eps
    assert cpu.get("episodes").min() >= (steps // p.episode_steps if auto_reset else 5)
    if not auto_reset:
        assert past > 50 * E
    print(chk.report(f"oracle {E}x{N} auto_reset={auto_reset}"))
    cpu.close()
    return chk


@pytest.mark.parametrize("auto_reset", [True, False])
def test_model_recounts_the_oracle_at_every_degradation_row(auto_reset):
    """64 envs x 50 EVs, >= 10 two-day episodes.  The oracle runs the same algorithm on the same samples in C, with libm `pow`
    where the reference's (and the model's) numpy array power is vectorised: a cycle stress may differ in its last bit, and a
    last-bit fd then flips the rounding of exp(-fd) ~ 1, which l ~ 1e-3 inherits 1e3-fold.  So: rainflow_length exact,
    fd_cyc / fd_cal / l <= 1e-11 relative, SoH <= 1e-15 absolute."""
    chk = _oracle_run(64, 50, auto_reset, 10 * 192 + 40, seed=11 if auto_reset else 12)
    assert chk.deg_rows >= 64 * 18


def test_model_recounts_linear_degradation_of_the_oracle():
    _oracle_run(64, 50, True, 2 * 192 + 10, seed=13, deg="linear")


def test_rainflow_decisions_name_the_tie():
    """The decision trace of the attribution helper: an equal-sample skip and a three-point test decided by X == Y."""
    d = rainflow_decisions([0.2, 0.5, 0.5, 0.3, 0.6])
    assert ("skip", 2, True, True) in d
    d1 = rainflow_decisions([0.25, 0.75, 0.25, 0.75])  # X = |0.25 - 0.75| == Y: the tie closes a half cycle
    assert any(x[0] == "close" and x[2] and x[3] for x in d1)
    d2 = rainflow_decisions([0.25, 0.75, 0.25000000000000006, 0.75])  # X < Y by one ulp: nothing closes
    k = next(k for k, (a, b) in enumerate(zip(d1, d2)) if a[:3] != b[:3])
    assert d1[k][0] == "close" and d1[k][3] and not d2[k][3]
    m = SeiModel(1, 1.0, 25.0)
    s = np.array([[0.5, 0.9, 0.2, 0.8, 0.1, 0.95, 0.3]])
    m.evaluate([0], s, [7], 0.25)
    assert m.rf_len[0] > 1 and m.fd_cyc[0] > 0 and 0 < m.l[0] < 1e-3
