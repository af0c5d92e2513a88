"""The kernels' rainflow count and SEI pass against a recount of their OWN logged SOC samples (tests/degradation_model.py):
after every step the host reads soc_deg / time_idx / episodes / done and appends each env's sample to its log; on every
degradation row of every env ALL its EVs are checked -- rainflow_length exact, fd_cyc / fd_cal / l <= 1e-8 relative (the bound
fleet_selftest_stress asserts for the stress approximation), the env-side SoH <= 1e-10 absolute at every step, the error bits
equal.  Every exact-equality decision of the reversal extraction is taken on the same numbers on both sides: no EV is exempt.
The headline run also steps the CPU oracle in lockstep; an EV whose bookkeeping differs from the oracle's must be explained by
an exact tie on one side (degradation_model.attribute), and such EVs must stay rare.  Needs an MI355X."""
import os

import numpy as np
import pytest

from degradation_model import Recount, RecountCheck, attribute_by_rerun, book_mismatch, deg_rows, starts_avoiding_deg_finish
from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu
THREADS = min(16, os.cpu_count() or 1)
DIVERGENCE_PER_EV_STEP = 1 / 2e7  # 4x the one observation before this test (1 EV in 8.2e7 EV-steps)


def _setup(E, N, deg, auto_reset, seed):
    from bench import bench_config
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params, time_features
    from fleetrl_amd.synth import synth_tables

    tb = synth_tables("ct", N)
    p = make_params(resolve_config(bench_config(E, N, "ct", deg=deg)), tb, E, auto_reset=auto_reset, seed=seed)
    return tb, p, time_features(tb)


class _Direct:
    """FleetBatch stepped one launch at a time through the library's own queue (the launch path bench.py times) from a device tape."""

    def __init__(self, b, tape):
        import torch

        self.b, self.tape = b, tape
        dev = torch.device("cuda", 0)
        self.o = (torch.zeros((b.E, b.obs_dim), device=dev), torch.zeros(b.E, device=dev, dtype=torch.float64),
                  torch.zeros(b.E, device=dev, dtype=torch.uint8))

    def reset(self):
        self.b.reset_dev(self.o[0].data_ptr())
        self.b.synchronize()
        return self.o[0].cpu().numpy()

    def step(self, k):
        row = self.tape[k % self.tape.shape[0]]
        self.b.run_tape_dev(1, row.data_ptr(), 1, *(t.data_ptr() for t in self.o), use_graph=_capi.LAUNCH_DIRECT)
        self.b.synchronize()
        return tuple(t.cpu().numpy() for t in self.o)


def test_headline_direct_run_recount_and_oracle_lockstep():
    """4096 envs x 50 EVs, bench.py's workload and tape distribution (uniform(-1, 1), 15 % zeros), auto-reset (the count stops
    at the episode's last degradation row, `rf_until`), > 10 two-day episodes per env.  The start rows come from a schedule in
    which no episode finishes on a 14:45 row: with auto-reset the finishing step's sample is replaced by the next episode's reset
    sample before the host can read it; away from a degradation row it is never needed (the count has stopped, reset() clears
    the log).  The oracle steps in lockstep: obs 1e-5, reward 1e-9, SOC / SoH 1e-9 and the bookkeeping at every degradation row
    for every EV that agrees with it; an EV that does not is attributed to an exact tie and then held to obs 1e-5, SoH 1e-4
    (one cycle counted otherwise moves SoH by its degradation) and, like every EV, to the recount of its own samples."""
    import torch

    from fleetrl_amd.batch import FleetBatch
    from oracle.fleet_oracle import OracleBatch

    E, N, L = 4096, 50, 32
    tb, p, tf = _setup(E, N, "rainflow", True, 0)
    rng = np.random.default_rng(21)
    steps = 10 * p.episode_steps + 24
    starts = starts_avoiding_deg_finish(rng, tb, p.start_lo, p.start_hi, p.episode_steps, (12, E))
    acts = rng.uniform(-1, 1, size=(L, E, N)).astype(np.float32)
    acts[rng.random(acts.shape) < 0.15] = 0.0
    b = FleetBatch(p, tb, tf)
    cpu = OracleBatch(p, tb, tf, threads=THREADS)
    for x in (b, cpu):
        x.set_start_schedule(starts)
    gpu = _Direct(b, torch.from_numpy(acts).to("cuda:0"))
    np.testing.assert_allclose(gpu.reset(), cpu.reset(), rtol=1e-6, atol=1e-7)
    chk = RecountCheck(Recount(E, N, "rainflow", init_soh=p.init_soh, temp=p.temperature, dt=p.dt), tb)
    chk.reset(b.get)
    ep_prev = b.get("episodes")
    off = np.zeros((E, N), bool)  # EVs whose bookkeeping differs from the oracle's
    first_off = {}
    for k in range(steps):
        oh, rh, dh = gpu.step(k)
        oc, rc, dc, _ = cpu.step(acts[k % L])
        what = f"step {k}"
        assert np.array_equal(dh, dc), f"done, {what}"
        eps = b.get("episodes")
        np.testing.assert_array_equal(eps, cpu.get("episodes"), err_msg=what)
        np.testing.assert_array_equal(b.get("time_idx"), cpu.get("time_idx"), err_msg=what)
        np.testing.assert_allclose(oh, oc, rtol=1e-5, atol=1e-6, err_msg=f"obs, {what}")
        np.testing.assert_allclose(rh, rc, rtol=1e-9, atol=1e-12, err_msg=f"reward, {what}")
        ev = chk.step(b.get, what, finished=eps != ep_prev)
        ep_prev = eps
        if ev.size:  # the degradation rows of this step: the kernels' bookkeeping against the oracle's
            hb = {f: b.get(f)[ev] for f in ("rf_len", "fd_cyc", "fd_cal", "sei_l")}
            cb = {f: cpu.get(f)[ev] for f in hb}
            new = book_mismatch(hb, cb) & ~off[ev]
            for kk, c in np.argwhere(new):
                first_off[(int(ev[kk]), int(c))] = k
            off[ev] |= new
        agree = ~off
        for f in ("soc", "soh"):
            h, c = b.get(f), cpu.get(f)
            np.testing.assert_allclose(h[agree], c[agree], rtol=1e-9, atol=1e-12, err_msg=f"{f}, {what}")
            # one cycle counted otherwise moves SoH by that cycle's degradation (measured 3.2e-5): 1e-4 for these EVs
            np.testing.assert_allclose(h[off], c[off], rtol=1e-4, atol=1e-9, err_msg=f"{f} (attributed EVs), {what}")
    assert b.get("episodes").min() >= 10
    b.check_errors()
    assert not cpu.get("error_bits").any()
    print(chk.report("kernels vs the recount of their own samples, 4096x50 direct"))
    n_off = int(off.sum())
    print(f"bookkeeping differs from the oracle for {n_off} EVs in {chk.ev_steps} EV-steps "
          f"(1 per {chk.ev_steps / max(n_off, 1):.3g}); bound 1 per {1 / DIVERGENCE_PER_EV_STEP:.3g}")
    assert n_off <= chk.ev_steps * DIVERGENCE_PER_EV_STEP, f"{n_off} EVs differ from the oracle: {sorted(first_off.items())[:8]}"
    # every such EV: an exact tie of the reversal extraction on one side, nothing else
    for e in sorted({e for e, _ in first_off}):
        evs = [c for (ee, c) in first_off if ee == e]
        pe = _setup(1, N, "rainflow", False, 0)[1]  # one env, no auto-reset: reset right after the finishing step instead
        recs = attribute_by_rerun(
            lambda: _one(FleetBatch(pe, tb, tf), starts[:, [e]]), lambda: _one(OracleBatch(pe, tb, tf), starts[:, [e]]), tb,
            lambda k: acts[k % L, [e]], steps, lambda k, d: d, e, evs, init_soh=p.init_soh, temp=p.temperature, dt=p.dt,
            final_gpu={f: b.get(f)[e] for f in ("rf_len", "fd_cyc", "sei_l", "soh")}, what="headline")
        print(f"env {e}: {recs}")
    b.close(); cpu.close()


def _one(x, starts):
    x.set_start_schedule(starts)
    return x


def _fleet_env_path(E, N, deg, steps, seed):
    """auto_reset = 0 (the gymnasium.Env path): after every step the envs whose episode has ended are reset -- a third of them at
    once, the others after a random while past done (their log keeps growing and their 14:45 rows evaluate it whole, as in the
    reference).  Any start row, finishes on a 14:45 row included."""
    from fleetrl_amd.batch import FleetBatch

    tb, p, tf = _setup(E, N, deg, False, seed)
    rng = np.random.default_rng(seed)
    starts = rng.integers(p.start_lo, p.start_hi + 1, size=(40, E)).astype(np.int32)
    starts[0, : E // 8] = (starts[0, : E // 8] // 96) * 96 + 58  # these finish on 14:45 (48 h episodes end on their start's clock)
    b = FleetBatch(p, tb, tf)
    b.set_start_schedule(starts)
    b.reset()
    chk = RecountCheck(Recount(E, N, deg, init_soh=p.init_soh, temp=p.temperature, dt=p.dt, evse_power=p.evse_power), tb)
    chk.reset(b.get)
    past, fin_deg = 0, 0
    for k in range(steps):
        a = rng.uniform(-1, 1, size=(E, N))
        a[rng.random(a.shape) < 0.15] = 0.0
        _, _, done, _ = b.step(a.astype(np.float32))
        done = done.astype(bool)
        fin_deg += int((done & deg_rows(tb, b.get("time_idx"))).sum())
        chk.step(b.get, f"step {k}")
        past += int(done.sum())
        m = done & ((np.arange(E) % 3 == 0) | (rng.random(E) < 0.1))
        if m.any():
            b.reset(m.astype(np.uint8))
            chk.reset(b.get, m)
    assert b.get("episodes").min() >= 10
    assert past > E and fin_deg > 0
    b.check_errors()
    print(chk.report(f"kernels vs the recount of their own samples, FleetEnv path {E}x{N} {deg}"))
    b.close()


@pytest.mark.parametrize("N", [5, 64, 65, 200])
def test_fleet_env_path_recount(N):
    _fleet_env_path(256, N, "rainflow", 11 * 192 + 60, seed=N)


def test_linear_degradation_recount_at_the_headline_shape():
    from fleetrl_amd.batch import FleetBatch
    import torch

    E, N, L = 4096, 50, 32
    tb, p, tf = _setup(E, N, "linear", True, 1)
    rng = np.random.default_rng(3)
    starts = starts_avoiding_deg_finish(rng, tb, p.start_lo, p.start_hi, p.episode_steps, (4, E))
    acts = rng.uniform(-1, 1, size=(L, E, N)).astype(np.float32)
    acts[rng.random(acts.shape) < 0.15] = 0.0
    b = FleetBatch(p, tb, tf)
    b.set_start_schedule(starts)
    gpu = _Direct(b, torch.from_numpy(acts).to("cuda:0"))
    gpu.reset()
    chk = RecountCheck(Recount(E, N, "linear", init_soh=p.init_soh, temp=p.temperature, dt=p.dt, evse_power=p.evse_power), tb)
    chk.reset(b.get)
    ep_prev = b.get("episodes")
    for k in range(2 * p.episode_steps + 24):
        gpu.step(k)
        eps = b.get("episodes")
        chk.step(b.get, f"step {k}", finished=eps != ep_prev)
        ep_prev = eps
    assert b.get("episodes").min() >= 2
    b.check_errors()
    print(chk.report("kernels vs the recount, linear 4096x50 direct"))
    b.close()
