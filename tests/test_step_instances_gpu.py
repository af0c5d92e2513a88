"""Every instance of the step kernel the launch planner can select, in every way it can be used, against the CPU oracle: the case list
of tests/step_instances.py (complete by tests/test_step_instances_cpu.py) on seeded synthetic tables -- 24 h episodes with the random
start picker, at least two auto-resets per env, every episode with its 14:45 degradation row, batches of whole workgroups plus a partly
filled last one.  Needs an MI355X.

Bounds (tests/test_hip_shapes.py, tests/golden_util.py): flags, indices and counters bit-exact; float32 observations and terminal rows
rtol 1e-5 / atol 1e-6; rewards rtol 1e-9 (atol 1e-9 per step, 1e-7 on 61-step sums, 1e-8 on policy-rollout sums); soc, soh, cashflow,
ep_return, sei_l rtol 1e-9; fd_cyc rtol 1e-8 (the bound fleet_selftest_stress asserts for the stress approximation).  Data-log columns:
the bounds tests/test_real_time_gpu.py holds the log to against the reference's DataLogger."""
import numpy as np
import pytest

import step_instances as si
from fleetrl_amd import _capi
from fleetrl_amd.config import resolve_config
from fleetrl_amd.params import make_params, time_features
from fleetrl_amd.synth import synth_tables

pytestmark = pytest.mark.gpu

_TABLES = {}
NIGHT_BY_HAND = (1, 30, 3)  # a window that opens every night (the derived one may sit at 24:00 and never open)


def _tables(uc, n):
    if (uc, n) not in _TABLES:
        tb = synth_tables(uc, n, seed=100 + n)
        _TABLES[(uc, n)] = (tb, time_features(tb))
    return _TABLES[(uc, n)]


def _close(got, want, rtol, atol, what):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


class ExpectedLog:
    """What the device-side data log must hold, rebuilt from what the oracle saw step by step (include/fleet_hip.h fleet_log_read;
    fleet_environment.py:420-432, 659-690): one row per table row an env passes -- with real_time several per step, of which the
    oracle shows the last one: the rows before it are checked for their table row and action only --, none for the step that ends an
    episode, and the reset row (bit 31) of the episode after it."""

    def __init__(self, cpu, cap, obs_dim, ep_steps):
        E, N = cpu.E, cpu.N
        self.cpu, self.cap, self.ep_steps = cpu, cap, ep_steps
        self.pos = np.zeros(E, dtype=np.int64)
        self.row = np.zeros((cap, E), dtype=np.uint32)
        self.full = np.zeros((cap, E), dtype=bool)     # every column is known (not a row the skipping loop passed on its way)
        self.deg_ok = np.zeros((cap, E), dtype=bool)   # ... the degradation column too
        self.env = np.zeros((cap, E, 4))
        self.act, self.energy, self.deg, self.soh = (np.zeros((cap, E, N)) for _ in range(4))
        self.obs = np.zeros((cap, E, obs_dim), dtype=np.float32)

    def reset_rows(self, envs, obs):
        k = self.pos[envs]
        assert (k < self.cap).all()
        self.row[k, envs] = self.cpu.get("start_idx")[envs].astype(np.uint32) | np.uint32(0x80000000)
        self.soh[k, envs] = self.cpu.get("soh")[envs]
        self.obs[k, envs] = obs[envs]
        self.full[k, envs] = self.deg_ok[k, envs] = True
        self.pos[envs] += 1

    def step(self, actions, t0, start0, soh0, obs, reward, done):
        cpu = self.cpu
        done = done.astype(bool)
        a = np.asarray(actions, dtype=np.float64)
        t1, soh1 = cpu.get("time_idx"), cpu.get("soh")
        last = np.where(done, start0 + self.ep_steps, t1)  # the table row of the step's last pass
        for e in np.nonzero(last - t0 > 1)[0]:  # real_time: the rows passed on the way
            for row in range(t0[e] + 1, last[e]):
                assert self.pos[e] < self.cap
                self.row[self.pos[e], e] = row
                self.act[self.pos[e], e] = a[e]
                self.pos[e] += 1
        nd = np.nonzero(~done)[0]
        k = self.pos[nd]
        assert (k < self.cap).all()
        self.row[k, nd] = t1[nd]
        self.env[k, nd] = np.stack([reward, cpu.get("cashflow"), cpu.get("overload"), cpu.get("soc_missing")], axis=1)[nd]
        self.act[k, nd] = a[nd]
        self.energy[k, nd] = cpu.get("charge_energy")[nd]
        self.deg[k, nd] = (soh0 - soh1)[nd]
        self.soh[k, nd] = soh1[nd]
        self.obs[k, nd] = obs[nd]
        self.full[k, nd] = True
        self.deg_ok[k, nd] = (t1 - t0 == 1)[nd]  # (a degradation row passed on the way is in the SoH, not in this row's column)
        self.pos[nd] += 1
        if done.any():
            self.reset_rows(np.nonzero(done)[0], obs)

    def check(self, hip):
        assert hip.log_dropped() == 0
        assert hip.log_capacity() == self.cap
        lg = hip.log_read()
        np.testing.assert_array_equal(lg["pos"], self.pos, err_msg="log rows per env")
        valid = np.arange(self.cap)[:, None] < self.pos[None, :]
        np.testing.assert_array_equal(lg["row"].view(np.uint32)[valid], self.row[valid], err_msg="table rows of the log (bit 31: reset rows)")
        assert (self.row[valid] >> 31).any() and self.full[valid].any()
        full = self.full & valid
        _close(lg["env"][full][:, 0], self.env[full][:, 0], 1e-9, 1e-9, "log: reward")
        _close(lg["env"][full][:, 1], self.env[full][:, 1], 1e-9, 1e-12, "log: cashflow")
        _close(lg["env"][full][:, 2], self.env[full][:, 2], 1e-9, 1e-12, "log: grid overloading")
        _close(lg["env"][full][:, 3], self.env[full][:, 3], 1e-9, 1e-12, "log: cumulative missing SOC")
        _close(lg["ev"][:, :, 0, :][valid], self.act[valid], 1e-9, 1e-12, "log: action")
        _close(lg["ev"][:, :, 1, :][full], self.energy[full], 1e-9, 1e-12, "log: energy per EV")
        ok = self.deg_ok & valid
        _close(lg["ev"][:, :, 2, :][ok], self.deg[ok], 1e-6, 1e-12, "log: degradation")
        _close(lg["ev"][:, :, 3, :][full], self.soh[full], 1e-9, 0, "log: SoH")
        _close(lg["obs"][full], self.obs[full], 1e-5, 1e-6, "log: observation")


class Pair:
    """The HIP batch and the oracle of one case, built from the same FleetParams, and the comparisons of one use each."""

    def __init__(self, case, log_rows=0, cfg=None, tables=None):
        """`cfg` / `tables` (a (FleetTables, time features) pair): another config dict and other tables than the case's own
        (tests/test_param_space_gpu.py); the episode is then `episode_length` hours at the config's own step."""
        import torch

        from fleetrl_amd.batch import FleetBatch
        from oracle.fleet_oracle import OracleBatch

        self.case, self.torch, self.dev = case, torch, torch.device("cuda", 0)
        self.tb, tf = _tables(case.uc, case.n_evs) if tables is None else tables
        self.rc = resolve_config(si.config_of(case) if cfg is None else cfg)
        p = make_params(self.rc, self.tb, case.num_envs, seed=case.seed + 1)
        if case.log_data:
            p.log_capacity = log_rows
        ep_steps = 96 if cfg is None else self.rc.episode_length * 60 // self.rc.minutes
        assert (p.auto_reset, p.log_data, p.real_time, p.episode_steps) == (1, int(case.log_data), int(case.real_time), ep_steps)
        self.p, self.E, self.N = p, case.num_envs, case.n_evs
        self.hip, self.cpu = FleetBatch(p, self.tb, tf), OracleBatch(p, self.tb, tf, threads=4)
        self.rng = np.random.default_rng(1000 + case.seed)
        self.s = 0  # steps taken so far: the phase of the action mix
        self.log = ExpectedLog(self.cpu, log_rows, self.hip.obs_dim, ep_steps) if case.log_data else None
        # the handle's own configuration must lead every launch of the case to the instance the case was written for
        for ln in case.launches():
            got = _capi.step_instance(self.hip.E, self.hip.N, p.deg_mode, p.real_time, p.log_data, ln.act_mode, ln.K, ln.has_done_count)[0]
            assert got == case.instance, f"{ln} takes {got}"
        obs = self.cpu.reset()
        np.testing.assert_array_equal(self.hip.reset(), obs)
        np.testing.assert_array_equal(self.hip.get("start_idx"), self.cpu.get("start_idx"))
        if self.log:
            self.log.reset_rows(np.arange(self.E), obs)
        self.obs_d = torch.empty((self.E, self.hip.obs_dim), device=self.dev)
        self.rsum_d = torch.empty(self.E, device=self.dev, dtype=torch.float64)
        self.count_d = torch.empty(self.E, device=self.dev, dtype=torch.int32)

    # ---- inputs ---------------------------------------------------------------------------------------------
    def actions(self, f64, quiet=False):
        """The mix of tests/test_hip_shapes.py `_compare`: uniform in [-1, 1], a charging-biased phase and all ones, 15 % exact zeros;
        float64 actions keep all their digits (not float32-representable)."""
        shape, rng, s = (self.E, self.N), self.rng, self.s
        mode = (s // 40) % 3
        a = rng.uniform(-1, 1, size=shape) if mode == 0 else rng.uniform(-0.2, 1, size=shape) if mode == 1 else np.full(shape, 1.0)
        a[rng.random(shape) < 0.15] = 0.0
        if quiet:  # half of the envs idle in two steps out of three, so that rows are really skipped
            a[(np.arange(self.E) % 2 == 0) & (s % 3 != 0)] = 0.0
        self.s += 1
        if f64:
            assert mode == 2 or (a != a.astype(np.float32)).any()
            return a
        return a.astype(np.float32)

    def upload(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.torch.cuda.synchronize()  # the handle launches on a stream of its own
        return t

    # ---- the oracle's side ------------------------------------------------------------------------------------
    def cpu_step(self, a):
        if self.log is None:
            return self.cpu.step(a)
        t0, start0, soh0 = self.cpu.get("time_idx"), self.cpu.get("start_idx"), self.cpu.get("soh")
        out = self.cpu.step(a)
        self.log.step(a, t0, start0, soh0, out[0], out[1], out[2])
        return out

    # ---- comparisons ------------------------------------------------------------------------------------------
    def check_state(self, where):
        hip, cpu = self.hip, self.cpu
        for name in ("done", "time_idx", "hours_left", "episodes", "start_idx"):
            np.testing.assert_array_equal(hip.get(name), cpu.get(name), err_msg=f"{name}, {where}")
        _close(hip.get("soc"), cpu.get("soc"), 1e-9, 1e-12, f"soc, {where}")
        _close(hip.get("soh"), cpu.get("soh"), 1e-9, 0, f"soh, {where}")
        _close(hip.get("cashflow"), cpu.get("cashflow"), 1e-9, 1e-12, f"cashflow, {where}")
        _close(hip.get("ep_return"), cpu.get("ep_return"), 1e-9, 1e-8, f"ep_return, {where}")
        if self.case.deg == "rainflow":
            np.testing.assert_array_equal(hip.get("rf_len"), cpu.get("rf_len"), err_msg=f"rf_len, {where}")
            _close(hip.get("fd_cyc"), cpu.get("fd_cyc"), 1e-8, 1e-18, f"fd_cyc, {where}")
            _close(hip.get("sei_l"), cpu.get("sei_l"), 1e-9, 1e-18, f"sei_l, {where}")

    def single_steps(self, n, f64, quiet=False, what="single step"):
        """n host steps compared one by one; returns the largest number of table rows one step advanced an env by."""
        most = 0
        for s in range(n):
            a = self.actions(f64, quiet)
            t0 = self.cpu.get("time_idx")
            oh, rh, dh, th = self.hip.step(a)
            oc, rc, dc, tc = self.cpu_step(a)
            np.testing.assert_array_equal(dh, dc, err_msg=f"done, {what} {s}")
            _close(oh, oc, 1e-5, 1e-6, f"obs, {what} {s}")
            _close(rh, rc, 1e-9, 1e-9, f"reward, {what} {s}")
            if dc.any():
                _close(th[dc.astype(bool)], tc[dc.astype(bool)], 1e-5, 1e-6, f"terminal obs, {what} {s}")
            if quiet:
                t1 = self.cpu.get("time_idx")
                np.testing.assert_array_equal(self.hip.get("time_idx"), t1, err_msg=f"time_idx, {what} {s}")
                live = ~dc.astype(bool)
                most = max(most, int((t1 - t0)[live].max()) if live.any() else 0)
            if s % 16 == 0 or s == n - 1:
                self.check_state(f"{what} {s}")
        return most

    def tape(self, K, launches, f64):
        """`launches` launches of K steps from an action tape (with a done_count buffer) against the oracle stepped row by row."""
        for l in range(launches):
            acts = np.stack([self.actions(f64) for _ in range(K)])
            tape = self.upload(acts)
            self.hip.step_many_dev(K, tape.data_ptr(), self.obs_d.data_ptr(), self.rsum_d.data_ptr(), self.count_d.data_ptr(),
                                   act_dtype=_capi.ACT_F64 if f64 else _capi.ACT_F32)
            self.hip.synchronize()
            want_r, want_d = np.zeros(self.E), np.zeros(self.E, dtype=np.int32)
            for k in range(K):
                oc, r, d, _t = self.cpu_step(acts[k])
                want_r += r
                want_d += d
            what = f"launch {l} of K = {K}"
            np.testing.assert_array_equal(self.count_d.cpu().numpy(), want_d, err_msg=f"done_count, {what}")
            _close(self.rsum_d.cpu().numpy(), want_r, 1e-9, 1e-9 if K == 1 else 1e-7, f"reward sum, {what}")
            _close(self.obs_d.cpu().numpy(), oc, 1e-5, 1e-6, f"last observation, {what}")
            if K > 1 or l % 16 == 0 or l == launches - 1:
                self.check_state(what)

    def policy(self, use, chunks, window=None):
        """Rollouts of a built-in policy in launches of `chunks` steps against the oracle driven by host-side actions; returns how
        many (env, step) pairs got all ones, all zeros, and -- night rule on a caretaker fleet -- the distributed rule of 11-14 h."""
        from oracle.fleet_oracle import NightChargingRule

        tb, ct = self.tb, bool(self.p.is_caretaker)
        if use == "night":
            self.hip.set_night_policy(*window)  # (clears the per-env window state)
            rules = [NightChargingRule(window[0], window[1], window[2], self.rc.minutes, ct) for _ in range(self.E)]
        n_ones = n_zeros = n_dist = 0
        for K in chunks:
            self.hip.rollout_policy_dev(si.POLICIES[use], K, self.obs_d.data_ptr(), self.rsum_d.data_ptr(), self.count_d.data_ptr())
            self.hip.synchronize()
            want_r, want_d = np.zeros(self.E), np.zeros(self.E, dtype=np.int32)
            for _ in range(K):
                if use == "uncontrolled":
                    a = np.ones((self.E, self.N))
                elif use == "distributed":
                    a = np.clip(self.cpu.dist_factor(), 0, 1)
                else:
                    t, df = self.cpu.get("time_idx"), self.cpu.dist_factor()
                    a = np.stack([rules[e].action(int(t[e]), int(tb.hour[t[e]]), int(tb.minute[t[e]]), self.N, df[e]) for e in range(self.E)])
                    lunch = ct & (tb.hour[t] >= 11) & (tb.hour[t] <= 14)
                    n_dist += int(lunch.sum())
                    n_ones += int(((a == 1).all(axis=1) & ~lunch).sum())
                    n_zeros += int(((a == 0).all(axis=1) & ~lunch).sum())
                oc, r, d, _t = self.cpu_step(a.astype(np.float64))
                want_r += r
                want_d += d
            what = f"{use} rollout of {K} steps"
            np.testing.assert_array_equal(self.count_d.cpu().numpy(), want_d, err_msg=f"done_count, {what}")
            _close(self.rsum_d.cpu().numpy(), want_r, 1e-9, 1e-9 if K == 1 else 1e-8, f"reward sum, {what}")
            _close(self.obs_d.cpu().numpy(), oc, 1e-5, 1e-6, f"last observation, {what}")
            self.check_state(what)
        return n_ones, n_zeros, n_dist

    def night(self, chunks_derived, chunks_by_hand):
        from fleetrl_amd.policies import night_schedule

        p = self.p
        derived = night_schedule(self.tb, target_soc=p.target_soc, init_battery_cap=p.init_battery_cap, charging_eff=p.charging_eff,
                                 evse_power=p.evse_power)
        a = self.policy("night", chunks_derived, derived)
        b = self.policy("night", chunks_by_hand, NIGHT_BY_HAND)
        n_ones, n_zeros, n_dist = (x + y for x, y in zip(a, b))
        assert n_ones > 0 and n_zeros > 0
        if p.is_caretaker:
            assert n_dist > 0  # the 11-14 h branch

    def finish(self):
        self.hip.check_errors()
        assert not self.cpu.get("error_bits").any()
        self.check_state("the end")
        np.testing.assert_array_equal(self.hip.get("episodes"), self.cpu.get("episodes"))
        _close(self.hip.get("last_ep_return"), self.cpu.get("last_ep_return"), 1e-9, 1e-8, "last_ep_return")
        assert self.cpu.get("episodes").min() >= 2  # every env went through at least two auto-resets
        if self.log:
            self.log.check(self.hip)

    def close(self):
        self.hip.close()
        self.cpu.close()


RT_STEPS = 210  # every step advances an env by at least one row: more than two 96-row episodes


def _run(case, make_pair=Pair):
    """`make_pair(case, log_rows=...)`: the pair of the case (tests/test_param_space_gpu.py builds it under a parameter set)."""
    if case.log_data and case.real_time:
        pair = make_pair(case, log_rows=4 * RT_STEPS + 32)  # a row with clock minute 15 is an event: at most 4 rows per step, plus resets
    elif case.log_data:
        pair = make_pair(case, log_rows=400)
    else:
        pair = make_pair(case)
    try:
        if case.real_time:
            assert case.uses == ("rt",)
            assert pair.single_steps(RT_STEPS, case.f64, quiet=True, what="real_time step") > 1  # rows were really skipped
        elif case.log_data:  # every non-real_time use through the one instance that writes the log: 310 rows
            assert set(case.uses) == {"f32", "f64", "tape1", "tape", "uncontrolled", "distributed", "night"}
            pair.single_steps(30, False, what="float32 step")
            pair.single_steps(30, True, what="float64 step")
            pair.tape(1, 5, case.f64)
            pair.tape(si.K_TAPE, 2, not case.f64)
            pair.policy("uncontrolled", case.policy_chunks())
            pair.policy("distributed", case.policy_chunks())
            pair.policy("night", case.policy_chunks(), NIGHT_BY_HAND)
        else:
            (use,) = case.uses
            if use in ("f32", "f64"):
                pair.single_steps(200, use == "f64")
            elif use == "tape1":
                pair.tape(1, 200, case.f64)
            elif use == "tape":
                pair.tape(si.K_TAPE, 4, case.f64)
                pair.single_steps(20, False, what="single step after the launches")  # the hand-over to the single-step kernel
            elif use == "night":
                pair.night(case.policy_chunks(), (si.K_TAPE, 40))
            else:
                pair.policy(use, case.policy_chunks())
        pair.finish()
    finally:
        pair.close()


@pytest.mark.parametrize("case", si.cases(), ids=lambda c: c.id)
def test_step_instance_matches_the_oracle(case):
    _run(case)
