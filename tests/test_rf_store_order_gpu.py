"""The memory operations of the rainflow push in the state-only twin (fleetrl_amd/csrc/fleet_rainflow.h rf_finish_win; DESIGN.md
section 4 "split push"; EXPERIMENTS.md "Rainflow push in the twin: no load wait behind a store"): the stores of the stack word, of
the top and of slot 0, the stress constant read from the kernel arguments, the `csum` update.  Whatever order they are issued in and
wherever the constant comes from, no stored byte may change: the same tape is run (a) on the library's queue with the twin, (b) on the queue with the twin
switched off (`fleet_set_direct_state_only(h, 0)`: the live instance, which keeps rf_finish_own_b), (c) as single launches on the HIP
stream, and after every run the rainflow rows (header, `csum`, stack words), the hot records, the SEI records, the error words and
everything else that can be read agree bit for bit; the final state meets the CPU oracle at the parity tolerances.

The series is the zigzag of tests/test_rf_window_gpu.py (`plan_lane`: a shrinking zigzag builds the stack up, one swing back out closes
exactly k cycles; every action is chosen from the oracle's current SOC), laid out for E = 29 x N = 50 (G64, three surplus groups), 15 x
100 (G128) and 8 x 200 (G256), all EVs always plugged in, episodes of 24 h (96 steps) from 15:00 on, runs of 1, 2, 3 and 200 steps back
to back along ONE tape of 206 steps.  All lanes of an env push the end point of their first swing in the same step, and among the
lanes of ONE wavefront that step holds: a pusher that closes nothing, the half cycle at size 3, one full closure, two, three (the
loop), and a second closure that is a half cycle (five points).  The series runs twice along the tape:
  * first episode: rainflow_length is 1, so every closure carries stress (the stress regions, `csum` requested and stored);
  * second episode, after the auto-reset inside a dead launch: rainflow_length is what the first episode's 14:45 row (its step 95)
    left -- the cycle count of a whole day -- and the closed-cycle count starts at 0 again (quirk Q6), so no closure of the first swing
    carries stress (the stress regions jumped over, `csum` untouched).
Both preconditions are asserted on the oracle's own `soc_deg` samples and rainflow_length, by a plain streaming three-point count.
Needs an MI355X."""
import numpy as np
import pytest

from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu

RUNS = (1, 2, 3, 200)
STEPS = sum(RUNS)
EP_HOURS, EP_STEPS = 24, 96
ROUNDS = 2  # closing pushes per lane and episode (steps 25 ... 27 and 50 ... 52 of the episode)
FIELDS = ("ep_return", "last_ep_return", "penalty_record", "error_bits", "rf_cycles", "rf_stack", "rf_len", "fd_cyc", "fd_cal", "sei_l", "soh")
CASES = [(50, 29), (100, 15), (200, 8)]  # N, E
_IDS = [f"N{n}-E{e}" for n, e in CASES]
# what a push can be, by (points on the stack with the pushed one, closures): the six kinds one wavefront must hold in one step
KINDS = {"closes nothing": lambda d, k: k == 0, "half cycle at size 3": lambda d, k: d == 3 and k == 1,
         "one full closure": lambda d, k: d >= 4 and k == 1, "two full closures": lambda d, k: d >= 6 and k == 2,
         "three closures (the loop)": lambda d, k: k == 3, "half second closure": lambda d, k: d == 5 and k == 2}


def _setup(N, E):
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params, time_features
    from test_rainflow_adversarial_gpu import _always_there_tables, _cfg

    tb = _always_there_tables(N)
    p = make_params(resolve_config(_cfg(EP_HOURS)), tb, E, seed=5)
    hour, minute = np.asarray(tb.hour), np.asarray(tb.minute)
    row15 = int(np.flatnonzero((hour == 15) & (minute == 0))[1])
    starts = np.full((1, E), row15, np.int32)
    return p, tb, time_features(tb), starts


class Series:
    """The tape of one shape, what the oracle made of it, and what every push of the oracle's samples did."""

    def __init__(self, N, E):
        from oracle.fleet_oracle import OracleBatch
        from test_rf_window_gpu import PAIRS, PERIOD, plan_lane, push

        self.N, self.E = N, E
        p, tb, tf, starts = _setup(N, E)
        cpu = OracleBatch(p, tb, tf, threads=4)
        cpu.set_start_schedule(starts)
        cpu.reset()
        cap0, P, dt, eta = float(p.init_battery_cap), min(float(p.obc_max_power), float(p.evse_power)), float(p.dt), float(p.charging_eff)
        max_step = 0.9 * P * dt * eta / cap0
        # per lane and step of an EPISODE: target offset from the episode's first sample, steps left of the move
        target = np.zeros((EP_STEPS, E, N)); left = np.zeros((EP_STEPS, E, N), np.int32)
        for e in range(E):
            for c in range(N):
                sign = 1.0 if (e + c) % 2 == 0 else -1.0
                moves, _ = plan_lane((7 * c + 13 * e) % len(PAIRS), ROUNDS, 1.9 * max_step, max_step)
                s = 0
                for w, n, r in moves:
                    hold = (r + 1) * PERIOD + e % 3 if r >= 0 else 0
                    assert s <= hold or r < 0, "a lane's round takes longer than PERIOD"
                    s = max(s, hold)
                    for j in range(n):
                        if s < EP_STEPS:
                            target[s, e, c], left[s, e, c] = sign * w, n - j
                        s += 1
        self.acts = np.zeros((STEPS, E, N), np.float32)
        self.soc_deg = np.zeros((STEPS + 1, E, N))
        self.soc_deg[0] = cpu.get("soc_deg")
        self.rf_len = np.zeros((STEPS, E, N), np.int32)
        self.episodes = np.zeros((STEPS + 1, E), np.int64)
        self.episodes[0] = cpu.get("episodes")
        soc0, s0 = cpu.get("soc").copy(), 0
        for s in range(STEPS):
            if s and (self.episodes[s] != self.episodes[s - 1]).any():  # the step before ended the episode: the series starts again
                assert (self.episodes[s] != self.episodes[s - 1]).all()
                soc0, s0 = cpu.get("soc").copy(), s
            soc, cap = cpu.get("soc"), cpu.get("soh") * cap0
            j = s - s0
            delta = np.where(left[j] > 0, (soc0 + target[j] - soc) / np.maximum(left[j], 1), 0.0) if j < EP_STEPS else np.zeros((E, N))
            a = np.where(delta > 0, delta * cap / (P * dt * eta), delta * cap / (P * dt))
            assert np.abs(a).max() <= 1.0
            self.acts[s] = a
            o, r, d, _ = cpu.step(self.acts[s].astype(np.float64))
            self.soc_deg[s + 1] = cpu.get("soc_deg")
            self.rf_len[s] = cpu.get("rf_len")
            self.episodes[s + 1] = cpu.get("episodes")
        assert not cpu.get("error_bits").any()
        assert self.soc_deg.min() > 0.05 and self.soc_deg.max() < 0.84, (self.soc_deg.min(), self.soc_deg.max())
        self.ref = {f: np.array(cpu.get(f)) for f in ("time_idx", "hours_left", "episodes", "soc", "soc_deg", "soh", "ep_return", "last_ep_return",
                                                       "penalty_record", "rf_len", "fd_cyc", "fd_cal", "sei_l", "error_bits")}
        self.ref.update(obs=np.array(o), reward=np.array(r), done=np.array(d))
        cpu.close()
        self.ends = [int(s) for s in range(1, STEPS + 1) if self.episodes[s, 0] != self.episodes[s - 1, 0]]  # steps that ended an episode
        # the streaming count over the oracle's samples, episode by episode: per (step, env, wavefront of the env) the pushes as
        # (points with the pushed one, closures, closures that carry stress)
        self.pushes = {}
        for e in range(E):
            for c in range(N):
                x = self.soc_deg[:, e, c]
                stack, nc, sgn, prev = [x[0]], 0, 0, x[0]
                for s in range(STEPS):
                    v = x[s + 1]
                    if s in self.ends:  # the sample after the reset starts a new series (the step's own sample went to the old one)
                        stack, nc, sgn, prev = [v], 0, 0, v
                        continue
                    if v != prev:
                        sg = 1 if v > prev else 2
                        if sgn and sg != sgn:  # `prev` was a reversal point
                            d = len(stack) + 1
                            k = push(stack, prev)
                            L = int(self.rf_len[s - 1, e, c]) if s else 1  # rainflow_length when the push runs
                            stressed = sum(1 for idx in range(nc, nc + k) if idx >= L - 1)
                            self.pushes.setdefault((s, e, c // 64), []).append((d, k, stressed))
                            nc += k
                        sgn, prev = sg, v

    def wavefronts_with_all_kinds(self, stress):
        """(step, env, wavefront) whose lanes hold every kind of push at once, every closure of those lanes with stress (`stress`) or
        every one without."""
        found = []
        for key, ps in self.pushes.items():
            ok = [(d, k) for d, k, st in ps if (st == k if stress else st == 0)]
            if all(any(kind(d, k) for d, k in ok) for kind in KINDS.values()):
                found.append(key)
        return found


_SERIES = {}


def _series(N, E):
    if (N, E) not in _SERIES:
        _SERIES[(N, E)] = Series(N, E)
    return _SERIES[(N, E)]


class _Way:
    """One handle, its output buffers and how it launches."""

    def __init__(self, N, E, mode, twin):
        import torch
        from fleetrl_amd.batch import FleetBatch

        p, tb, tf, starts = _setup(N, E)
        self.b = FleetBatch(p, tb, tf)
        self.b.set_start_schedule(starts)
        self.mode = mode
        dev = torch.device("cuda", 0)
        self.out = (torch.zeros((E, self.b.obs_dim), device=dev), torch.zeros(E, device=dev, dtype=torch.float64),
                    torch.zeros(E, device=dev, dtype=torch.uint8))
        if twin is not None:
            self.b.set_direct_state_only(twin)
        self.b.reset_dev(self.out[0].data_ptr())

    def run(self, steps, tape):
        self.b.run_tape_dev(steps, tape.data_ptr(), steps, *(t.data_ptr() for t in self.out), use_graph=self.mode, act_dtype=_capi.ACT_F32)
        self.b.synchronize()

    def everything(self):
        got = {f"out.{k}": t.cpu().numpy() for k, t in zip(("obs", "reward", "done"), self.out)}
        got.update({f"get.{f}": self.b.get(f) for f in FIELDS})
        # every section of the saved state: the rainflow rows, the hot records, the SEI records and the error words among them
        got.update({f"state.{k}": np.array(v).view(np.uint8) for k, v in self.b.state_dict().items()})
        # of a rainflow row the live part is state -- the 6 header words (`csum` is the fifth) and the stack words below the top entry;
        # the words beyond were never written or are popped entries (tests/test_direct_state_only_twin_gpu.py)
        rows = got["state.rf_rows"].view(np.uint64)
        live = 6 + np.maximum(got["get.rf_stack"].astype(np.int64) - 1, 0)
        rows[np.arange(rows.shape[2])[None, None, :] >= live[:, :, None]] = 0
        return got


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")


@pytest.mark.parametrize("N,E", CASES, ids=_IDS)
def test_one_wavefront_holds_every_kind_of_push_with_stress_and_without(N, E):
    """The precondition, on the CPU oracle alone."""
    sr = _series(N, E)
    assert len(sr.ends) == 2 and sr.ends[0] == EP_STEPS, sr.ends  # the second series starts behind the first episode's end
    first_run_end = sum(RUNS[:-1])
    for stress in (True, False):
        found = sr.wavefronts_with_all_kinds(stress)
        print(N, E, "stress" if stress else "no stress", found[:4], len(found))
        assert found, f"no wavefront and step with every kind of push, {'all' if stress else 'none'} of their closures with stress"
        # ... in a dead launch of the run of 200 (the twin), in the first episode (stress) / the second (none)
        steps = {s for s, _, _ in found}
        assert all(first_run_end < s < STEPS - 1 for s in steps)
        assert all((s < sr.ends[0]) == stress for s in steps)
    # the first episode's pushes all carry stress (rainflow_length 1), and its 14:45 row moved rainflow_length on
    assert all(st == k for (s, _, _), ps in sr.pushes.items() if s < sr.ends[0] - 1 for _, k, st in ps)
    assert sr.rf_len[sr.ends[0]].min() > 1


@pytest.mark.parametrize("N,E", CASES, ids=_IDS)
def test_twin_equals_live_instance_equals_stream_and_meets_the_oracle(N, E):
    import torch

    sr = _series(N, E)
    assert _capi.step_has_state_only(E, N, 2, False, False, _capi.ACT_F32)
    tape = torch.from_numpy(sr.acts).to("cuda:0")
    torch.cuda.synchronize()
    ways = {"twin": _Way(N, E, _capi.LAUNCH_DIRECT, True), "flag": _Way(N, E, _capi.LAUNCH_DIRECT, False),
            "stream": _Way(N, E, _capi.LAUNCH_EAGER, None)}
    live = dead = done = 0
    for steps in RUNS:  # back to back along the tape, everything read in between
        for w in ways.values():
            w.run(steps, tape[done:])
        done += steps
        want = ways["stream"].everything()
        _same(ways["twin"].everything(), want, f"twin vs stream after a run of {steps}")
        _same(ways["flag"].everything(), want, f"flag vs stream after a run of {steps}")
        live, dead = live + 1, dead + steps - 1
        assert ways["twin"].b.direct_packet_counts() == (live, dead)      # the twin for every launch but a run's last
        assert ways["flag"].b.direct_packet_counts() == (live + dead, 0)  # switched off: the live instance throughout
    for w in ways.values():
        w.b.check_errors()
    # `csum` was written: the first episode's closures all carried stress, and its 14:45 row consumed the sum (fd_cyc)
    assert (ways["twin"].b.get("fd_cyc") > 0).all()

    # the twin's final state and last outputs against the CPU oracle (tolerances: tests/test_hip_shapes.py, tests/test_rf_window_gpu.py)
    b, ref = ways["twin"].b, sr.ref
    for f in ("time_idx", "hours_left", "episodes", "rf_len"):
        np.testing.assert_array_equal(b.get(f), ref[f], err_msg=f)
    assert not b.get("error_bits").any() and not ref["error_bits"].any()
    for f in ("soc", "soh", "ep_return", "penalty_record"):
        np.testing.assert_allclose(b.get(f), ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    np.testing.assert_allclose(b.get("last_ep_return"), ref["last_ep_return"], rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(b.get("fd_cyc"), ref["fd_cyc"], rtol=1e-8, atol=1e-18)
    np.testing.assert_allclose(b.get("sei_l"), ref["sei_l"], rtol=1e-9, atol=1e-18)
    obs, rew, dn = (t.cpu().numpy() for t in ways["twin"].out)
    np.testing.assert_array_equal(dn, ref["done"])
    np.testing.assert_allclose(obs, ref["obs"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rew, ref["reward"], rtol=1e-9, atol=1e-9)
    for w in ways.values():
        w.b.close()
