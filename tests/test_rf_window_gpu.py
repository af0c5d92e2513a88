"""The rainflow push (fleetrl_amd/csrc/fleet_rainflow.h rf_request / rf_finish / rf_finish_own_b / rf_finish_win): the closures a
push performs from the request's window -- registers: the first one everywhere, the second one too in the state-only twin -- and the
ones it performs from the stack words, at every stack depth and closure count at which the two meet.

The series.  32 envs x 50 EVs (groups of 64 lanes, eight workgroups: the smallest grid the library's own queue takes), all EVs
always plugged in (`_always_there_tables`), one 72 h episode from 15:00 on, 200 steps: past the second day's 14:45 row.  Every EV
walks a list of SOC waypoints, each of which becomes a reversal point; every action is chosen from the ORACLE's current SOC (closed
loop on the CPU), so the SOC series is the planned one.  A zigzag of strictly shrinking ranges (each 0.85 of the one before: nothing
closes) builds the stack up to `d - 1` points; one swing back out then ends between two chosen older points, and the push of its end
point -- the stack holds `d` points with it -- closes exactly `k` cycles.  The next round's zigzag continues inside the last range.
(d, k) runs over d = 3 ... 13 (3: the half cycle at size 3; shallow stacks, whose window words are header words; depths whose words
lie beyond the row's first 128-byte line), k = 0 ... 5, as far as a stack of d points can close k cycles (k <= (d - 1) // 2: 46
pairs).  The 50 lanes of an env are given different pairs in the same round and all push their end point in the same step, so one
wavefront holds lanes that close 0, 1, 2, 3, 4 and 5 cycles at once.  What the oracle's series really produced is counted by a plain
streaming three-point rainflow over the oracle's own `soc_deg` samples, and the histogram is asserted.

The paths: (1) step by step through fleet_step_dev (the live instance), (2) the tape as one run on the library's own queue (the
state-only twin, with the deep window, for all launches but the last), (3) fleet_step_many_dev (K-step: the carried header).  `rf_cycles` and
`rf_stack` equal the streaming count exactly (after every step of (1)); `rf_len` exactly, `fd_cyc` / `fd_cal` / `sei_l` to 1e-9 and
`soh` to 1e-10 against the oracle (after every step of (1), the two daily rows among them -- the first one evaluates closures that
all carried stress, rainflow_length being 1 until then: the `csum` update of the push); (1) and (2) bit for bit in every state field.
Needs an MI355X."""
import math

import numpy as np
import pytest

from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu

E, N, STEPS, EP_HOURS = 32, 50, 200, 72
Q = 0.85             # each zigzag range is this share of the one before
PERIOD = 25          # steps between two closing pushes of a lane
PAIRS = [(d, k) for d in range(3, 14) for k in range(6) if k <= (d - 1) // 2]
BOOK = ("rf_len", "fd_cyc", "fd_cal", "sei_l", "soh")


def push(stack, p):
    """rainflow.extract_cycles' three-point rule for one new reversal point: returns the closed cycles."""
    stack.append(p)
    k = 0
    while len(stack) >= 3 and not abs(stack[-1] - stack[-2]) < abs(stack[-2] - stack[-3]):
        k += 1
        if len(stack) == 3:
            stack.pop(0)
        else:
            last = stack.pop(); stack.pop(); stack.pop(); stack.append(last)
    return k


def plan_lane(first, rounds, r0, max_step):
    """Waypoints of one EV as offsets from its first sample, in units of SOC: [(offset, steps of the move, round whose closing push
    the departure from the PREVIOUS waypoint is -- or -1)], and the (d, k) planned per round.  `first`: index into PAIRS to start at."""
    S = [0.0, r0]
    moves = [(r0, -1)]
    planned = []
    nxt = first
    for r in range(rounds):
        for j in range(len(PAIRS)):  # the next pair this stack can still be built up to
            d, k = PAIRS[(nxt + j) % len(PAIRS)]
            if d - 1 >= len(S):
                nxt = (nxt + j + 1) % len(PAIRS)
                break
        else:  # too deep for every pair: collapse it
            d = len(S) + 1
            k = (d - 1) // 2
        while len(S) < d - 1:  # shrinking zigzag: nothing closes
            w = S[-1] + Q * (S[-2] - S[-1])
            assert push(S, w) == 0
            moves.append((w, -1))
        n = d - 1
        if k == 0:
            p = S[-1] + 0.5 * (S[-2] - S[-1])
        else:
            lo = S[n - 2 * k]  # the swing passes this point ...
            p = 0.5 * (lo + S[n - 2 - 2 * k]) if n - 2 - 2 * k >= 0 else lo + 0.25 * (lo - S[n - 2 * k + 1])  # ... and not the one behind it
        assert push(S, p) == k, (d, k)
        moves.append((p, -1))
        planned.append((d, k))
        # the departure from p, in the same step for every lane of the env, pushes it
        w = S[-1] + Q * (S[-2] - S[-1])
        assert push(S, w) == 0
        moves.append((w, r))
    out, at = [], 0.0
    for w, r in moves:
        out.append((w, max(1, math.ceil(abs(w - at) / max_step - 1e-9)), r))
        at = w
    return out, planned


class Series:
    """The tape, and what the oracle and the streaming count make of it."""

    def __init__(self):
        from fleetrl_amd.config import resolve_config
        from fleetrl_amd.params import make_params, time_features
        from oracle.fleet_oracle import OracleBatch
        from test_rainflow_adversarial_gpu import _always_there_tables, _cfg

        self.tb = tb = _always_there_tables(N)
        self.p = p = make_params(resolve_config(_cfg(EP_HOURS)), tb, E, seed=5)
        self.tf = time_features(tb)
        hour, minute = np.asarray(tb.hour), np.asarray(tb.minute)
        row15 = int(np.flatnonzero((hour == 15) & (minute == 0))[1])
        self.starts = (row15 + np.arange(E) % 4).astype(np.int32)[None, :]  # the envs meet their daily rows in different steps
        cpu = OracleBatch(p, tb, self.tf)
        cpu.set_start_schedule(self.starts)
        cpu.reset()
        cap0, P, dt, eta = float(p.init_battery_cap), min(float(p.obc_max_power), float(p.evse_power)), float(p.dt), float(p.charging_eff)
        max_step = 0.9 * P * dt * eta / cap0  # SOC gained by one step at 90 % power (a discharging step moves further)
        rounds = STEPS // PERIOD
        # per lane: target offset, steps left of the move and the step before which the move may not start, per step of the run
        soc0 = cpu.get("soc").copy()
        target = np.zeros((STEPS, E, N)); left = np.zeros((STEPS, E, N), np.int32)
        self.planned = []
        for e in range(E):
            for c in range(N):
                sign = 1.0 if (e + c) % 2 == 0 else -1.0
                moves, planned = plan_lane((7 * c + 13 * e) % len(PAIRS), rounds, 1.9 * max_step, max_step)
                self.planned += planned
                s = 0
                for w, n, r in moves:
                    hold = (r + 1) * PERIOD + e % 3 if r >= 0 else 0
                    assert s <= hold or r < 0, "a lane's round takes longer than PERIOD"
                    s = max(s, hold)  # (until then: action 0, equal samples, which the reversal extraction skips)
                    for j in range(n):
                        if s < STEPS:
                            target[s, e, c], left[s, e, c] = sign * w, n - j
                        s += 1
        acts = np.zeros((STEPS, E, N), np.float32)
        self.soc_deg = np.zeros((STEPS + 1, E, N))
        self.soc_deg[0] = cpu.get("soc_deg")
        self.book = {f: np.zeros((STEPS, E, N), cpu.get(f).dtype) for f in BOOK}
        self.time_idx = np.zeros((STEPS, E), np.int32)
        for s in range(STEPS):
            soc, cap = cpu.get("soc"), cpu.get("soh") * cap0
            delta = np.where(left[s] > 0, (soc0 + target[s] - soc) / np.maximum(left[s], 1), 0.0)
            a = np.where(delta > 0, delta * cap / (P * dt * eta), delta * cap / (P * dt))
            assert np.abs(a).max() <= 1.0
            acts[s] = a
            cpu.step(acts[s].astype(np.float64))
            self.soc_deg[s + 1] = cpu.get("soc_deg")
            for f in BOOK:
                self.book[f][s] = cpu.get(f)
            self.time_idx[s] = cpu.get("time_idx")
        assert (self.time_idx[-1] == self.starts[0] + STEPS).all()  # one episode: no reset inside the run
        assert not cpu.get("error_bits").any()
        assert self.soc_deg.min() > 0.05 and self.soc_deg.max() < 0.84, (self.soc_deg.min(), self.soc_deg.max())
        cpu.close()
        self.acts = acts
        # the streaming count over the oracle's samples: cycles and stack size after every step, and what every push did
        self.cycles = np.zeros((STEPS, E, N), np.int32); self.stack = np.zeros((STEPS, E, N), np.int32)
        self.hist = {}
        self.closed_by_wave = [[set() for _ in range(E)] for _ in range(STEPS)]
        self.stressed_multi = [0, 0]  # pushes closing >= 2 cycles of which one carries stress: before / after the first daily row
        for e in range(E):
            for c in range(N):
                x = self.soc_deg[:, e, c]
                stack, nc, sgn, prev = [x[0]], 0, 0, x[0]
                for s in range(STEPS):
                    v = x[s + 1]
                    if v != prev:
                        sg = 1 if v > prev else 2
                        if sgn and sg != sgn:  # `prev` was a reversal point
                            size = len(stack) + 1
                            k = push(stack, prev)
                            self.hist[(size, k)] = self.hist.get((size, k), 0) + 1
                            self.closed_by_wave[s][e].add(k)
                            rf_len = int(self.book["rf_len"][max(s - 1, 0), e, c])  # rainflow_length when the push runs (step 0 is no daily row)
                            if k >= 2 and nc + k - 1 >= rf_len - 1:
                                self.stressed_multi[1 if rf_len > 1 else 0] += 1
                            nc += k
                        sgn, prev = sg, v
                    self.cycles[s, e, c], self.stack[s, e, c] = nc, len(stack)


@pytest.fixture(scope="module")
def series():
    return Series()


def _handle(sr):
    import torch
    from fleetrl_amd.batch import FleetBatch

    b = FleetBatch(sr.p, sr.tb, sr.tf)
    b.set_start_schedule(sr.starts)
    b.set_rainflow_count_all(True)  # (by default the count stops at the episode's last degradation row: tests/test_rf_tail_gpu.py)
    dev = torch.device("cuda", 0)
    out = (torch.zeros((E, b.obs_dim), device=dev), torch.zeros(E, device=dev, dtype=torch.float64), torch.zeros(E, device=dev, dtype=torch.uint8))
    b.reset_dev(out[0].data_ptr())
    return b, out


def _check_book(b, sr, s, where):
    np.testing.assert_array_equal(b.get("rf_len"), sr.book["rf_len"][s], err_msg=f"rainflow_length, {where}")
    for f in ("fd_cyc", "fd_cal", "sei_l"):
        np.testing.assert_allclose(b.get(f), sr.book[f][s], rtol=1e-9, atol=1e-18, err_msg=f"{f}, {where}")
    np.testing.assert_allclose(b.get("soh"), sr.book["soh"][s], rtol=1e-10, err_msg=f"soh, {where}")


def _state(b):
    """Every section of the saved state; of a rainflow row its live part (header and the stack words below the top entry: what lies
    beyond was never written or holds popped entries)."""
    got = {k: np.array(v).view(np.uint8) for k, v in b.state_dict().items()}
    rows = got["rf_rows"].view(np.uint64)
    live = 6 + np.maximum(b.get("rf_stack").astype(np.int64) - 1, 0)
    rows[np.arange(rows.shape[2])[None, None, :] >= live[:, :, None]] = 0
    return got


def test_the_series_hold_every_depth_and_closure_count(series):
    missing = [dk for dk in PAIRS if not series.hist.get(dk)]
    assert not missing, f"(stack points with the pushed one, closures) never produced: {missing}"
    print({dk: series.hist[dk] for dk in PAIRS})
    assert any({0, 1, 2, 3, 4} <= ks for step in series.closed_by_wave for ks in step)  # in ONE wavefront and step
    assert series.stack.max() >= 13 and max(k for _, k in series.hist) >= 5
    # pushes of two and more closures whose cycles carry stress (index >= rainflow_length - 1): in the first day (rainflow_length 1)
    # and between the two daily rows
    assert series.stressed_multi[0] > 100 and series.stressed_multi[1] > 100, series.stressed_multi
    daily = (np.asarray(series.tb.hour)[series.time_idx] == 14) & (np.asarray(series.tb.minute)[series.time_idx] == 45)
    assert (daily.sum(axis=0) == 2).all()  # every env passed two daily rows


def test_step_by_step_against_the_streaming_count_and_the_oracle_and_the_queue_run(series):
    import torch

    sr = series
    tape = torch.from_numpy(sr.acts).to("cuda:0")
    torch.cuda.synchronize()
    b, out = _handle(sr)
    for s in range(STEPS):
        b.step_dev(tape[s].data_ptr(), *(t.data_ptr() for t in out))
        b.synchronize()
        np.testing.assert_array_equal(b.get("rf_cycles"), sr.cycles[s], err_msg=f"closed cycles, step {s}")
        np.testing.assert_array_equal(b.get("rf_stack"), sr.stack[s], err_msg=f"stack size, step {s}")
        _check_book(b, sr, s, f"step {s}")
    b.check_errors()
    # the same tape as one run on the library's own queue: the state-only twin for all launches but the last
    q, qout = _handle(sr)
    q.run_tape_dev(STEPS, tape.data_ptr(), STEPS, *(t.data_ptr() for t in qout), use_graph=_capi.LAUNCH_DIRECT)
    q.synchronize()
    q.check_errors()
    assert q.direct_packet_counts() == (1, STEPS - 1)
    np.testing.assert_array_equal(q.get("rf_cycles"), sr.cycles[-1])
    np.testing.assert_array_equal(q.get("rf_stack"), sr.stack[-1])
    _check_book(q, sr, STEPS - 1, "end of the queue run")
    want, got = _state(b), _state(q)
    assert want.keys() == got.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"state section {k}: queue run vs single launches")
    for w, g, what in zip(out, qout, ("obs", "reward", "done")):
        np.testing.assert_array_equal(g.cpu().numpy(), w.cpu().numpy(), err_msg=what)
    b.close(); q.close()


def test_k_step_launch_against_the_streaming_count_and_the_oracle(series):
    import torch

    sr = series
    tape = torch.from_numpy(sr.acts).to("cuda:0")
    torch.cuda.synchronize()
    b, out = _handle(sr)
    rsum = torch.zeros(E, device="cuda:0", dtype=torch.float64)
    dcnt = torch.zeros(E, device="cuda:0", dtype=torch.int32)
    done = 0
    for K in (PERIOD + 3, STEPS - (PERIOD + 3)):  # the first launch ends between two closing pushes
        b.step_many_dev(K, tape[done:].data_ptr(), out[0].data_ptr(), rsum.data_ptr(), dcnt.data_ptr())
        b.synchronize()
        done += K
        np.testing.assert_array_equal(b.get("rf_cycles"), sr.cycles[done - 1], err_msg=f"closed cycles after {done} steps")
        np.testing.assert_array_equal(b.get("rf_stack"), sr.stack[done - 1], err_msg=f"stack size after {done} steps")
        _check_book(b, sr, done - 1, f"after {done} steps")
    b.check_errors()
    b.close()
