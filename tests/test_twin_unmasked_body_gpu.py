"""The lane body of the step kernel's state-only twin without an exec-mask region around it (fleetrl_amd/csrc/fleet_kernels.hip,
`kBody`; DESIGN.md section 4 "The state-only twin"): every lane of the twin runs the body, a surplus lane (g >= N) on the env's last
EV with its stores, its rainflow push and its sums switched off.  None of it changes a value: the same seeded tape is run (a) on the
library's queue with the twin, (b) on the queue with the twin switched off (`set_direct_state_only(0)`: the live instance, whose
body is still a masked region), (c) as single launches on the HIP stream, and everything that can be read afterwards must agree bit
for bit -- every section of the saved state (rainflow rows masked to their live words), the `get` fields, the error words, the last
step's obs / reward / done -- and the final state must meet the CPU oracle at the project's parity tolerances
(tests/test_hip_shapes.py).  The three ways and the comparison are those of tests/test_direct_twin_tail_gpu.py.

Shapes (N EVs x E envs), the smallest at which the change can go wrong:
  50 x 29   G64: 14 surplus lanes, the leader lane is one of them; three surplus groups (`env_ok == false`)
  64 x 5    G64: no surplus lane; the leader IS an EV lane and its sums must not be zeroed
  33 x 9    G64: 31 surplus lanes
  65 x 7    G128: the second wavefront holds one real lane
  129 x 4   G256: one wavefront with one real lane, one wholly surplus (it runs the clamped body too)
  200 x 8   G256: the geometry of the benchmark's c5
Runs of 1, 2, 3 and 200 steps back to back; episodes of 48 h (192 steps), so the run of 200 has the auto-reset inside a dead launch
and two 14:45 rows.

Precondition, asserted per case on the CPU oracle's samples of the 200-step run: EV N-1 -- the EV the surplus lanes copy -- pushes a
reversal point and closes a cycle (what changes `rf_stack` / `rf_cycles`; the oracle has no such fields, so both are read off its
`soc_deg` samples, `_precondition` says how), crosses a schedule event (`hours_left` turns zero or non-zero) and stands on a 14:45
row that updates its state of health, each before the env's reset and each in at least half of the envs.  A surplus lane that
stored, pushed or added to the sums would then have had something to get wrong.  Needs an MI355X (the precondition test alone
does not touch it)."""
import numpy as np
import pytest

from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu

CASES = [(50, 29), (64, 5), (33, 9), (65, 7), (129, 4), (200, 8)]  # N, E
_IDS = [f"N{n}-E{e}" for n, e in CASES]
_ORACLE = {}


def _twin_tail():
    import test_direct_twin_tail_gpu as tt  # the three ways, the tape and the comparison

    return tt


def _oracle(N, E):
    """The CPU oracle stepped through the same runs: final state, last outputs, and EV N-1's samples after the reset and after every
    step.  Computed once per case and shared."""
    if (N, E) not in _ORACLE:
        from oracle.fleet_oracle import OracleBatch

        tt = _twin_tail()
        p, tb, tf = tt._setup(N, E, None)
        cpu = OracleBatch(p, tb, tf, threads=4)
        acts = tt._tape(N, E)
        cpu.reset()
        fields = ("soc_deg", "hours_left", "soh")
        samples = {f: [cpu.get(f)[:, N - 1].copy()] for f in fields}
        episodes = [cpu.get("episodes").copy()]
        for steps in tt.RUNS:
            for k in range(steps):
                o, r, d, _ = cpu.step(acts[k % tt.TAPE_LEN])
                for f in fields:
                    samples[f].append(cpu.get(f)[:, N - 1].copy())
                episodes.append(cpu.get("episodes").copy())
        res = {f: np.array(cpu.get(f)) for f in ("time_idx", "hours_left", "episodes", "soc", "soh", "ep_return", "last_ep_return",
                                                   "penalty_record", "rf_len", "fd_cyc", "sei_l", "error_bits")}
        res.update(obs=np.array(o), reward=np.array(r), done=np.array(d))
        res["last_ev"] = {f: np.array(v) for f, v in samples.items()}  # [1 + 206, E]
        res["last_ev"]["episodes"] = np.array(episodes)
        cpu.close()
        _ORACLE[(N, E)] = res
    return _ORACLE[(N, E)]


def _precondition(N, E):
    """Envs in which EV N-1, inside the 200-step run and before the env's reset, (push) logged a reversal point: a strict change of
    the slope's sign in its `soc_deg` samples, equal samples skipped, which is what changes `rf_stack`; (close) closed a full
    cycle by the three-point rule, which is what changes `rf_cycles` -- the oracle's own rainflow of the episode's samples, a cycle of
    count 1 that ends inside the run; (event) arrived or departed; (daily) had its state of health updated."""
    from oracle.fleet_oracle import rainflow

    tt = _twin_tail()
    s = _oracle(N, E)["last_ev"]
    first = sum(tt.RUNS[:-1])  # sample index of the state the long run starts from
    got = dict(push=0, close=0, event=0, daily=0)
    for e in range(E):
        resets = np.flatnonzero(np.diff(s["episodes"][:, e]) != 0)
        assert len(resets) == 1 and resets[0] >= first, "every env goes through one reset, inside the long run"
        last = resets[0]  # samples first .. last belong to the long run and to the first episode
        x = s["soc_deg"][: last + 1, e]
        moves = np.flatnonzero(np.diff(x) != 0)            # steps that logged a new value
        sign = np.sign(np.diff(x)[moves])
        turn = moves[1:][sign[1:] != sign[:-1]]             # ... whose slope turned: the previous sample becomes a reversal point
        got["push"] += bool((turn >= first).any())
        cyc = rainflow(x)
        got["close"] += bool(((cyc[:, 2] == 1.0) & (cyc[:, 3] > first) & (cyc[:, 3] < last)).any())
        hl = s["hours_left"][first : last + 1, e] != 0
        got["event"] += bool((hl[1:] != hl[:-1]).any())
        got["daily"] += bool((np.diff(s["soh"][first : last + 1, e]) != 0).any())
    return got


@pytest.mark.parametrize("N,E", CASES, ids=_IDS)
def test_the_last_ev_pushes_closes_crosses_an_event_and_is_evaluated(N, E):
    """The precondition of the case, on the CPU oracle alone."""
    got = _precondition(N, E)
    print(f"N={N} E={E}: envs in which EV N-1 meets each clause: {got}")
    for clause, envs in got.items():
        assert envs * 2 >= E, (clause, envs, E)


@pytest.mark.parametrize("N,E", CASES, ids=_IDS)
def test_unmasked_body_twin_equals_flag_equals_stream_and_meets_the_oracle(N, E):
    import torch

    tt = _twin_tail()
    assert _capi.step_has_state_only(E, N, 2, False, False, _capi.ACT_F32)
    for clause, envs in _precondition(N, E).items():
        assert envs * 2 >= E, (clause, envs, E)
    tape = torch.from_numpy(tt._tape(N, E)).to("cuda:0")
    ways = {"twin": tt._Way(N, E, None, _capi.LAUNCH_DIRECT, True), "flag": tt._Way(N, E, None, _capi.LAUNCH_DIRECT, False),
            "stream": tt._Way(N, E, None, _capi.LAUNCH_EAGER, None)}
    live = dead = 0
    episodes0 = ways["stream"].b.get("episodes").copy()
    for steps in tt.RUNS:  # back to back, everything read in between
        for w in ways.values():
            w.run(steps, tape)
        want = ways["stream"].everything()
        tt._same(ways["twin"].everything(), want, f"twin vs stream after a run of {steps}")
        tt._same(ways["flag"].everything(), want, f"flag vs stream after a run of {steps}")
        live, dead = live + 1, dead + steps - 1
        assert ways["twin"].b.direct_packet_counts() == (live, dead)      # the twin for every launch but a run's last
        assert ways["flag"].b.direct_packet_counts() == (live + dead, 0)  # switched off: the live instance throughout
    assert (ways["stream"].b.get("episodes") - episodes0).min() >= 1      # every env went through the in-launch reset
    for w in ways.values():
        w.b.check_errors()

    # the twin's final state and last outputs against the CPU oracle (tolerances: tests/test_hip_shapes.py)
    b, ref = ways["twin"].b, _oracle(N, E)
    for f in ("time_idx", "hours_left", "episodes", "rf_len"):
        np.testing.assert_array_equal(b.get(f), ref[f], err_msg=f)
    assert not b.get("error_bits").any() and not ref["error_bits"].any()
    for f in ("soc", "soh", "ep_return", "penalty_record"):
        np.testing.assert_allclose(b.get(f), ref[f], rtol=1e-9, atol=1e-9, err_msg=f)
    np.testing.assert_allclose(b.get("last_ep_return"), ref["last_ep_return"], rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(b.get("fd_cyc"), ref["fd_cyc"], rtol=1e-8, atol=1e-18)
    np.testing.assert_allclose(b.get("sei_l"), ref["sei_l"], rtol=1e-9, atol=1e-18)
    obs, rew, done = (t.cpu().numpy() for t in ways["twin"].out)
    np.testing.assert_array_equal(done, ref["done"])
    np.testing.assert_allclose(obs, ref["obs"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rew, ref["reward"], rtol=1e-9, atol=1e-9)
    for w in ways.values():
        w.b.close()
