"""The step kernel's state-only twin (fleetrl_amd/csrc/fleet_kernels.hip, `DEAD`; DESIGN.md section 4 "What a run writes"): on the
library's own queue every launch of a run but its last takes an instance compiled without anything that feeds `obs`, `reward`, `done`
or the cashflow.  The same seeded tape is run three ways -- (a) twin on, (b) twin off: the live instance with its run-time flag,
(c) single launches on the HIP stream -- and everything that can be read afterwards must agree bit for bit: every section of the
saved state (of a rainflow row its live part: what lies beyond the stack was never written), the last step's outputs, and the fields
`get` unpacks.

Shapes: the smallest at which the twin can go wrong.  The queue wants whole multiples of 8 workgroups, and the last workgroup is
partly filled where a workgroup holds several envs: G64 (4 envs per workgroup) with E = 30, G128 (2) with E = 15, G256 (1) with
E = 8; N = 50 / 100 / 130 leave surplus lanes in every group, N = 64 none.  Episodes of 26 h (104 steps), so a run of 250 steps
crosses two auto-resets and the 14:45 degradation row of an episode's second day.  Needs an MI355X.

(`tests/test_direct_state_only_gpu.py` is an older file: the run-time flag's tests against eager stepping.  It stays as it is and now
runs the twin too, since the twin is on by default.)"""
import numpy as np
import pytest

from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu

FIELDS = ("ep_return", "last_ep_return", "rf_cycles", "rf_stack")
RUNS = (1, 2, 3, 250)  # 1: the one launch is live, no twin packet; 2: a recording dead first launch, then the live one; 3: one plain dead launch between
TAPE_LEN = 11

CASES = [  # N, E, degradation, float64 actions
    (50, 30, "rainflow", False),
    (50, 30, "rainflow", True),
    (50, 30, "linear", False),
    (50, 30, "none", False),
    (64, 30, "rainflow", False),
    (100, 15, "rainflow", False),
    (130, 8, "rainflow", False),
]


def _make(N, E, deg):
    from fleetrl_amd.batch import FleetBatch
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params, time_features
    from test_hip_shapes import _cfg, _tables

    tb = _tables("ct", N)
    p = make_params(resolve_config(_cfg("ct", deg, False, episode_length=26)), tb, E, seed=5)
    return FleetBatch(p, tb, time_features(tb))


class _Way:
    """One handle, its output buffers and how it launches."""

    def __init__(self, N, E, deg, f64, mode, twin):
        import torch

        self.b = _make(N, E, deg)
        self.mode, self.f64 = mode, f64
        dev = torch.device("cuda", 0)
        self.out = (torch.zeros((E, self.b.obs_dim), device=dev), torch.zeros(E, device=dev, dtype=torch.float64),
                    torch.zeros(E, device=dev, dtype=torch.uint8))
        if twin is not None:
            self.b.set_direct_state_only(twin)
        self.b.reset_dev(self.out[0].data_ptr())

    def run(self, steps, tape):
        self.b.run_tape_dev(steps, tape.data_ptr(), TAPE_LEN, *(t.data_ptr() for t in self.out), use_graph=self.mode,
                            act_dtype=_capi.ACT_F64 if self.f64 else _capi.ACT_F32)
        self.b.synchronize()

    def everything(self):
        got = {f"out.{k}": t.cpu().numpy() for k, t in zip(("obs", "reward", "done"), self.out)}
        got.update({f"get.{f}": self.b.get(f) for f in FIELDS})
        got.update({f"state.{k}": np.array(v).view(np.uint8) for k, v in self.b.state_dict().items()})
        # of a rainflow row the live part is state -- the 6 header words and the stack words below the top entry (stack size - 1 of
        # them; the top is in the header); the words beyond were never written or are popped entries: they may hold anything
        if "state.rf_rows" in got:
            rows = got["state.rf_rows"].view(np.uint64)
            live = 6 + np.maximum(got["get.rf_stack"].astype(np.int64) - 1, 0)
            rows[np.arange(rows.shape[2])[None, None, :] >= live[:, :, None]] = 0
        return got


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")


@pytest.mark.parametrize("N,E,deg,f64", CASES, ids=[f"N{n}-E{e}-{d}-{'f64' if f else 'f32'}" for n, e, d, f in CASES])
def test_twin_equals_flag_equals_stream(N, E, deg, f64):
    import torch

    assert _capi.step_has_state_only(E, N, {"none": 0, "linear": 1, "rainflow": 2}[deg], False, False,
                                     _capi.ACT_F64 if f64 else _capi.ACT_F32)
    rng = np.random.default_rng(1000 * N + E)
    acts = rng.uniform(-1, 1, size=(TAPE_LEN, E, N))
    acts[rng.uniform(size=acts.shape) < 0.15] = 0.0
    tape = torch.from_numpy(acts if f64 else acts.astype(np.float32)).to("cuda:0")
    ways = {"twin": _Way(N, E, deg, f64, _capi.LAUNCH_DIRECT, True), "flag": _Way(N, E, deg, f64, _capi.LAUNCH_DIRECT, False),
            "stream": _Way(N, E, deg, f64, _capi.LAUNCH_EAGER, None)}
    live = dead = 0
    episodes0 = ways["stream"].b.get("episodes").copy()
    for steps in RUNS:  # back to back with everything read in between: a live last launch, then the next run's recording dead first launch
        for w in ways.values():
            w.run(steps, tape)
        want = ways["stream"].everything()
        _same(ways["twin"].everything(), want, f"twin vs stream after a run of {steps}")
        _same(ways["flag"].everything(), want, f"flag vs stream after a run of {steps}")
        live, dead = live + 1, dead + steps - 1
        assert ways["twin"].b.direct_packet_counts() == (live, dead)           # the twin for every launch but a run's last
        assert ways["flag"].b.direct_packet_counts() == (live + dead, 0)       # switched off: one kernel object
        assert ways["twin"].b.direct_queues() == 1 and ways["flag"].b.direct_queues() == 1
    assert (ways["stream"].b.get("episodes") - episodes0).min() >= 2          # every env was reset twice inside the runs
    for w in ways.values():
        w.b.check_errors()
        w.b.close()


def test_switching_the_twin_off_and_on_again_rebuilds_the_run():
    """One handle: on, off, on.  Every switch takes effect at the next run and the results stay those of the stream launches."""
    import torch

    N, E = 50, 30
    rng = np.random.default_rng(77)
    tape = torch.from_numpy(rng.uniform(-1, 1, size=(TAPE_LEN, E, N)).astype(np.float32)).to("cuda:0")
    a, s = _Way(N, E, "rainflow", False, _capi.LAUNCH_DIRECT, None), _Way(N, E, "rainflow", False, _capi.LAUNCH_EAGER, None)
    counts = [a.b.direct_packet_counts()]
    assert counts[0] == (0, 0)
    for on in (None, False, True):  # None: the default, which is on
        if on is not None:
            a.b.set_direct_state_only(on)
        a.run(40, tape)
        s.run(40, tape)
        _same(a.everything(), s.everything(), f"switch {on}")
        counts.append(a.b.direct_packet_counts())
    assert counts[1:] == [(1, 39), (41, 39), (42, 78)]
    a.b.check_errors()
    a.b.close(); s.b.close()


def test_a_configuration_without_a_twin_is_unchanged():
    """8-lane groups have no twin: the switch changes nothing, every packet takes the live instance."""
    import torch

    N, E = 5, 250
    assert not _capi.step_has_state_only(E, N, 2, False, False)
    rng = np.random.default_rng(3)
    tape = torch.from_numpy(rng.uniform(-1, 1, size=(TAPE_LEN, E, N)).astype(np.float32)).to("cuda:0")
    a, s = _Way(N, E, "rainflow", False, _capi.LAUNCH_DIRECT, True), _Way(N, E, "rainflow", False, _capi.LAUNCH_EAGER, None)
    for steps in (3, 120):
        a.run(steps, tape)
        s.run(steps, tape)
        _same(a.everything(), s.everything(), f"after a run of {steps}")
    assert a.b.direct_packet_counts() == (123, 0)
    a.b.check_errors()
    a.b.close(); s.b.close()
