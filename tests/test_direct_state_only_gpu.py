"""Every launch of a run on the library's own queue (FLEET_LAUNCH_DIRECT) but the last one does STATE work only: it stores no
observation row, no reward, no done flag and no cashflow, and its auto-reset writes no start row (fleetrl_amd/csrc/fleet_kernels.hip,
"Dead outputs"); the single-step kernel requests the rainflow row of a pushing EV in the middle of the step and first reads it in
rf_finish.  What a caller can see must not change: after every run the observations, rewards, done flags, every field `get()` exposes, the saved state
blob and the error word are those of eager `step_dev` stepping of a twin handle -- bit for bit.

Shapes: the smallest at which each lane mapping can go wrong -- one wavefront per env with surplus lanes and a surplus group in the
last workgroup (5 x 50), several envs per wavefront with a ragged last wavefront (37 x 5), an env of four wavefronts with the sums
in the LDS (3 x 200).  Episodes are 24 h = 96 steps with all envs in lock step, so a 14:45 row and a reset fall inside the longer
runs.  Needs an MI355X."""
import numpy as np
import pytest

from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu

TAPE_LEN = 7
EP_STEPS = 96
SHAPES = [(5, 50), (37, 5), (3, 200)]
# 1, 2, 3 steps; a run that ENDS on the reset step, and that plus 1
RUNS = [1, 2, 3, EP_STEPS, EP_STEPS + 1]
_SETUP = {}


def _setup(E, N):
    """Tables, parameters and the seeded tape of a shape: made once, shared, never modified."""
    if (E, N) not in _SETUP:
        from fleetrl_amd.config import resolve_config
        from fleetrl_amd.params import make_params, time_features
        from test_hip_shapes import _cfg, _tables

        tb = _tables("ct", N)
        p = make_params(resolve_config(_cfg("ct", "rainflow", False, aux=True, building=True, pv=True, episode_length=24)), tb, E, seed=11)
        acts = np.random.default_rng(77 * E + N).uniform(-1, 1, size=(TAPE_LEN, E, N)).astype(np.float32)
        acts.setflags(write=False)
        _SETUP[(E, N)] = (tb, p, time_features(tb), acts)
    return _SETUP[(E, N)]


class _Side:
    """One batch with its output buffers.  `direct`: runs go to the library's queue; else every step is one eager `step_dev`.  The
    observation buffer is filled with NaN after the reset, so a row no launch wrote shows.  `twin_of`: start from that side's state
    blob -- the stack words of the rainflow rows beyond an EV's stack are never initialised, and only a loaded twin holds the same
    bytes there, so that whole blobs can be compared afterwards."""

    def __init__(self, E, N, direct, count_all=False, twin_of=None):
        import torch
        from fleetrl_amd.batch import FleetBatch

        tb, p, tf, acts = _setup(E, N)
        dev = torch.device("cuda", 0)
        self.direct = direct
        self.b = FleetBatch(p, tb, tf)
        if count_all:
            self.b.set_rainflow_count_all(True)  # takes effect at the reset below
        self.tape = torch.from_numpy(np.array(acts)).to(dev)
        self.obs = torch.zeros((E, self.b.obs_dim), device=dev)
        self.reward = torch.zeros(E, device=dev, dtype=torch.float64)
        self.done = torch.zeros(E, device=dev, dtype=torch.uint8)
        self.b.reset_dev(self.obs.data_ptr())
        self.b.synchronize()
        if twin_of is not None:
            self.b.load_state(twin_of.b.save_state())
        self.obs.fill_(float("nan"))
        torch.cuda.synchronize()

    def ptrs(self):
        return self.tape.data_ptr(), TAPE_LEN, self.obs.data_ptr(), self.reward.data_ptr(), self.done.data_ptr()

    def run(self, steps):
        """Every run replays the tape from its first row."""
        if self.direct:
            self.b.run_tape_dev(steps, *self.ptrs(), use_graph=_capi.LAUNCH_DIRECT)
        else:
            for k in range(steps):
                self.b.step_dev(self.tape[k % TAPE_LEN].data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(), self.done.data_ptr())
        self.b.synchronize()

    def close(self):
        self.b.close()


def _assert_same(direct, eager, what):
    obs = direct.obs.cpu().numpy()
    assert not np.isnan(obs).any(), f"{what}: the run left observation slots unwritten"
    # (bit patterns: array_equal on the float views would let -0.0 pass for 0.0)
    np.testing.assert_array_equal(obs.view(np.uint32), eager.obs.cpu().numpy().view(np.uint32), err_msg=f"obs {what}")
    np.testing.assert_array_equal(direct.reward.cpu().numpy().view(np.uint64), eager.reward.cpu().numpy().view(np.uint64), err_msg=f"reward {what}")
    np.testing.assert_array_equal(direct.done.cpu().numpy(), eager.done.cpu().numpy(), err_msg=f"done {what}")
    for f, (_, dtype, _) in _capi.FIELDS.items():  # cashflow, ep_return, penalty_record and last_ep_return among them
        got, want = direct.b.get(f), eager.b.get(f)
        raw = {4: np.uint32, 8: np.uint64}.get(np.dtype(dtype).itemsize)
        if raw is not None and np.dtype(dtype).kind == "f":
            got, want = got.view(raw), want.view(raw)
        np.testing.assert_array_equal(got, want, err_msg=f"{f} {what}")
    np.testing.assert_array_equal(direct.b.save_state(), eager.b.save_state(), err_msg=f"state blob {what}")
    direct.b.check_errors()
    eager.b.check_errors()


@pytest.mark.parametrize("K", RUNS)
@pytest.mark.parametrize("E,N", SHAPES)
def test_one_run_of_k_steps_equals_eager_stepping(E, N, K):
    d = _Side(E, N, True)
    e = _Side(E, N, False, twin_of=d)
    d.run(K)
    e.run(K)
    _assert_same(d, e, f"after one run of {K}")
    if K == EP_STEPS:
        assert (e.b.get("episodes") >= 1).all() and (e.b.get("ep_len") == 0).all()  # the run's last launch was the reset step
    if K == EP_STEPS + 1:
        assert (e.b.get("ep_len") == 1).all()  # ... and here a dead launch: the row its reset would store is the next launch's
    d.close(); e.close()


@pytest.mark.parametrize("E,N", SHAPES)
def test_two_runs_back_to_back_on_the_same_prepared_blocks(E, N):
    """No re-preparation between the runs (same tape, same buffers, same handle).  The second run crosses the episode end."""
    import torch

    d = _Side(E, N, True)
    e = _Side(E, N, False, twin_of=d)
    for steps in (5, EP_STEPS - 3):
        d.obs.fill_(float("nan"))
        torch.cuda.synchronize()
        d.run(steps)
        e.run(steps)
        _assert_same(d, e, f"after the run of {steps}")
    assert (e.b.get("episodes") >= 1).all()
    d.close(); e.close()


@pytest.mark.parametrize("E,N", SHAPES)
def test_one_timed_regions_call(E, N):
    """Three regions of five steps, chained without a wait in between: the outputs after the read are those of fifteen eager steps
    (every region replays the tape from its first row, as every run does)."""
    d = _Side(E, N, True)
    e = _Side(E, N, False, twin_of=d)
    d.b.time_regions_begin(3, 5, *d.ptrs(), use_graph=_capi.LAUNCH_DIRECT)
    ms = d.b.time_regions_read()
    assert ms.shape == (3,) and (ms > 0).all()
    for _ in range(3):
        e.run(5)
    _assert_same(d, e, "after 3 timed regions of 5")
    assert (e.b.get("ep_len") == 15).all()
    d.close(); e.close()


def test_pushes_on_every_step_of_a_run_with_the_count_kept_running():
    """`set_rainflow_count_all`: the count does not stop at the episode's last degradation row, so reversal points are pushed -- and
    the row is requested and consumed -- in every launch of the run, the dead ones included, up to the reset."""
    E, N = SHAPES[0]
    d = _Side(E, N, True, count_all=True)
    e = _Side(E, N, False, count_all=True, twin_of=d)
    before = e.b.get("rf_cycles").astype(np.int64) + e.b.get("rf_stack")
    d.run(EP_STEPS - 1)
    e.run(EP_STEPS - 1)
    _assert_same(d, e, f"after a run of {EP_STEPS - 1} with the count kept running")
    assert ((e.b.get("rf_cycles").astype(np.int64) + e.b.get("rf_stack")) > before).any()  # points were pushed
    d.close(); e.close()
