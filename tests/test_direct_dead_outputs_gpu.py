"""A run on the library's own queue (FLEET_LAUNCH_DIRECT) stores observation rows in its LAST launch only: every other launch of the
run carries the "outputs are dead" argument and skips what feeds only the row (fleetrl_amd/csrc/fleet_kernels.hip, "Dead outputs";
fleet_direct.hip keeps two argument blocks per tape row and picks per packet).  What a caller can see must not change: after a run
the observations, rewards, done flags and every field `get()` exposes are the eager stream launches' -- bit for bit, for runs of one
step, runs that end on any tape row, runs that end on a reset step, runs back to back on the same prepared blocks, and the
timed-regions entry.  The two-queue (split) layout cannot be forced at a small shape (the threshold is a compile-time constant of
the library): it is covered by tests/test_direct_gpu.py::test_large_batch_runs_on_two_queues_bit_identically and the 16384-env case
of test_direct_long_run_at_the_bench_shapes only.  Needs an MI355X."""
import numpy as np
import pytest

from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu

TAPE_LEN = 7
# several envs per wavefront | one wavefront per env with surplus lanes | an env of four wavefronts
SHAPES = [(8, 5), (6, 50), (3, 130)]
# 24 h episodes = 96 steps, all envs in lock step: K = 200 crosses two episode ends with auto-reset, K = 192 ENDS on a reset step
RUNS = [1, 2, 7, 8, 192, 200]
_SETUP = {}


def _setup(E, N):
    """Tables, parameters and the seeded tape of a shape: made once, shared, never modified."""
    if (E, N) not in _SETUP:
        from fleetrl_amd.config import resolve_config
        from fleetrl_amd.params import make_params, time_features
        from test_hip_shapes import _cfg, _tables

        tb = _tables("ct", N)
        p = make_params(resolve_config(_cfg("ct", "rainflow", False, aux=True, building=True, pv=True, episode_length=24)), tb, E, seed=5)
        acts = np.random.default_rng(1000 * E + N).uniform(-1, 1, size=(TAPE_LEN, E, N)).astype(np.float32)
        acts.setflags(write=False)
        _SETUP[(E, N)] = (tb, p, time_features(tb), acts)
    return _SETUP[(E, N)]


class _Side:
    """One batch with its output buffers; the observation buffer is filled with NaN after the reset, so a row no launch wrote shows."""

    def __init__(self, E, N, mode):
        import torch
        from fleetrl_amd.batch import FleetBatch

        tb, p, tf, acts = _setup(E, N)
        dev = torch.device("cuda", 0)
        self.mode = mode
        self.b = FleetBatch(p, tb, tf)
        self.tape = torch.from_numpy(np.array(acts)).to(dev)
        self.obs = torch.zeros((E, self.b.obs_dim), device=dev)
        self.reward = torch.zeros(E, device=dev, dtype=torch.float64)
        self.done = torch.zeros(E, device=dev, dtype=torch.uint8)
        self.b.reset_dev(self.obs.data_ptr())
        self.b.synchronize()
        self.obs.fill_(float("nan"))
        torch.cuda.synchronize()

    def ptrs(self):
        return self.tape.data_ptr(), TAPE_LEN, self.obs.data_ptr(), self.reward.data_ptr(), self.done.data_ptr()

    def run(self, steps):
        self.b.run_tape_dev(steps, *self.ptrs(), use_graph=self.mode)
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
    for f, (_, dtype, _) in _capi.FIELDS.items():
        got, want = direct.b.get(f), eager.b.get(f)
        raw = {4: np.uint32, 8: np.uint64}.get(np.dtype(dtype).itemsize)
        if raw is not None and np.dtype(dtype).kind == "f":
            got, want = got.view(raw), want.view(raw)
        np.testing.assert_array_equal(got, want, err_msg=f"{f} {what}")
    direct.b.check_errors()


@pytest.mark.parametrize("K", RUNS)
@pytest.mark.parametrize("E,N", SHAPES)
def test_one_run_of_k_steps_equals_the_eager_launches(E, N, K):
    d, e = _Side(E, N, _capi.LAUNCH_DIRECT), _Side(E, N, _capi.LAUNCH_EAGER)
    d.run(K)
    e.run(K)
    _assert_same(d, e, f"after one run of {K}")
    if K >= 192:
        assert e.b.get("episodes").min() >= 2  # the run crossed the episode ends it is here for
    if K == 192:
        assert (e.b.get("ep_len") == 0).all()  # ... and its last launch was the reset step
    d.close(); e.close()


@pytest.mark.parametrize("E,N", SHAPES)
def test_runs_back_to_back_on_the_same_prepared_blocks(E, N):
    """No re-preparation between the runs (same tape, same buffers, same handle): each run's last launch must take the storing block
    of the tape row IT ends on -- rows 4, 2, 0 and 5 of 7 here --, and a run of one step the storing first-launch block."""
    import torch

    d, e = _Side(E, N, _capi.LAUNCH_DIRECT), _Side(E, N, _capi.LAUNCH_EAGER)
    for steps in (5, 10, 1, 13):
        assert steps == 1 or steps % TAPE_LEN != 0
        d.obs.fill_(float("nan"))
        torch.cuda.synchronize()
        d.run(steps)
        e.run(steps)
        _assert_same(d, e, f"after the run of {steps}")
    d.close(); e.close()


@pytest.mark.parametrize("E,N", SHAPES)
def test_timed_regions_store_the_outputs_of_every_regions_last_launch(E, N):
    """Three regions of five steps, chained without a wait in between: the outputs after the read are those of fifteen eager steps
    (every region replays the tape from its first row, as every run does)."""
    d, e = _Side(E, N, _capi.LAUNCH_DIRECT), _Side(E, N, _capi.LAUNCH_EAGER)
    d.b.time_regions_begin(3, 5, *d.ptrs(), use_graph=_capi.LAUNCH_DIRECT)
    ms = d.b.time_regions_read()
    assert ms.shape == (3,) and (ms > 0).all()
    for _ in range(3):
        e.run(5)
    _assert_same(d, e, "after 3 timed regions of 5")
    assert (e.b.get("ep_len") == 15).all()
    d.close(); e.close()
