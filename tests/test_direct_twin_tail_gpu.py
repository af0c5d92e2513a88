"""The tail of the step kernel's state-only twin (fleetrl_amd/csrc/fleet_kernels.hip, `kTailA` / `kTailB` / `kTailC`; DESIGN.md
section 4 "The state-only twin"): the row request's scalars fetched at the entry, ONE late fetch of everything the rest of the step
reads of the kernel-argument segment (the self-check, the leader's overload constants, `auto_reset`, the placement guard's piece),
the env record stored through the preloaded pointer with the reset's flag re-read inside the reset branch.  None of it changes a value: the same seeded tape is run (a) on the library's queue with the
twin, (b) on the queue with the twin switched off (`fleet_set_direct_state_only(h, 0)`: the live instance, whose tail is untouched),
(c) as single launches on the HIP stream, and everything that can be read afterwards must agree bit for bit -- every section of the
saved state, the rainflow fields, the error words, the last step's obs / reward / done -- and the final state must meet the CPU
oracle at the project's parity tolerances (tests/test_hip_shapes.py).

Shapes: whole multiples of 8 workgroups, the last one partly filled where a workgroup holds several envs -- E = 29 x N = 50 (G64,
three surplus groups: wavefronts with `env_ok == false` walk the new tail too), E = 15 x N = 100 (G128, one surplus group), E = 8 x
N = 200 (G256, the LDS meeting point).  Runs of 1, 2, 3 and 200 steps back to back on the same prepared blocks; episodes of 48 h (192
steps), so the run of 200 crosses the episode end -- an auto-reset inside a dead launch: the moved flag re-read -- and two 14:45 rows.
One case has a grid connection so small that the leader's overload branch fires in most steps (the late block's constants); its
precondition -- the oracle's `penalty_record` differs from the default grid connection's on at least half of the envs -- is asserted.
Needs an MI355X."""
import numpy as np
import pytest

from fleetrl_amd import _capi

pytestmark = pytest.mark.gpu

FIELDS = ("ep_return", "last_ep_return", "penalty_record", "error_bits", "rf_cycles", "rf_stack", "rf_len")
RUNS = (1, 2, 3, 200)
TAPE_LEN = 11
EPISODE_H = 48  # 192 steps: the 200-step run ends the episode at its launch 186, a dead one
SMALL_GRID = 20.0  # kW; the default of the synthetic caretaker fleet is hundreds

CASES = [  # N, E, grid connection (None: the configuration's)
    (50, 29, None),
    (100, 15, None),
    (200, 8, None),
    (50, 29, SMALL_GRID),
]
_IDS = [f"N{n}-E{e}-{'grid' + str(int(g)) if g else 'default'}" for n, e, g in CASES]


def _setup(N, E, grid):
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.params import make_params, time_features
    from test_hip_shapes import _cfg, _tables

    tb = _tables("ct", N)
    p = make_params(resolve_config(_cfg("ct", "rainflow", False, episode_length=EPISODE_H)), tb, E, seed=5)
    if grid is not None:
        p.grid_connection = grid
    return p, tb, time_features(tb)


def _tape(N, E):
    rng = np.random.default_rng(1000 * N + E)
    acts = rng.uniform(-1, 1, size=(TAPE_LEN, E, N))
    acts[rng.uniform(size=acts.shape) < 0.15] = 0.0
    return acts.astype(np.float32)


_ORACLE = {}


def _oracle(N, E, grid):
    """The CPU oracle stepped through the same runs (every run replays the tape from row 0): final state and last outputs.  Computed
    once per case and shared."""
    key = (N, E, grid)
    if key not in _ORACLE:
        from oracle.fleet_oracle import OracleBatch

        p, tb, tf = _setup(N, E, grid)
        cpu = OracleBatch(p, tb, tf, threads=4)
        acts = _tape(N, E)
        cpu.reset()
        for steps in RUNS:
            for k in range(steps):
                o, r, d, _ = cpu.step(acts[k % TAPE_LEN])
        res = {f: np.array(cpu.get(f)) for f in ("time_idx", "hours_left", "episodes", "soc", "soh", "ep_return", "last_ep_return",
                                                   "penalty_record", "rf_len", "fd_cyc", "sei_l", "error_bits")}
        res.update(obs=np.array(o), reward=np.array(r), done=np.array(d))
        cpu.close()
        _ORACLE[key] = res
    return _ORACLE[key]


class _Way:
    """One handle, its output buffers and how it launches."""

    def __init__(self, N, E, grid, mode, twin):
        import torch
        from fleetrl_amd.batch import FleetBatch

        self.b = FleetBatch(*_setup(N, E, grid))
        self.mode = mode
        dev = torch.device("cuda", 0)
        self.out = (torch.zeros((E, self.b.obs_dim), device=dev), torch.zeros(E, device=dev, dtype=torch.float64),
                    torch.zeros(E, device=dev, dtype=torch.uint8))
        if twin is not None:
            self.b.set_direct_state_only(twin)
        self.b.reset_dev(self.out[0].data_ptr())

    def run(self, steps, tape):
        self.b.run_tape_dev(steps, tape.data_ptr(), TAPE_LEN, *(t.data_ptr() for t in self.out), use_graph=self.mode, act_dtype=_capi.ACT_F32)
        self.b.synchronize()

    def everything(self):
        got = {f"out.{k}": t.cpu().numpy() for k, t in zip(("obs", "reward", "done"), self.out)}
        got.update({f"get.{f}": self.b.get(f) for f in FIELDS})
        got.update({f"state.{k}": np.array(v).view(np.uint8) for k, v in self.b.state_dict().items()})
        # of a rainflow row the live part is state -- the 6 header words and the stack words below the top entry; the words beyond
        # were never written or are popped entries (tests/test_direct_state_only_twin_gpu.py)
        rows = got["state.rf_rows"].view(np.uint64)
        live = 6 + np.maximum(got["get.rf_stack"].astype(np.int64) - 1, 0)
        rows[np.arange(rows.shape[2])[None, None, :] >= live[:, :, None]] = 0
        return got


def _same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")


def test_the_small_grid_connection_makes_the_overload_branch_fire():
    """The precondition of the overload case, on the CPU oracle alone: with the small grid connection the episode's penalty record
    differs from the default configuration's on at least half of the envs (it does on every env: any charging fleet overloads 20 kW)."""
    N, E = 50, 29
    small, default = _oracle(N, E, SMALL_GRID)["penalty_record"], _oracle(N, E, None)["penalty_record"]
    assert (small != default).sum() * 2 >= E
    assert (small < default).sum() * 2 >= E  # penalties are negative: more of them


@pytest.mark.parametrize("N,E,grid", CASES, ids=_IDS)
def test_twin_tail_equals_flag_equals_stream_and_meets_the_oracle(N, E, grid):
    import torch

    assert _capi.step_has_state_only(E, N, 2, False, False, _capi.ACT_F32)
    tape = torch.from_numpy(_tape(N, E)).to("cuda:0")
    ways = {"twin": _Way(N, E, grid, _capi.LAUNCH_DIRECT, True), "flag": _Way(N, E, grid, _capi.LAUNCH_DIRECT, False),
            "stream": _Way(N, E, grid, _capi.LAUNCH_EAGER, None)}
    live = dead = 0
    episodes0 = ways["stream"].b.get("episodes").copy()
    for steps in RUNS:  # back to back, everything read in between
        for w in ways.values():
            w.run(steps, tape)
        want = ways["stream"].everything()
        _same(ways["twin"].everything(), want, f"twin vs stream after a run of {steps}")
        _same(ways["flag"].everything(), want, f"flag vs stream after a run of {steps}")
        live, dead = live + 1, dead + steps - 1
        assert ways["twin"].b.direct_packet_counts() == (live, dead)      # the twin for every launch but a run's last
        assert ways["flag"].b.direct_packet_counts() == (live + dead, 0)  # switched off: the live instance throughout
    assert (ways["stream"].b.get("episodes") - episodes0).min() >= 1      # every env went through the in-launch reset
    for w in ways.values():
        w.b.check_errors()

    # the twin's final state and last outputs against the CPU oracle (tolerances: tests/test_hip_shapes.py)
    b, ref = ways["twin"].b, _oracle(N, E, grid)
    if grid is not None:
        assert (ref["penalty_record"] != _oracle(N, E, None)["penalty_record"]).sum() * 2 >= E  # the overload branch fired
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
