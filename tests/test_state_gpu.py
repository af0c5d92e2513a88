"""Env state on the device (include/fleet_hip.h "env state"): save / load of a whole handle and the fork of chosen envs.  Every
comparison between two runs of the library is bit for bit -- these are copies; only the comparisons with the CPU oracle carry the
tolerances of tests/golden_util.py (obs 1e-5, float64 state 1e-9).  Needs an MI355X."""
import copy

import numpy as np
import pytest

from fleetrl_amd import _capi
from fleetrl_amd.config import resolve_config
from fleetrl_amd.params import make_params, time_features
from test_hip_shapes import _cfg, _tables

pytestmark = pytest.mark.gpu

FIELDS = tuple(_capi.FIELDS)
FKEYS = tuple("f_" + k for k in FIELDS)  # (the getter fields have a "done" of their own: episode.done, not the step's output)
EP = 96  # rows of a 24 h episode


def _make(uc, n_evs, E, deg, *, seed=1, real_time=False, log=False, picker="random", auto_reset=True, env_id_offset=0):
    cfg = _cfg(uc, deg, False, real_time=real_time)
    cfg["log_data"] = log
    cfg["time_picker"] = picker
    tb = _tables(uc, n_evs)
    p = make_params(resolve_config(cfg), tb, E, seed=seed, auto_reset=auto_reset, env_id_offset=env_id_offset)
    return p, tb, time_features(tb)


def _batch(args):
    from fleetrl_amd.batch import FleetBatch

    return FleetBatch(*args)


def _fields(b, names=FIELDS):
    return {"f_" + k: b.get(k) for k in names}


def _tape(rng, K, E, N):
    """Random actions with idle stretches, full-power stretches and 15 % zeros: SOC series with reversals of many sizes."""
    a = rng.uniform(-1, 1, size=(K, E, N))
    for k in range(K):
        if (k // 9) % 4 == 3:
            a[k] = np.abs(a[k])
    a[rng.random(a.shape) < 0.15] = 0.0
    return a.astype(np.float32)


def _run(b, tape, with_fields=True, log=False):
    """Step `b` through the tape; everything a caller can see after each step."""
    out = []
    for a in tape:
        obs, rew, done, term = b.step(a)
        d = done.astype(bool)
        rec = {"obs": obs.copy(), "reward": rew.copy(), "done": done.copy(), "term": term * d[:, None]}  # (rows of done envs only)
        if with_fields:
            rec.update(_fields(b))
        out.append(rec)
    if log:
        out.append({k: v for k, v in b.log_read().items() if k != "capacity"})
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.keys() == w.keys()
        for name in w:
            np.testing.assert_array_equal(g[name], w[name], err_msg=f"{what}: {name}, step {k}")


def _crosses_episode_end_and_degradation_row(recs, tb):
    done = np.array([r["done"] for r in recs]).astype(bool)
    rows = np.array([r["f_time_idx"] for r in recs])
    at_deg = (np.asarray(tb.hour) == 14) & (np.asarray(tb.minute) == 45)
    # (a step that does not end an episode leaves row time_idx - 1 for row time_idx: both were passed)
    return bool(done.any()), bool(at_deg[rows].any() or at_deg[np.maximum(rows - 1, 0)][~done].any())


# ---- 1. rewind ---------------------------------------------------------------------------------------------------------------
REWIND = [
    dict(uc="ct", n=5, E=33, deg="rainflow"), dict(uc="ct", n=50, E=40, deg="rainflow"), dict(uc="lmd", n=64, E=9, deg="rainflow"),
    dict(uc="lmd", n=65, E=7, deg="rainflow"), dict(uc="ut", n=200, E=5, deg="rainflow"), dict(uc="ut", n=257, E=3, deg="rainflow"),
    dict(uc="ct", n=5, E=33, deg="linear"), dict(uc="ct", n=50, E=17, deg="none"),
    dict(uc="ct", n=5, E=21, deg="rainflow", real_time=True),
    dict(uc="ct", n=5, E=13, deg="rainflow", log=True),
    dict(uc="ct", n=5, E=13, deg="rainflow", schedule=True),
    dict(uc="ct", n=5, E=13, deg="rainflow", count_all=True),
]


@pytest.mark.parametrize("case", REWIND, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_rewind_replays_bit_for_bit(case):
    c = dict(case)
    log, rt = c.pop("log", False), c.pop("real_time", False)
    sched, count_all = c.pop("schedule", False), c.pop("count_all", False)
    E, N = c["E"], c["n"]
    p, tb, tf = _make(c["uc"], N, E, c["deg"], real_time=rt, log=log)
    b = _batch((p, tb, tf))
    rng = np.random.default_rng(5)
    if sched:
        b.set_start_schedule(rng.integers(0, tb.T - 3 * EP, size=(3, E)).astype(np.int32))
    if count_all:
        b.set_rainflow_count_all(True)
    b.reset()
    K = 200  # two whole episodes and more: every env passes an episode end and a 14:45 row
    tape = _tape(rng, 40 + K, E, N)
    _run(b, tape[:40], with_fields=False)
    blob = b.save_state()
    first = _run(b, tape[40:], log=log)
    if sched:   # what a load must put back: the schedule is gone, the switch is off
        b.set_start_schedule(None)
    if count_all:
        b.set_rainflow_count_all(False)
    b.load_state(blob)
    second = _run(b, tape[40:], log=log)
    _assert_same(second, first, "second pass after load")
    recs = first[:-1] if log else first
    ends, deg_row = _crosses_episode_end_and_degradation_row(recs, tb)
    assert ends and deg_row, f"the K rows must span an episode end ({ends}) and a 14:45 row ({deg_row})"
    if sched:
        assert (first[-1]["f_episodes"] >= 1).all()
    b.check_errors()
    b.close()


def test_rewind_with_the_night_policy_window_open():
    """The night policy keeps a per-env "charging since" row (cold.night_start) that survives resets: saved while it is open."""
    import torch

    E, N = 19, 5
    p, tb, tf = _make("ct", N, E, "rainflow")
    b = _batch((p, tb, tf))
    dev = torch.device("cuda", 0)
    obs = torch.zeros((E, b.obs_dim), device=dev)
    rs = torch.zeros(E, device=dev, dtype=torch.float64)
    dc = torch.zeros(E, device=dev, dtype=torch.int32)
    b.set_start_schedule(np.full((1, E), int(np.flatnonzero((np.asarray(tb.hour) == 18) & (np.asarray(tb.minute) == 0))[3]), np.int32))
    b.set_night_policy(20, 0, 6)
    b.reset_dev(obs.data_ptr())
    b.rollout_policy_dev(_capi.POLICY_NIGHT, 12, obs.data_ptr(), rs.data_ptr(), dc.data_ptr())  # 18:00 -> 21:00: the window is open
    b.synchronize()
    blob = torch.empty(b.state_bytes(), dtype=torch.uint8, device=dev)
    b.save_state(blob)
    b.synchronize()
    night = _capi.state_views(blob.cpu().numpy())["night_start"]
    assert (night != np.iinfo(np.int32).min).all(), "the charging window must be open when the state is saved"

    def go():
        out = []
        for _ in range(14):  # 8 rows each: through the window's end, an episode end and a 14:45 row
            b.rollout_policy_dev(_capi.POLICY_NIGHT, 8, obs.data_ptr(), rs.data_ptr(), dc.data_ptr())
            b.synchronize()
            out.append({"obs": obs.cpu().numpy(), "reward_sum": rs.cpu().numpy(), "done_count": dc.cpu().numpy(), **_fields(b)})
        return out

    first = go()
    b.set_night_policy(3, 15, 1)  # other parameters, window state cleared: the load restores both
    b.load_state(blob)
    second = go()
    _assert_same(second, first, "night policy after load")
    assert sum(int(r["done_count"].sum()) for r in first) >= E
    b.close()


def test_rewind_second_pass_through_the_direct_queue():
    import torch

    E, N, K = 256, 50, 150
    p, tb, tf = _make("ct", N, E, "rainflow")
    b = _batch((p, tb, tf))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2)
    tape = torch.from_numpy(_tape(rng, 31, E, N)).to(dev)
    obs = torch.zeros((E, b.obs_dim), device=dev)
    rew = torch.zeros(E, device=dev, dtype=torch.float64)
    done = torch.zeros(E, device=dev, dtype=torch.uint8)
    ptrs = (obs.data_ptr(), rew.data_ptr(), done.data_ptr())
    b.reset_dev(obs.data_ptr())
    b.run_tape_dev(45, tape.data_ptr(), 31, *ptrs, use_graph=_capi.LAUNCH_EAGER)
    blob = torch.empty(b.state_bytes(), dtype=torch.uint8, device=dev)
    b.save_state(blob)

    def go(mode):
        b.run_tape_dev(K, tape.data_ptr(), 31, *ptrs, use_graph=mode)
        b.synchronize()
        return [{"obs": obs.cpu().numpy(), "reward": rew.cpu().numpy(), "done": done.cpu().numpy(), **_fields(b)}]

    first = go(_capi.LAUNCH_EAGER)
    b.load_state(blob)
    second = go(_capi.LAUNCH_DIRECT)
    _assert_same(second, first, "direct run after load")
    assert (first[0]["f_episodes"] >= 1).all()
    # ... and a save taken right behind a direct run (the entry drains it first) equals one taken behind the stream's launches
    blob2 = torch.empty_like(blob)
    b.save_state(blob2)
    b.load_state(blob)
    go(_capi.LAUNCH_EAGER)
    blob3 = torch.empty_like(blob)
    b.save_state(blob3)
    b.synchronize()
    assert torch.equal(blob2, blob3)
    b.close()


# ---- 2. resume elsewhere, 3. two saves of one state ---------------------------------------------------------------------------
def _vs_oracle(rec, o):
    oo, ro, do, to = o
    np.testing.assert_array_equal(rec["done"], do)
    np.testing.assert_allclose(rec["obs"], oo, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rec["reward"], ro, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(rec["term"][do.astype(bool)], to[do.astype(bool)], rtol=1e-5, atol=1e-6)


def _fields_vs_oracle(b, cpu, rainflow, sel=slice(None), osel=slice(None)):
    np.testing.assert_array_equal(b.get("time_idx")[sel], cpu.get("time_idx")[osel])
    np.testing.assert_array_equal(b.get("hours_left")[sel], cpu.get("hours_left")[osel])
    np.testing.assert_allclose(b.get("soc")[sel], cpu.get("soc")[osel], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(b.get("soh")[sel], cpu.get("soh")[osel], rtol=1e-9)
    np.testing.assert_allclose(b.get("ep_return")[sel], cpu.get("ep_return")[osel], rtol=1e-9, atol=1e-8)
    if rainflow:
        np.testing.assert_array_equal(b.get("rf_len")[sel], cpu.get("rf_len")[osel])
        np.testing.assert_allclose(b.get("fd_cyc")[sel], cpu.get("fd_cyc")[osel], rtol=1e-8, atol=1e-18)
        np.testing.assert_allclose(b.get("sei_l")[sel], cpu.get("sei_l")[osel], rtol=1e-9, atol=1e-18)


@pytest.mark.parametrize("uc,n,E,deg,steps,cut", [("ct", 50, 4096, "rainflow", 2 * EP + 8, 77), ("lmd", 5, 37, "rainflow", 150, 60),
                                                  ("ut", 64, 6, "linear", 150, 101), ("lmd", 100, 5, "rainflow", 150, 50),
                                                  ("ut", 200, 3, "rainflow", 150, 97), ("ct", 300, 2, "rainflow", 150, 33)])
def test_resume_in_a_fresh_handle_equals_the_uninterrupted_run_and_the_oracle(uc, n, E, deg, steps, cut):
    from oracle.fleet_oracle import OracleBatch

    args = _make(uc, n, E, deg)
    whole, cpu = _batch(args), OracleBatch(*args, threads=16)
    rng = np.random.default_rng(8)
    tape = _tape(rng, steps, E, n)
    every = 1 if E < 100 else 24
    np.testing.assert_array_equal(whole.reset(), cpu.reset())
    part = _batch(args)
    part.reset()
    for a in tape[:cut]:
        part.step(a)
    blob = part.save_state()
    again = part.save_state()
    assert blob.tobytes() == again.tobytes(), "two saves of one state"
    # the device-free check on a blob a handle really wrote: accepted for its own parameters and tables, refused for others
    th = _capi.state_table_hash(args[0], args[1], args[2])
    _capi.state_check(args[0], th, blob)
    _refused(lambda: _capi.state_check(args[0], th, blob[:4096]), _capi.ERR_INVALID, "shorter")
    _refused(lambda: _capi.state_check(args[0], th ^ 1, blob), _capi.ERR_INVALID, "table_hash")
    _refused(lambda: _capi.state_check(_make(uc, n, E + 1, deg)[0], th, blob), _capi.ERR_INVALID, "num_envs")
    _refused(lambda: _capi.state_check(_make(uc, n, E, "none")[0], th, blob), _capi.ERR_INVALID, "deg_mode")
    part.close()
    fresh = _batch(args)  # never reset, never stepped
    fresh.load_state(blob)
    assert fresh.save_state().tobytes() == blob.tobytes(), "save, load, save"
    ends = 0
    for k, a in enumerate(tape):
        rec = _run(whole, [a], with_fields=False)[0]
        _vs_oracle(rec, cpu.step(a))
        ends += int(rec["done"].sum())
        if k >= cut:
            got = _run(fresh, [a], with_fields=False)[0]
            _assert_same([got], [rec], f"resumed handle, step {k}")
            if k % every == 0 or k == steps - 1:
                _assert_same([_fields(fresh)], [_fields(whole)], f"resumed handle's fields, step {k}")
                _fields_vs_oracle(fresh, cpu, deg == "rainflow")
    assert ends >= E * (2 if E == 4096 else 1)
    fresh.check_errors()
    for x in (whole, fresh, cpu):
        x.close()


# ---- 4. / 5. fork ---------------------------------------------------------------------------------------------------------------
def fork_scenario(kind):
    """-> dict(Es, Ed, src_idx, dst_idx, same): which envs are copied where."""
    if kind == "within-broadcast":       # one source to a set, inside one handle
        return dict(Es=12, Ed=12, same=True, src_idx=[3] * 5, dst_idx=[0, 4, 7, 10, 11])
    if kind == "within-many":            # many to many with repeated sources, inside one handle
        return dict(Es=12, Ed=12, same=True, src_idx=[1, 1, 5, 8, 5], dst_idx=[2, 3, 9, 6, 11])
    if kind == "across-equal":           # two handles of equal E, many to many with repeats
        return dict(Es=10, Ed=10, same=False, src_idx=[0, 7, 7, 4, 9, 0], dst_idx=[5, 1, 8, 3, 0, 9])
    if kind == "across-one-to-many":     # a 1-env handle seeds a batch
        return dict(Es=1, Ed=9, same=False, src_idx=[0] * 6, dst_idx=[8, 1, 2, 5, 6, 3])
    raise KeyError(kind)


FORK_AT, FORK_TOTAL, FORK_N = 70, 140, 7


def _deep_stack_tape(rng, E, tb, starts0, shift=0):
    """Up to the fork: five of an env's seven EVs swing with alternating sign and an amplitude that shrinks by a fifth per plugged-in
    row, from 0.9 at every arrival (every range smaller than the one before, also across the charge / discharge asymmetry: no cycle
    closes, the rainflow stack grows by one entry per row), the other two -- which two depends on the env -- idle, so that their
    stacks stay flat.  Two envs with different idle EVs therefore have a deeper stack each somewhere.  After the fork: random
    actions."""
    tape = _tape(rng, FORK_TOTAL, E, FORK_N)
    there = np.asarray(tb.there)
    for e in range(E):
        idle = {(e + shift) % FORK_N, (e + shift + 1) % FORK_N}
        for n in range(FORK_N):
            j = 0
            for k in range(FORK_AT):
                plugged = bool(there[starts0[e] + k, n])
                j = j + 1 if plugged else 0
                tape[k, e, n] = 0.0 if (n in idle or not plugged) else 0.9 * 0.8 ** (j - 1) * (1.0 if j % 2 else -1.0)
    return tape


def fork_inputs(kind):
    """Start rows and tapes of a fork test.  tests/test_state_cpu.py runs the CPU oracle on the same inputs and checks the
    conditions of fork_preconditions that it can (stack sizes from a rainflow residue count of the oracle's SOC series)."""
    sc = fork_scenario(kind)
    rng = np.random.default_rng(31 + len(kind))
    tb = _tables("ct", FORK_N)
    early = np.flatnonzero((np.asarray(tb.hour) < 9) & (np.arange(tb.T) < tb.T - 4 * EP))  # the 14:45 row comes within 60 rows
    sc["starts_s"] = rng.choice(early, size=(3, sc["Es"]), replace=False).astype(np.int32)
    sc["starts_d"] = sc["starts_s"] if sc["same"] else rng.choice(early, size=(3, sc["Ed"]), replace=False).astype(np.int32)
    sc["tape_s"] = _deep_stack_tape(rng, sc["Es"], tb, sc["starts_s"][0])
    sc["tape_d"] = sc["tape_s"] if sc["same"] else _deep_stack_tape(rng, sc["Ed"], tb, sc["starts_d"][0], shift=3)
    sc["tb"] = tb
    return sc


def fork_preconditions(sc, fs, fd):
    """Test 5: the fork must have something to do.  `fs` / `fd`: fields of the source / destination handle read BEFORE the fork."""
    tb, src, dst = sc["tb"], np.array(sc["src_idx"]), np.array(sc["dst_idx"])
    deg = (np.asarray(tb.hour) == 14) & (np.asarray(tb.minute) == 45)
    for e in np.unique(src):
        assert deg[fs["f_start_idx"][e]:fs["f_time_idx"][e]].any(), "the fork point lies after the episode's first degradation row"
    stack_s, stack_d = fs["f_rf_stack"][src], fd["f_rf_stack"][dst]
    assert ((stack_s >= 3) & (fs["f_rf_len"][src] > 0)).mean() >= 0.5, "at least half of the forked EVs have a stack of >= 3 entries"
    for i, (s, d) in enumerate(zip(src, dst)):
        assert not np.array_equal(fs["f_soc"][s], fd["f_soc"][d]), f"pair {i}: SOC"
        assert fs["f_time_idx"][s] != fd["f_time_idx"][d], f"pair {i}: time row"
        assert not np.array_equal(fs["f_rf_stack"][s], fd["f_rf_stack"][d]), f"pair {i}: rainflow stack"
    assert (stack_d > stack_s).any(), "a destination stack deeper than its source's: stale words stay behind"
    assert (stack_d < stack_s).any(), "a destination stack shallower than its source's"


def _live_part_only(rows_s, rows_d, rows_after, stack_s, src_idx, dst_idx):
    """The rainflow rows after a fork, word for word (as bit patterns: never-written words may hold anything): of a destination
    row the 6 header words and the source's stack words below its top entry (stack size - 1 of them; the top is in the header) are
    the source's; the kernel moves 16-byte pieces, so one more word may be either's; every word beyond is what the destination held
    before.  Rows of envs that are no destination are untouched."""
    u = lambda a: np.ascontiguousarray(a).view(np.uint64)  # noqa: E731
    rows_s, rows_d, rows_after = u(rows_s), u(rows_d), u(rows_after)
    others = np.setdiff1d(np.arange(rows_d.shape[0]), dst_idx)
    np.testing.assert_array_equal(rows_after[others], rows_d[others], err_msg="rainflow rows of bystanders")
    kept = 0
    for s, d in zip(src_idx, dst_idx):
        for c in range(rows_d.shape[1]):
            words = max(int(stack_s[s, c]) - 1, 0)
            live, piece_end = 6 + words, 6 + (words + 1) // 2 * 2
            np.testing.assert_array_equal(rows_after[d, c, :live], rows_s[s, c, :live], err_msg=f"live words, env {s} -> {d}, EV {c}")
            np.testing.assert_array_equal(rows_after[d, c, piece_end:], rows_d[d, c, piece_end:],
                                          err_msg=f"words beyond the live part, env {s} -> {d}, EV {c}")
            kept += int((rows_d[d, c, piece_end:] != rows_s[s, c, piece_end:]).sum())
    assert kept > 0, "source and destination rows must differ beyond the live part, else 'stays as it was' shows nothing"


@pytest.mark.parametrize("kind", ["within-broadcast", "within-many", "across-equal", "across-one-to-many"])
def test_fork_copies_envs_and_nothing_else(kind):
    from oracle.fleet_oracle import OracleBatch

    sc = fork_inputs(kind)
    Es, Ed, N, same = sc["Es"], sc["Ed"], FORK_N, sc["same"]
    src_idx, dst_idx = np.array(sc["src_idx"]), np.array(sc["dst_idx"])
    args_s, args_d = _make("ct", N, Es, "rainflow", seed=3), _make("ct", N, Ed, "rainflow", seed=3)
    hs = _batch(args_s)
    hd = hs if same else _batch(args_d)
    ctl = _batch(args_d)                      # the destination handle's twin: same tape, no fork
    cpu_s = OracleBatch(*args_s)              # the source handle, straight through
    # per pair: the source's history, then the DESTINATION's start row at the next reset -- what the forked env must be
    args_p = _make("ct", N, len(dst_idx), "rainflow", seed=3)
    cpu_p = OracleBatch(*args_p)
    starts_p = sc["starts_s"][:, src_idx].copy()
    starts_p[1:] = sc["starts_d"][1:, dst_idx]
    for x, st in ((hs, sc["starts_s"]), (hd, sc["starts_d"]), (ctl, sc["starts_d"]), (cpu_s, sc["starts_s"]), (cpu_p, starts_p)):
        x.set_start_schedule(st)
        if x in (hs, hd, ctl):
            # count to the episode's end (a switch of the handle; outputs and SoH do not depend on it): by default the count stops at
            # the 14:45 row, before the evening's swings, and the stacks would be two or three entries deep at the fork
            x.set_rainflow_count_all(True)
        x.reset()
    for k in range(FORK_AT):
        rs = _run(hs, [sc["tape_s"][k]], with_fields=False)[0]
        _vs_oracle(rs, cpu_s.step(sc["tape_s"][k]))
        cpu_p.step(sc["tape_s"][k][src_idx])
        if not same:
            hd.step(sc["tape_d"][k])
        ctl.step(sc["tape_d"][k])
    fs, fd = _fields(hs), _fields(hd)
    fork_preconditions(sc, fs, fd)
    rows_s, rows_d = hs.state_dict()["rf_rows"].copy(), hd.state_dict()["rf_rows"].copy()
    hd.fork_envs(src_idx, dst_idx, source=None if same else hs)
    others = np.setdiff1d(np.arange(Ed), dst_idx)
    _live_part_only(rows_s, rows_d, hd.state_dict()["rf_rows"], fs["f_rf_stack"], src_idx, dst_idx)
    _assert_same([{k: v[others] for k, v in _fields(hd).items()}], [{k: v[others] for k, v in fd.items()}], "envs outside dst_idx")
    _assert_same([{k: v[dst_idx] for k, v in _fields(hd).items()}], [{k: v[src_idx] for k, v in fs.items()}], "forked envs")
    running = True  # the sources' episode (all envs of these handles end theirs on the same step)
    for k in range(FORK_AT, FORK_TOTAL):
        a_s = sc["tape_s"][k]
        a_d = sc["tape_d"][k].copy()
        a_c = a_d.copy()
        a_d[dst_idx] = a_s[src_idx] if running else sc["tape_d"][k][dst_idx]
        if same:
            rs = rd = _run(hd, [a_d])[0]
        else:
            rs, rd = _run(hs, [a_s])[0], _run(hd, [a_d])[0]
        rc = _run(ctl, [a_c])[0]
        o_s = cpu_s.step(a_d if same else a_s)
        o_p = cpu_p.step(a_d[dst_idx])
        done_now = bool(rs["done"][src_idx].any())
        if running:  # (a) the destination is its source, outputs and fields, through the step that ends the episode
            assert (rs["done"][src_idx] == rs["done"][src_idx][0]).all()
            for name in ("reward", "done", "term") + (() if done_now else ("obs",) + FKEYS):
                np.testing.assert_array_equal(rd[name][dst_idx], rs[name][src_idx], err_msg=f"fork pair: {name}, step {k}")
        # (b) everything else never noticed
        for name in ("obs", "reward", "done", "term") + FKEYS:
            np.testing.assert_array_equal(rd[name][others], rc[name][others], err_msg=f"bystanders: {name}, step {k}")
        # (c) the destination against the oracle env that lived the source's history and then took the destination's start row
        _vs_oracle({name: rd[name][dst_idx] for name in ("obs", "reward", "done", "term")}, o_p)
        _fields_vs_oracle(hd, cpu_p, True, sel=dst_idx)
        # (d) the source handle against its oracle (within one handle: its envs that are not destinations)
        keep = others if same else np.arange(Es)
        _vs_oracle({name: rs[name][keep] for name in ("obs", "reward", "done", "term")}, tuple(x[keep] for x in o_s))
        _fields_vs_oracle(hs, cpu_s, True, sel=keep, osel=keep)
        if done_now:
            running = False
            np.testing.assert_array_equal(hd.get("start_idx")[dst_idx], sc["starts_d"][1, dst_idx],
                                          err_msg="after its reset the destination starts on its OWN column of the schedule")
    assert not running, "the test must run past the end of the forked episode"
    for x in {hs, hd, ctl}:
        x.check_errors()
        x.close()


def test_fork_from_a_single_env_without_auto_reset_seeds_an_auto_resetting_batch():
    """auto_reset is not part of the fingerprint: a 1-env handle with gymnasium semantics (no auto-reset: its count never stops,
    FLEET_F_RF_UNTIL = INT32_MAX) seeds envs of a vec-env batch.  They continue its episode bit for bit, end it on the same step,
    and then -- unlike their source, which stays done -- reset themselves onto their own start rows and match the oracle."""
    from oracle.fleet_oracle import OracleBatch

    sc = fork_inputs("across-one-to-many")
    Ed, N = sc["Ed"], FORK_N
    src_idx, dst_idx = np.array(sc["src_idx"]), np.array(sc["dst_idx"])
    others = np.setdiff1d(np.arange(Ed), dst_idx)
    args_d = _make("ct", N, Ed, "rainflow", seed=3)
    hs = _batch(_make("ct", N, 1, "rainflow", seed=3, auto_reset=False))
    hd, ctl = _batch(args_d), _batch(args_d)
    cpu_p = OracleBatch(*_make("ct", N, len(dst_idx), "rainflow", seed=3))  # auto-resetting, as the destinations are
    starts_p = sc["starts_s"][:, src_idx].copy()
    starts_p[1:] = sc["starts_d"][1:, dst_idx]
    for x, st in ((hs, sc["starts_s"]), (hd, sc["starts_d"]), (ctl, sc["starts_d"]), (cpu_p, starts_p)):
        x.set_start_schedule(st)
        if x in (hd, ctl):
            x.set_rainflow_count_all(True)
        x.reset()
    for k in range(FORK_AT):
        hs.step(sc["tape_s"][k])
        cpu_p.step(sc["tape_s"][k][src_idx])
        hd.step(sc["tape_d"][k])
        ctl.step(sc["tape_d"][k])
    fs, fd = _fields(hs), _fields(hd)
    assert fs["f_rf_until"][0] == np.iinfo(np.int32).max and not fs["f_done"][0]
    fork_preconditions(sc, fs, fd)
    hd.fork_envs(src_idx, dst_idx, source=hs)
    running = True
    for k in range(FORK_AT, FORK_TOTAL):
        a_d = sc["tape_d"][k].copy()
        a_c = a_d.copy()
        if running:
            a_d[dst_idx] = sc["tape_s"][k][src_idx]
            rs = _run(hs, [sc["tape_s"][k]])[0]
        rd, rc = _run(hd, [a_d])[0], _run(ctl, [a_c])[0]
        o_p = cpu_p.step(a_d[dst_idx])
        if running:
            done_now = bool(rs["done"][0])
            np.testing.assert_array_equal(rd["reward"][dst_idx], rs["reward"][src_idx], err_msg=f"reward, step {k}")
            np.testing.assert_array_equal(rd["done"][dst_idx], rs["done"][src_idx], err_msg=f"done, step {k}")
            if done_now:  # without auto-reset the observation of the step that ends the episode IS the terminal observation
                np.testing.assert_array_equal(rd["term"][dst_idx], rs["obs"][src_idx], err_msg="terminal observation")
                assert rs["f_done"][0] == 1 and not rd["f_done"][dst_idx].any(), "the source stays done, the destinations have reset"
                np.testing.assert_array_equal(rd["f_start_idx"][dst_idx], sc["starts_d"][1, dst_idx])
                running = False
            else:
                for name in ("obs",) + FKEYS:
                    np.testing.assert_array_equal(rd[name][dst_idx], rs[name][src_idx], err_msg=f"fork pair: {name}, step {k}")
        for name in ("obs", "reward", "done", "term") + FKEYS:
            np.testing.assert_array_equal(rd[name][others], rc[name][others], err_msg=f"bystanders: {name}, step {k}")
        _vs_oracle({name: rd[name][dst_idx] for name in ("obs", "reward", "done", "term")}, o_p)
        _fields_vs_oracle(hd, cpu_p, True, sel=dst_idx)
    assert not running
    for x in (hs, hd, ctl):
        x.check_errors()
        x.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def _refused(fn, status, match):
    with pytest.raises(_capi.FleetHipError, match=match) as ei:
        fn()
    assert ei.value.status == status


def test_refusals_leave_the_state_untouched():
    import torch

    args = _make("ct", 5, 8, "rainflow")
    a, b = _batch(args), _batch(args)
    rng = np.random.default_rng(0)
    for x in (a, b):
        x.reset()
        _run(x, _tape(rng, 30, 8, 5), with_fields=False)
    before = (a.save_state(), b.save_state())
    _refused(lambda: a.fork_envs([0, 1], [2, 2]), _capi.ERR_INVALID, "twice")
    _refused(lambda: a.fork_envs([0, 1], [3, 0]), _capi.ERR_INVALID, "both a source and a destination")
    _refused(lambda: a.fork_envs([0], [8]), _capi.ERR_INVALID, "out of range")
    _refused(lambda: a.fork_envs([-1], [1]), _capi.ERR_INVALID, "out of range")
    _refused(lambda: a.fork_envs([8], [1], source=b), _capi.ERR_INVALID, "out of range")
    other = _batch(_make("ct", 5, 8, "rainflow", seed=99))       # another picker seed
    tables2 = _batch(_make("ut", 5, 8, "rainflow"))               # other tables
    linear = _batch(_make("ct", 5, 8, "linear"))
    _refused(lambda: a.fork_envs([0], [1], source=other), _capi.ERR_INVALID, "seed")
    _refused(lambda: a.fork_envs([0], [1], source=tables2), _capi.ERR_INVALID, "table_hash")
    _refused(lambda: a.fork_envs([0], [1], source=linear), _capi.ERR_INVALID, "deg_mode")
    logged = _batch(_make("ct", 5, 8, "rainflow", log=True))
    logged.reset()
    _refused(lambda: logged.fork_envs([0], [1]), _capi.ERR_UNSUPPORTED, "data log")
    _refused(lambda: a.fork_envs([0], [1], source=logged), _capi.ERR_UNSUPPORTED, "data log")
    if torch.cuda.device_count() > 1:
        far = _batch((*args, 1))
        _refused(lambda: a.fork_envs([0], [1], source=far), _capi.ERR_INVALID, "different devices")
        far.close()
    # loads: wrong E, other tables, a truncated blob, a foreign blob
    wide = _batch(_make("ct", 5, 9, "rainflow"))
    wide.reset()
    _refused(lambda: a.load_state(wide.save_state()), _capi.ERR_INVALID, "num_envs")
    tables2.reset()
    _refused(lambda: a.load_state(tables2.save_state()), _capi.ERR_INVALID, "table_hash")
    _refused(lambda: a.load_state(before[0][:-1]), _capi.ERR_INVALID, "shorter")
    junk = before[0].copy()
    junk[0] ^= 0xFF
    _refused(lambda: a.load_state(junk), _capi.ERR_INVALID, "magic")
    _refused(lambda: a.save_state(np.empty(100, np.uint8)), _capi.ERR_INVALID, "needs")
    # a handle with a device error raised (an episode that leaves the table: tests/test_capi_gpu.py) is neither saved nor forked
    bad = _batch(args)
    bad.set_start_schedule(np.full((1, 8), args[1].T - 3, dtype=np.int32))
    bad.reset()
    z = np.zeros((8, 5), np.float32)
    bad.step(z)
    bad.step(z)
    with pytest.raises(IndexError):
        bad.step(z)
    _refused(bad.save_state, _capi.ERR_STATE, "error bits")
    _refused(lambda: a.fork_envs([0], [1], source=bad), _capi.ERR_STATE, "error bits")
    _refused(lambda: bad.fork_envs([0], [1], source=a), _capi.ERR_STATE, "error bits")
    assert a.save_state().tobytes() == before[0].tobytes() and b.save_state().tobytes() == before[1].tobytes()
    a.fork_envs([], [])  # nothing to do is not an error
    assert a.save_state().tobytes() == before[0].tobytes()
    for x in (a, b, other, tables2, linear, logged, wide, bad):
        x.close()


# ---- 7. Python surface ----------------------------------------------------------------------------------------------------------
def _env_cfg(deg="rainflow"):
    return _cfg("ct", deg, False)


def test_deepcopy_of_a_fleet_env_continues_identically_and_independently():
    from fleetrl_amd import FleetEnv

    tb = _tables("ct", 5)
    env = FleetEnv(_env_cfg(), tables=tb, seed=4)
    env.reset()
    rng = np.random.default_rng(1)
    acts = rng.uniform(-1, 1, size=(100, 5)).astype(np.float32)
    for a in acts[:50]:
        env.step(a)
    twin = copy.deepcopy(env)
    assert twin.core.batch.h.value != env.core.batch.h.value
    t0 = env.get_time()
    twin.step(acts[50])                      # stepping the copy does not move the original
    assert env.get_time() == t0 and twin.get_time() != t0
    o1 = [env.step(a) for a in acts[50:]]
    o2 = [twin.step(a) for a in acts[51:]]
    third = copy.deepcopy(env)               # (a copy at the end state, compared below)
    for (oa, ra, da, _, _), (ob, rb, db, _, _) in zip(o1[1:], o2):
        np.testing.assert_array_equal(oa, ob)
        assert ra == rb and da == db
    assert any(d for _, _, d, _, _ in o1), "the run must reach the episode's end"
    for f in FIELDS:
        np.testing.assert_array_equal(twin.core.batch.get(f), env.core.batch.get(f), err_msg=f)
        np.testing.assert_array_equal(third.core.batch.get(f), env.core.batch.get(f), err_msg=f)
    for e in (env, twin, third):
        e.close()


def test_deepcopy_of_a_vec_env_steps_on_torch_streams_like_the_original():
    """The original has adopted torch's stream through step_torch; its copy is a new handle and must adopt it too (the cache of
    the adopted stream does not travel), so that its launches are ordered with the torch ops around them."""
    import torch
    from fleetrl_amd import FleetVecEnv

    tb = _tables("ct", 5)
    E = 64
    dev = torch.device("cuda", 0)
    env = FleetVecEnv(_env_cfg(), E, tables=tb, seed=4)
    env.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    acts = torch.rand((150, E, 5), device=dev, generator=gen) * 2 - 1
    for k in range(40):
        env.step_torch(acts[k])
    assert env._torch_stream == torch.cuda.current_stream(dev).cuda_stream
    twin = copy.deepcopy(env)
    assert not hasattr(twin, "_torch_stream") and twin.core.batch.h.value != env.core.batch.h.value
    assert twin.core.batch.stream_ptr() != env.core.batch.stream_ptr(), "a new handle launches on its own stream until told"
    ends = 0
    for k in range(40, 150):
        a = acts[k] * 1.0  # produced on torch's stream right before the launch: an unordered launch would race with it
        o1, r1, d1 = env.step_torch(a)
        o2, r2, d2 = twin.step_torch(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), f"step {k}"
        ends += int(d1.sum())
    assert twin.core.batch.stream_ptr() == env.core.batch.stream_ptr() == torch.cuda.current_stream(dev).cuda_stream
    assert ends >= E
    for f in FIELDS:
        np.testing.assert_array_equal(twin.core.batch.get(f), env.core.batch.get(f), err_msg=f)
    env.close()
    twin.close()


def test_vec_env_state_through_a_file(tmp_path):
    from fleetrl_amd import FleetVecEnv

    tb = _tables("ct", 5)
    E = 6
    rng = np.random.default_rng(2)
    acts = rng.uniform(-1, 1, size=(160, E, 5)).astype(np.float32)
    env = FleetVecEnv(_env_cfg(), E, tables=tb, seed=4)
    env.reset()
    for a in acts[:45]:
        env.step(a)
    env.env_method("set_start_time", "2020-03-01 12:00:00", indices=[2])
    path = tmp_path / "env_state.npz"
    env.save_state(path)
    want = [env.step(a) for a in acts[45:]]
    fresh = FleetVecEnv(_env_cfg(), E, tables=tb, seed=4)
    fresh.load_state(path)
    assert fresh.env_method("get_start_time")[2] == "2020-03-01 12:00:00", "an override given as a str comes back as that str"
    got = [fresh.step(a) for a in acts[45:]]
    # the saved env dropped the override when env 2's episode ended; the resumed one must have done the same
    assert env.env_method("get_start_time") == fresh.env_method("get_start_time")
    assert fresh.env_method("get_start_time")[2] != "2020-03-01 12:00:00"
    n_done = 0
    for (oa, ra, da, ia), (ob, rb, db, ib) in zip(want, got):
        np.testing.assert_array_equal(oa, ob)
        np.testing.assert_array_equal(ra, rb)
        np.testing.assert_array_equal(da, db)
        for x, y in zip(ia, ib):
            assert x.keys() == y.keys()
            if x:
                np.testing.assert_array_equal(x["terminal_observation"], y["terminal_observation"])
                assert x["episode"] == y["episode"]
                n_done += 1
    assert n_done >= E
    # a file that carries a pickled object is refused
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["state_soh"] = np.array([object()], dtype=object)
    bad = tmp_path / "bad.npz"
    np.savez(bad, **d)
    with pytest.raises(ValueError):
        fresh.load_state(bad)
    # fork through the env class: env 0's state in every other env, its start-time override with it -- until the episode ends
    fresh.env_method("set_start_time", "2021-01-01 00:00:00", indices=[0])
    fresh.fork_envs(0, list(range(1, E)))
    soc = fresh.core.batch.get("soc")
    assert (soc == soc[0]).all()
    assert fresh.env_method("get_start_time") == ["2021-01-01 00:00:00"] * E
    for a in acts[:EP]:
        _, _, dones, _ = fresh.step(a)
        if dones.all():
            break
    assert dones.all() and "2021-01-01 00:00:00" not in fresh.env_method("get_start_time")
    env.close()
    fresh.close()


def test_mixed_vec_env_keeps_one_state_per_group(tmp_path):
    from fleetrl_amd.mixed import FleetMixedVecEnv

    groups = [(_cfg("ct", "rainflow", False), 4, {"tables": _tables("ct", 5), "seed": 1}),
              (_cfg("ut", "rainflow", False), 3, {"tables": _tables("ut", 5), "seed": 1})]
    rng = np.random.default_rng(3)
    acts = rng.uniform(-1, 1, size=(150, 7, 5)).astype(np.float32)
    env = FleetMixedVecEnv(groups)
    env.reset()
    for a in acts[:40]:
        env.step(a)
    path = tmp_path / "mixed.npz"
    env.save_state(path)
    want = [env.step(a) for a in acts[40:]]
    fresh = FleetMixedVecEnv(groups)
    fresh.load_state(path)
    got = [fresh.step(a) for a in acts[40:]]
    for (oa, ra, da, _), (ob, rb, db, _) in zip(want, got):
        np.testing.assert_array_equal(oa, ob)
        np.testing.assert_array_equal(ra, rb)
        np.testing.assert_array_equal(da, db)
    assert sum(int(d.sum()) for _, _, d, _ in want) >= 7
    one = FleetMixedVecEnv(groups[:1])
    with pytest.raises(_capi.FleetHipError):
        one.load_state(path)
    for e in (env, fresh, one):
        e.close()


def test_vec_normalize_and_env_saved_and_loaded_together(tmp_path):
    from fleetrl_amd import FleetVecEnv, FleetVecNormalize

    tb = _tables("ct", 5)
    E = 6
    rng = np.random.default_rng(4)
    acts = rng.uniform(-1, 1, size=(140, E, 5)).astype(np.float32)
    vn = FleetVecNormalize(FleetVecEnv(_env_cfg(), E, tables=tb, seed=2))
    vn.reset()
    for a in acts[:96]:   # through an episode end: the discounted returns are zero again on the step the pair is saved
        _, _, dones, _ = vn.step(a)
    assert dones.all()
    vn.save(tmp_path / "norm.npz")
    vn.venv.save_state(tmp_path / "env.npz")
    want = [vn.step(a) for a in acts[96:]]
    venv = FleetVecEnv(_env_cfg(), E, tables=tb, seed=2)
    venv.load_state(tmp_path / "env.npz")
    vn2 = FleetVecNormalize.load(tmp_path / "norm.npz", venv)
    got = [vn2.step(a) for a in acts[96:]]
    for (oa, ra, da, _), (ob, rb, db, _) in zip(want, got):
        np.testing.assert_array_equal(oa, ob)
        np.testing.assert_array_equal(ra, rb)
        np.testing.assert_array_equal(da, db)
    vn.close()
    vn2.close()
