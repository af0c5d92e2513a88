"""The replay buffer on the device (fleet_replay.hip) against the NumPy model of tests/replay_model.py, bit for bit.  Needs an
MI355X."""
import os
import sys

import numpy as np
import pytest

import replay_model as rp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POISON = np.array([0x7FC0DEAD], np.uint32).view(np.float32)[0]  # a NaN with a payload: any read of it shows in a bit comparison


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poisoned(shape):
    return torch.from_numpy(np.full(shape, POISON, np.float32)).to(DEV)


def source(a, offset):
    """`a` on the device inside a longer poisoned allocation: `offset` floats of poison before it (offset 1: the data start 4
    bytes off a 16-byte boundary), poison after it."""
    a = np.ascontiguousarray(a)
    n = a.size
    if a.dtype == np.float32:
        t = poisoned(n + 64 + offset)
    else:
        t = torch.full((n + 64 + offset,), 0xAB if a.dtype == np.uint8 else float("nan"), dtype=torch.from_numpy(a).dtype, device=DEV)
    v = t[offset:offset + n]
    v.copy_(up(a.reshape(-1)))
    return v.view(a.shape)


def make(size, E, D, A, **kw):
    from fleetrl_amd import DeviceReplayBuffer

    return DeviceReplayBuffer(size, E, D, A, **kw)


def arrays_equal(buf, model):
    for n in rp.ARRAYS:
        if not same(getattr(buf, n), getattr(model, n)):
            return n
    return None


def signed_magnitudes(rng, shape):
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-6, 4, shape)).astype(np.float32)


def done_pattern(name, rng, E):
    if name == "none":
        return np.zeros(E, np.uint8)
    if name == "all":
        return np.ones(E, np.uint8)
    if name == "every7th":
        return (np.arange(E) % 7 == 0).astype(np.uint8)
    d = (rng.random(E) < 0.3).astype(np.uint8)
    d[rng.integers(E)] = 200  # any non-zero byte is a done
    return d


# ---- add -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 50])
@pytest.mark.parametrize("D", [7, 388])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 300, 4096])
def test_add_equals_the_model_after_every_add(E, D, A):
    """R = 5, 13 adds (two wraps); float64 / float32 rewards, the four done patterns, with and without terminal rows and timeouts,
    sources 16-byte aligned and 4 bytes off, poison in every byte that must not be read."""
    rng = np.random.default_rng(E * 1000 + D * 10 + A)
    buf, model = make(5 * E, E, D, A), rp.ReplayModel(5 * E, E, D, A)
    assert buf.rows == 5 and buf.size() == 0
    patterns = ("none", "all", "every7th", "random")
    for k in range(13):
        done = done_pattern(patterns[k % 4], rng, E)
        obs, nxt, act = signed_magnitudes(rng, (E, D)), signed_magnitudes(rng, (E, D)), signed_magnitudes(rng, (E, A))
        rew = rng.standard_normal(E) * 10.0 ** rng.uniform(-3, 3, E)
        if k % 2:
            rew = rew.astype(np.float32)
        term = signed_magnitudes(rng, (E, D))
        term_dev = term.copy()
        term_dev[done == 0] = POISON  # stale rows: must never reach the buffer
        use_term, use_tmo = k % 5 != 4, k % 3 == 0
        tmo = (done != 0) & (rng.random(E) < 0.5) if use_tmo else None
        off = (k // 2) % 2  # 0: aligned, 1: the scalar path
        buf.add(source(obs, off), source(nxt, off), source(act, off), source(rew, 0), source(done, 0),
                source(term_dev, off) if use_term else None, source(tmo.astype(np.uint8), 0) if use_tmo else None)
        model.add(obs, nxt, act, rew, done, term if use_term else None, tmo)
        assert arrays_equal(buf, model) is None, (k, arrays_equal(buf, model))
        assert (buf.pos, buf.full, buf.size()) == (model.pos, model.full, model.upper())
    assert not np.isnan(buf.next_observations.cpu().numpy()).any()
    buf.check_errors()
    buf.close()


# ---- gather ----------------------------------------------------------------------------------------------------------------------
def stats_of(norm):
    st, s = norm.get_state(), norm.settings
    return dict(obs_mean=st.obs_rms.mean, obs_var=st.obs_rms.var, ret_var=float(st.ret_rms.var), norm_obs=s.norm_obs,
                norm_reward=s.norm_reward, clip_obs=s.clip_obs, clip_reward=s.clip_reward, epsilon=s.epsilon)


def norm_batch(rng, E, D, shift=0.0):
    """observations whose column 0 is 1e4 +- 0.1 and whose column 1 is constant"""
    x = (rng.standard_normal((E, D)) * 3 + shift).astype(np.float32)
    x[:, 0] = (1e4 + rng.uniform(-0.1, 0.1, E)).astype(np.float32)
    if D > 1:
        x[:, 1] = 2.5
    return x


def step_norm(norm, rng, E, D, shift=0.0):
    norm.step_torch(up(norm_batch(rng, E, D, shift)), up(rng.standard_normal(E) * 5), up((rng.random(E) < 0.1).astype(np.uint8)))


def fill(buf, model, rng, adds, E, D, A):
    for _ in range(adds):
        obs, nxt = norm_batch(rng, E, D), norm_batch(rng, E, D)
        obs[rng.integers(E), 0] = 2e4  # far outside the column's spread, even with the trace of the statistics' start: the clip
        if D > 1:
            nxt[rng.integers(E), 1] = 3.5  # off the constant column: (1 / sqrt(eps)) clipped
        act, rew = signed_magnitudes(rng, (E, A)), rng.standard_normal(E) * 10.0 ** rng.uniform(-2, 3, E)
        done = done_pattern("random", rng, E)
        term, tmo = norm_batch(rng, E, D, 1.0), ((done != 0) & (rng.random(E) < 0.5)).astype(np.uint8)
        buf.add(up(obs), up(nxt), up(act), up(rew), up(done), up(term), up(tmo))
        model.add(obs, nxt, act, rew, done, term, tmo)


@pytest.mark.parametrize("E,D,A", [(64, 388, 50), (37, 7, 3), (300, 1438, 5), (5, 3100, 1)])
@pytest.mark.parametrize("mode", ["none", "obs_off", "reward_off", "both"])
def test_gather_equals_the_model_under_the_current_statistics(E, D, A, mode):
    from fleetrl_amd import DeviceNormalizer

    rng = np.random.default_rng(E + D)
    R = 6
    buf, model = make(R * E, E, D, A), rp.ReplayModel(R * E, E, D, A)
    norm = None
    if mode != "none":
        norm = DeviceNormalizer(E, D, norm_obs=mode != "obs_off", norm_reward=mode != "reward_off")
        step_norm(norm, rng, E, D)
    fill(buf, model, rng, R + 2, E, D, A)
    if norm is not None:
        for _ in range(3):  # the statistics move on after the rows were added
            step_norm(norm, rng, E, D, 0.5)
    # every transition once, then repeats
    rows = np.concatenate([np.repeat(np.arange(R), E), rng.integers(0, R, 500)]).astype(np.int32)
    envs = np.concatenate([np.tile(np.arange(E), R), rng.integers(0, E, 500)]).astype(np.int32)
    perm = rng.permutation(rows.size)
    rows, envs = rows[perm], envs[perm]
    got = buf.gather(up(rows), up(envs), env=norm)
    stats1 = None if norm is None else stats_of(norm)
    want = model.get_samples(rows, envs, stats1)
    for name, g, w in zip(got._fields, got, want):
        assert same(g, w), name
    assert got.dones.shape == got.rewards.shape == (rows.size, 1)
    if mode in ("both", "reward_off"):
        w = want[0]
        assert (w == 10.0).any() and (w[:, 0] != 10.0).any(), "the clip is reached, and not everywhere"
        if D > 1:
            # the constant column (batch variance 0 in every update; the running one keeps a trace of its start at 1)
            assert (want[2][:, 1] == 10.0).any() and (np.abs(want[2][:, 1]) < 1).any()
    if norm is not None:
        step_norm(norm, rng, E, D, -2.0)
        got2 = buf.gather(up(rows), up(envs), env=norm)
        want2 = model.get_samples(rows, envs, stats_of(norm))
        for name, g, w in zip(got2._fields, got2, want2):
            assert same(g, w), name
        if mode != "obs_off":
            assert not same(got2.observations, got.observations)
        if mode != "reward_off":
            assert not same(got2.rewards, got.rewards)
        norm.close()
    buf.check_errors()
    buf.close()


def test_gather_needs_a_normaliser_of_the_same_width():
    from fleetrl_amd import DeviceNormalizer, FleetHipError, _capi

    buf = make(16, 4, 6, 2)
    buf.add(*(up(np.zeros(s, np.float32)) for s in ((4, 6), (4, 6), (4, 2))), up(np.zeros(4)), up(np.zeros(4, np.uint8)))
    norm = DeviceNormalizer(4, 5)
    z = up(np.zeros(2, np.int32))
    with pytest.raises(FleetHipError) as ei:
        buf.gather(z, z, env=norm)
    assert ei.value.status == _capi.ERR_INVALID and "obs_dim" in str(ei.value)
    with pytest.raises(TypeError):
        buf.gather(z, z, env=object())
    norm.close()
    buf.close()


@pytest.mark.parametrize("bad", ["row", "env", "negative"])
def test_an_index_out_of_range_writes_nothing_and_is_reported_once(bad):
    from fleetrl_amd import FleetHipError, ReplayBatch, _capi

    E, D, A, R = 9, 8, 4, 5
    rng = np.random.default_rng(3)
    buf, model = make(R * E, E, D, A), rp.ReplayModel(R * E, E, D, A)
    fill(buf, model, rng, 3, E, D, A)  # upper = 3 of 5 rows
    rows, envs = np.array([0, 2, 1, 2], np.int32), np.array([0, 8, 3, 5], np.int32)
    if bad == "row":
        rows[1] = 3  # a row of the allocation, but not filled yet
    elif bad == "env":
        envs[2] = E
    else:
        rows[1], envs[2] = -1, -5
    out = ReplayBatch(poisoned((4, D)), poisoned((4, A)), poisoned((4, D)), poisoned((4, 1)), poisoned((4, 1)))
    buf.gather(up(rows), up(envs), out=out)
    ok = np.array([True, bad == "env", bad == "row", True])
    want = model.get_samples(np.where(ok, rows, 0), np.where(ok, envs, 0))
    for name, g, w in zip(out._fields, out, want):
        g = bits(g)
        assert np.array_equal(g[ok], bits(w)[ok]), name
        assert (g[~ok] == 0x7FC0DEAD).all(), name
    with pytest.raises(FleetHipError) as ei:
        buf.check_errors()
    assert ei.value.status == _capi.ERR_STATE
    buf.check_errors()  # once and only once
    buf.gather(up(rows[:1]), up(envs[:1]))
    buf.check_errors()
    buf.close()


# ---- sample ----------------------------------------------------------------------------------------------------------------------
def draw_tensors(B):
    return torch.full((B,), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("B", [1, 255, 256, 65536])
@pytest.mark.parametrize("filled", ["partial", "full"])
def test_sample_draws_the_models_indices_and_gathers_them(B, filled):
    from fleetrl_amd import DeviceNormalizer

    E, D, A, R, seed = 300, 12, 3, 5, 0x1234_5678_9ABC_DEF0
    rng = np.random.default_rng(B)
    buf, twin, model = make(R * E, E, D, A, seed=seed), make(R * E, E, D, A, seed=seed), rp.ReplayModel(R * E, E, D, A, seed=seed)
    fill(buf, model, rng, 3 if filled == "partial" else 7, E, D, A)
    for n in rp.ARRAYS:
        getattr(twin, n).copy_(getattr(buf, n))
    twin.set_position(buf.pos, buf.full, 0)
    upper = 3 if filled == "partial" else R
    assert buf.size() == upper == model.upper()
    norm = DeviceNormalizer(E, D)
    step_norm(norm, rng, E, D)
    stats = stats_of(norm)
    drawn = []
    for call in range(2):
        ri, ei = draw_tensors(B)
        got = buf.sample(B, env=norm, indices_out=(ri, ei))
        wr, we = rp.draw(seed, call, B, upper, E)
        assert same(ri, wr) and same(ei, we), call
        (want, mr, me) = model.sample(B, stats)
        assert np.array_equal(mr, wr) and np.array_equal(me, we)
        for name, g, w in zip(got._fields, got, want):
            assert same(g, w), (call, name)
        again = buf.gather(ri, ei, env=norm)  # the five outputs are a gather at the drawn indices
        for name, g, w in zip(got._fields, got, again):
            assert same(g, w), (call, name)
        drawn.append((bits(ri).copy(), bits(ei).copy(), got))
    if B > 1:
        assert not np.array_equal(drawn[0][0], drawn[1][0]) or not np.array_equal(drawn[0][1], drawn[1][1])
    assert buf.calls == 2
    # a second buffer with the same seed agrees, call by call
    for call in range(2):
        ri, ei = draw_tensors(B)
        got = twin.sample(B, env=norm, indices_out=(ri, ei))
        assert same(ri, drawn[call][0]) and same(ei, drawn[call][1])
        assert all(same(g, w) for g, w in zip(got, drawn[call][2]))
    # an earlier call counter replays its minibatch
    buf.set_position(buf.pos, buf.full, 1)
    ri, ei = draw_tensors(B)
    got = buf.sample(B, env=norm, indices_out=(ri, ei))
    assert same(ri, drawn[1][0]) and same(ei, drawn[1][1]) and all(same(g, w) for g, w in zip(got, drawn[1][2]))
    raw = buf.sample(B)  # call 2, no normaliser, no index outputs
    wr, we = rp.draw(seed, 2, B, upper, E)
    assert all(same(g, w) for g, w in zip(raw, model.get_samples(wr, we)))
    buf.check_errors()
    norm.close()
    buf.close()
    twin.close()


def test_sample_on_an_empty_buffer_is_a_state_error():
    from fleetrl_amd import FleetHipError, _capi

    buf = make(64, 8, 5, 2)
    with pytest.raises(FleetHipError) as ei:
        buf.sample(4)
    assert ei.value.status == _capi.ERR_STATE and "empty" in str(ei.value) and buf.calls == 0
    buf.close()


# ---- in the loop, full size --------------------------------------------------------------------------------------------------------
def run_loop(steps, R, B, model=None):
    """4096 x 50 under FleetVecNormalize on torch's stream; returns the buffer, the final statistics and one minibatch."""
    sys.path.insert(0, ROOT)
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    E, N = 4096, 50
    env = FleetVecNormalize(FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=0), clip_reward=10.0)
    D = env.norm.D
    assert D == 388
    buf = make(R * E, E, D, N, seed=99)
    g = torch.Generator(device=DEV).manual_seed(5)
    tape = torch.rand((16, E, N), device=DEV, generator=g) * 2 - 1
    term_out = torch.empty((E, D), device=DEV)
    env.reset_torch()
    prev = env.original_torch().obs.clone()
    n_done = 0
    for t in range(steps):
        act = tape[t % 16]
        env.original_torch().terminal.copy_(poisoned((E, D)))  # what the step does not write stays poison
        _, _, done = env.step_torch(act, terminal_out=term_out)
        o = env.original_torch()
        buf.add(prev, o.obs, act, o.reward, done, terminal=o.terminal)
        if model is not None:
            d = done.cpu().numpy()
            n_done += int(d.sum())
            model.add(prev.cpu().numpy(), o.obs.cpu().numpy(), act.cpu().numpy(), o.reward.cpu().numpy(), d, o.terminal.cpu().numpy())
        prev = o.obs.clone()
    ri, ei = draw_tensors(B)
    batch = buf.sample(B, env=env, indices_out=(ri, ei))
    buf.check_errors()
    return env, buf, batch, (ri, ei), n_done


def test_full_size_loop_equals_the_shadow_buffer_and_repeats():
    steps, R, B = 300, 192, 65536
    model = rp.ReplayModel(R * 4096, 4096, 388, 50, seed=99)
    env, buf, batch, (ri, ei), n_done = run_loop(steps, R, B, model)
    assert n_done > 0, "some episodes ended: terminal rows were substituted"
    assert (buf.pos, buf.full) == (steps % R, True) == (model.pos, model.full)
    assert arrays_equal(buf, model) is None, arrays_equal(buf, model)
    wr, we = rp.draw(99, 0, B, R, 4096)
    assert same(ri, wr) and same(ei, we)
    want = model.get_samples(wr, we, stats_of(env.norm))
    for name, g, w in zip(batch._fields, batch, want):
        assert same(g, w), name
    del model
    first = {n: getattr(buf, n).clone() for n in rp.ARRAYS}
    first_batch = [x.clone() for x in batch]
    env.close()
    buf.close()
    env2, buf2, batch2, _, _ = run_loop(steps, R, B)
    for n in rp.ARRAYS:
        assert torch.equal(getattr(buf2, n).view(torch.uint8), first[n].view(torch.uint8)), n
    for a, b in zip(batch2, first_batch):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    env2.close()
    buf2.close()


# ---- streams ---------------------------------------------------------------------------------------------------------------------
def test_sample_on_the_buffers_own_stream_sees_the_normalisers_last_enqueued_step():
    """The normaliser steps on torch's stream, the buffer samples on its own: no synchronisation by the caller in between."""
    from fleetrl_amd import DeviceNormalizer

    E, D, A, R, B = 4096, 388, 50, 4, 4096
    rng = np.random.default_rng(8)
    buf, model = make(R * E, E, D, A, seed=4), rp.ReplayModel(R * E, E, D, A, seed=4)
    fill(buf, model, rng, R, E, D, A)
    torch.cuda.synchronize()
    own = torch.cuda.Stream()
    buf.set_stream(own.cuda_stream)  # a side stream nobody else waits on
    norm = DeviceNormalizer(E, D)
    outs = [torch.empty((B, D), device=DEV), torch.empty((B, A), device=DEV), torch.empty((B, D), device=DEV),
            torch.empty((B, 1), device=DEV), torch.empty((B, 1), device=DEV)]
    ri, ei = draw_tensors(B)
    batches = [(up(norm_batch(rng, E, D, k)), up(rng.standard_normal(E) * 5), up(np.zeros(E, np.uint8))) for k in range(20)]
    torch.cuda.synchronize()
    for x, r, d in batches:  # a queue of updates on torch's stream, the sample enqueued right behind the last of them
        norm.step_torch(x, r, d)
    buf.sample_dev(B, norm, *(o.data_ptr() for o in outs), ri.data_ptr(), ei.data_ptr())
    norm.step_torch(*batches[0])  # ... and an update behind the sample must wait for it
    buf.check_errors()  # waits for the buffer's stream
    torch.cuda.synchronize()
    stats_after = stats_of(norm)
    # the statistics the sample must have seen: those after 20 steps, rebuilt on a second normaliser
    ref = DeviceNormalizer(E, D)
    for x, r, d in batches:
        ref.step_torch(x, r, d)
    stats = stats_of(ref)
    assert not np.array_equal(stats["obs_mean"], stats_after["obs_mean"])
    wr, we = rp.draw(4, 0, B, R, E)
    assert same(ri, wr) and same(ei, we)
    want = model.get_samples(wr, we, stats)
    for name, g, w in zip(("observations", "actions", "next_observations", "dones", "rewards"), outs, want):
        assert same(g, w), name
    ref.close()
    norm.close()
    buf.close()
