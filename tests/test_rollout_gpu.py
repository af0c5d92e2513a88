"""The rollout buffer on the device (fleet_rollout.hip) against the NumPy model of tests/rollout_model.py, bit for bit.  Needs an
MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rollout_model as rm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def signed_magnitudes(rng, shape):
    """1e-6 .. 1e4, both signs"""
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-6, 4, shape)).astype(np.float32)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make(E, K, D=1, A=1, **kw):
    from fleetrl_amd import DeviceRolloutBuffer

    return DeviceRolloutBuffer(E, K, D, A, **kw)


# ---- advantages and returns -----------------------------------------------------------------------------------------------------
DONE_PATTERNS = ("none", "all", "last_row", "final_dones", "bernoulli", "one_env_always")
GAMMA_LAMBDA = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.0), (1.0, 0.95), (0.99, 1.0), (0.0, 0.95), (0.99, 0.0), (0.99, 0.9))


def done_pattern(name, rng, K, E):
    starts, dones = np.zeros((K, E), np.uint8), np.zeros(E, np.uint8)
    if name == "all":
        starts[:], dones[:] = 1, 1
    elif name == "last_row":
        starts[K - 1] = 1
    elif name == "final_dones":
        dones[:] = 1
    elif name == "bernoulli":
        starts = (rng.random((K, E)) < 1 / 192).astype(np.uint8)
        dones = (rng.random(E) < 1 / 192).astype(np.uint8)
        starts[rng.integers(K), rng.integers(E)] = 255  # any non-zero byte is a start
    elif name == "one_env_always":
        starts[:, E // 2], dones[E // 2] = 1, 1
    return starts, dones


@pytest.mark.parametrize("K", [1, 2, 61, 192, 2048])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 300, 4096])
def test_gae_equals_the_model_bit_for_bit(E, K):
    rng = np.random.default_rng(E * 10000 + K)
    for gamma, lam in GAMMA_LAMBDA:
        buf = make(E, K, gamma=gamma, gae_lambda=lam)
        for pattern in DONE_PATTERNS:
            r, v, lv = signed_magnitudes(rng, (K, E)), signed_magnitudes(rng, (K, E)), signed_magnitudes(rng, E)
            starts, dones = done_pattern(pattern, rng, K, E)
            buf.rewards.copy_(up(r))
            buf.values.copy_(up(v))
            buf.episode_starts.copy_(up(starts))
            buf.advantages.fill_(float("nan"))
            buf.returns.fill_(float("nan"))
            buf.compute_returns_and_advantage(up(lv), up(dones))
            adv, ret = rm.gae(r, v, starts, lv, dones, gamma, lam)
            tag = (gamma, lam, pattern)
            assert same(buf.advantages, adv), tag
            assert same(buf.returns, ret), tag
            assert same(buf.rewards, r) and same(buf.values, v) and same(buf.episode_starts, starts), tag  # inputs untouched
        buf.check_errors()
        buf.close()


def test_gae_accepts_a_critics_column_and_bool_dones():
    E, K = 65, 7
    rng = np.random.default_rng(3)
    buf = make(E, K)
    r, v, lv = signed_magnitudes(rng, (K, E)), signed_magnitudes(rng, (K, E)), signed_magnitudes(rng, E)
    buf.rewards.copy_(up(r))
    buf.values.copy_(up(v))
    dones = rng.random(E) < 0.5
    buf.compute_returns_and_advantage(up(lv).reshape(E, 1), up(dones))
    adv, ret = rm.gae(r, v, np.zeros((K, E), np.uint8), lv, dones, 0.99, 0.95)
    assert same(buf.advantages, adv) and same(buf.returns, ret)
    buf.close()


# ---- add ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,D,A", [(7, 37, 5), (64, 388, 50), (300, 388, 3), (4096, 388, 50)])
def test_add_stores_rows_and_rounds_a_float64_reward_once(E, D, A):
    K = 3
    rng = np.random.default_rng(E + D)
    buf, model = make(E, K, D, A), rm.RolloutModel(E, K, D, A)
    for t in range(K):
        obs, act = rng.normal(0, 3, (E, D)).astype(np.float32), rng.normal(0, 1, (E, A)).astype(np.float32)
        rew = rng.normal(0, 5, E) * (1 + 2.0 ** -30)  # float64 values that are not float32 values
        rew[0] = 1.0 + 2.0 ** -25                      # a quarter of float32's spacing above 1: rounds to 1.0
        if t == 1:
            rew = rew.astype(np.float32)               # the float32 entry
        start = (rng.random(E) < 0.3).astype(np.uint8)
        val, logp = signed_magnitudes(rng, E), -np.abs(signed_magnitudes(rng, E))
        assert buf.pos == t and not buf.full
        buf.add(up(obs), up(act), up(rew), up(start), up(val).reshape(E, 1), up(logp))
        model.add(obs, act, rew, start, val, logp)
    assert buf.full and buf.pos == K
    for name, dev in (("obs", buf.observations), ("actions", buf.actions), ("rewards", buf.rewards), ("episode_starts", buf.episode_starts),
                      ("values", buf.values), ("log_probs", buf.log_probs)):
        assert same(dev, getattr(model, name)), name
    assert buf.rewards[0, 0].item() == 1.0
    with pytest.raises(Exception):
        buf.add(up(obs), up(act), up(rew), up(start), up(val), up(logp))  # full
    buf.reset()
    assert buf.pos == 0 and not buf.full
    buf.add(obs, act, rew, start, val, logp)  # NumPy input is copied up
    assert same(buf.observations[0], obs) and same(buf.rewards[0], rew.astype(np.float32))
    buf.close()


def test_add_skips_what_was_written_in_place():
    """The row's own addresses (slot) as sources: those arrays are not copied over -- the row keeps, bit for bit, the poison
    pattern (NaN payloads included) that was written into it, while the other arrays arrive."""
    E, K, D, A, t = 65, 4, 388, 50, 2
    rng = np.random.default_rng(5)
    buf = make(E, K, D, A)
    s = buf.slot(t)
    assert s.obs.data_ptr() == buf.observations[t].data_ptr() == buf.slot_dev(t).obs and s.obs.shape == (E, D)
    assert s.episode_start.data_ptr() == buf.slot_dev(t).episode_start and s.episode_start.dtype == torch.uint8
    poison_obs = rng.integers(0, 2 ** 32, (E, D), dtype=np.uint32)
    poison_obs[::3] |= 0x7FC00000  # quiet NaNs with payloads
    poison_start = rng.integers(0, 256, E, dtype=np.uint8)
    s.obs.view(torch.int32).copy_(up(poison_obs.view(np.int32)))
    s.episode_start.copy_(up(poison_start))
    act, rew = rng.normal(0, 1, (E, A)).astype(np.float32), rng.normal(0, 5, E)
    val, logp = signed_magnitudes(rng, E), signed_magnitudes(rng, E)
    buf.pos = t
    buf.add(s.obs, up(act), up(rew), s.episode_start, up(val), up(logp))
    torch.cuda.synchronize()
    assert np.array_equal(s.obs.view(torch.int32).cpu().numpy().view(np.uint32), poison_obs)
    assert np.array_equal(s.episode_start.cpu().numpy(), poison_start)
    assert same(buf.actions[t], act) and same(buf.rewards[t], rew.astype(np.float32)) and same(buf.values[t], val) and same(buf.log_probs[t], logp)
    # every array in place, float32 reward included: the launch changes nothing at all
    before = {n: getattr(buf, n).clone() for n in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs")}
    buf.pos = t
    buf.add(*s)
    for n, b in before.items():
        a = getattr(buf, n)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), n
    # a float64 reward cannot live at the row's float32 address
    from fleetrl_amd import FleetHipError, _capi

    sd = buf.slot_dev(t)
    with pytest.raises(FleetHipError) as ei:
        buf.add_dev(t, sd.obs, sd.actions, sd.reward, _capi.ACT_F64, sd.episode_start, sd.value, sd.log_prob)
    assert ei.value.status == _capi.ERR_INVALID
    with pytest.raises(FleetHipError):
        buf.add_dev(K, sd.obs, sd.actions, sd.reward, _capi.ACT_F32, sd.episode_start, sd.value, sd.log_prob)
    buf.close()


@pytest.mark.parametrize("f64", [True, False])
@pytest.mark.parametrize("gamma", [0.99, 1.0, 0.0])
def test_add_bootstraps_done_rows_only(f64, gamma):
    E, K, D, A = 300, 2, 5, 2
    rng = np.random.default_rng(9)
    buf, model = make(E, K, D, A, gamma=gamma), rm.RolloutModel(E, K, D, A, gamma=gamma)
    obs, act = rng.normal(0, 3, (E, D)).astype(np.float32), rng.normal(0, 1, (E, A)).astype(np.float32)
    rew = rng.normal(0, 5, E) if f64 else rng.normal(0, 5, E).astype(np.float32)
    start, done = np.zeros(E, np.uint8), (rng.random(E) < 0.4).astype(np.uint8)
    done[0], done[1] = 0, 200
    val, logp, tv = signed_magnitudes(rng, E), signed_magnitudes(rng, E), signed_magnitudes(rng, E)
    buf.add(up(obs), up(act), up(rew), up(start), up(val), up(logp), terminal_value=up(tv), done=up(done))
    model.add(obs, act, rew, start, val, logp, tv, done)
    buf.add(up(obs), up(act), up(rew), up(start), up(val), up(logp))  # NULL: nothing
    model.add(obs, act, rew, start, val, logp)
    assert same(buf.rewards, model.rewards)
    r32 = rew.astype(np.float32)
    assert same(buf.rewards[1], r32) and same(buf.rewards[0][up(done == 0)], r32[done == 0])
    if not f64:  # in place: the row's own float32 reward is bootstrapped where done
        buf.reset()
        s = buf.slot(0)
        s.reward.copy_(up(rew))
        buf.add(up(obs), up(act), s.reward, up(start), up(val), up(logp), terminal_value=up(tv), done=up(done))
        assert same(buf.rewards[0], model.rewards[0])
    buf.close()


# ---- gather ---------------------------------------------------------------------------------------------------------------------
def filled(E, K, D, A, seed):
    rng = np.random.default_rng(seed)
    buf, model = make(E, K, D, A), rm.RolloutModel(E, K, D, A)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    for name, m_name in (("observations", "obs"), ("actions", "actions"), ("values", "values"), ("log_probs", "log_probs"),
                         ("advantages", "advantages"), ("returns", "returns")):
        t = getattr(buf, name)
        t.copy_(torch.randn(t.shape, device=DEV, generator=gen))
        setattr(model, m_name, t.cpu().numpy())
    buf.pos, buf.full = K, True
    return buf, model, rng


def check_batch(batch, model, idx):
    want = model.sample(idx)
    for name, got, w in zip(batch._fields, batch, want):
        assert got.dtype == torch.float32 and tuple(got.shape) == w.shape, name
        assert same(got, w), name


@pytest.mark.parametrize("E,K,D,A", [(512, 192, 388, 50), (300, 61, 37, 5), (64, 16, 388, 8)])
def test_gather_equals_fancy_indexing_of_the_flattened_view(E, K, D, A):
    buf, model, rng = filled(E, K, D, A, seed=E + D)
    n = E * K
    perm = rng.permutation(n).astype(np.int32)
    check_batch(buf.gather(up(perm)), model, perm)  # a full permutation
    for B in (1, 128, 65536, 1000 + 37):
        if B > n:
            continue
        idx = rng.integers(0, n, B).astype(np.int32)  # with repeats
        check_batch(buf.gather(up(idx)), model, idx)
    # get(): SB3's minibatches over a fresh permutation, remainder included
    for bs in (None, 128 if n <= 1 << 15 else 65536, 4000 + 37):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(77)
        want_perm = torch.randperm(n, device=DEV, dtype=torch.int32, generator=gen).cpu().numpy()
        gen.manual_seed(77)
        sizes, start = [], 0
        for batch in buf.get(bs, generator=gen):
            B = batch.observations.shape[0]
            check_batch(batch, model, want_perm[start:start + B])
            sizes.append(B)
            start += B
        step = n if bs is None else bs
        assert start == n and sizes == [min(step, n - s) for s in range(0, n, step)]
    buf.check_errors()
    buf.close()


def test_get_draws_a_fresh_permutation_and_needs_a_full_buffer():
    buf, model, _ = filled(64, 16, 8, 2, seed=1)
    a = next(iter(buf.get(None))).returns.cpu().numpy()
    b = next(iter(buf.get(None))).returns.cpu().numpy()
    assert not np.array_equal(a, b) and np.array_equal(np.sort(a), np.sort(b))
    assert np.array_equal(np.sort(a), np.sort(model.returns.reshape(-1)))
    buf.reset()
    with pytest.raises(Exception):
        next(iter(buf.get(None)))
    buf.close()


def test_gather_into_a_misaligned_output_takes_the_scalar_path():
    from fleetrl_amd.rollout import RolloutBatch

    E, K, D, A, B = 300, 16, 388, 52, 1000
    buf, model, rng = filled(E, K, D, A, seed=4)
    idx = rng.integers(0, E * K, B).astype(np.int32)
    flat_o, flat_a = torch.full((B * D + 1,), -7.0, device=DEV), torch.full((B * A + 3,), -7.0, device=DEV)
    out = RolloutBatch(flat_o[1:].view(B, D), flat_a[3:].view(B, A), *(torch.empty(B, device=DEV) for _ in range(4)))
    assert out.observations.data_ptr() % 16 == 4 and out.actions.data_ptr() % 16 == 12
    got = buf.gather(up(idx), out=out)
    check_batch(got, model, idx)
    assert flat_o[0].item() == -7.0 and torch.all(flat_a[:3] == -7.0)
    # ... and only some of the outputs
    part = RolloutBatch(None, None, None, None, torch.empty(B, device=DEV), None)
    buf.gather(up(idx), out=part)
    assert same(part.advantages, model.sample(idx)[4])
    buf.close()


def test_gather_out_of_range_index_is_an_error_return():
    from fleetrl_amd import FleetHipError, _capi
    from fleetrl_amd.rollout import RolloutBatch

    E, K, D, A, B = 65, 9, 388, 5, 257
    buf, model, rng = filled(E, K, D, A, seed=6)
    n = E * K
    idx = rng.integers(0, n, B).astype(np.int32)
    bad = {0: -1, 17: n, 100: n + 12345, 256: np.iinfo(np.int32).min, 255: np.iinfo(np.int32).max}
    for b, v in bad.items():
        idx[b] = v
    out = RolloutBatch(torch.full((B, D), 123.5, device=DEV), torch.full((B, A), 123.5, device=DEV),
                       *(torch.full((B,), 123.5, device=DEV) for _ in range(4)))
    buf.gather(up(idx), out=out)
    good = np.array([b not in bad for b in range(B)])
    want = model.sample(idx[good])
    for got, w in zip(out, want):
        g = got.cpu().numpy()
        assert same(g[good], w)
        assert np.all(g[~good] == 123.5)  # untouched
    with pytest.raises(FleetHipError) as ei:
        buf.check_errors()
    assert ei.value.status == _capi.ERR_STATE
    buf.check_errors()  # once: clean afterwards
    ok = rng.integers(0, n, B).astype(np.int32)
    check_batch(buf.gather(up(ok)), model, ok)
    buf.check_errors()
    buf.close()


# ---- integration ----------------------------------------------------------------------------------------------------------------
def make_env(E, N, seed=5):
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv
    from fleetrl_amd.synth import synth_tables

    return FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=seed)


class LinearPolicy:
    """A fixed, seeded policy that is linear in the observation and bit-reproducible by construction: elementwise products and
    torch's (atomic-free) row sums, no GEMM whose split could depend on the library's choice of kernel."""

    def __init__(self, D, N, seed):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed)
        self.cols = torch.randint(0, D, (N,), device=DEV, generator=gen)
        self.w = torch.randn(N, device=DEV, generator=gen)
        self.b = 0.3 * torch.randn(N, device=DEV, generator=gen)
        self.wv = torch.randn(D, device=DEV, generator=gen) / D

    def __call__(self, obs):
        act = (obs[:, self.cols] * self.w + self.b).clamp(-1, 1)
        value = (obs * self.wv).sum(1)
        log_prob = -0.5 * (act * act).sum(1)
        return act, value, log_prob


def rollout(E, N, K, in_place):
    """K steps of FleetVecNormalize(FleetVecEnv) under the linear policy -> the eight arrays (NumPy), last_values, dones.
    in_place: observations and dones land in the buffer's rows, add() stores the rest, the buffer computes the GAE;
    otherwise: plain tensors, every step's cloned, no buffer anywhere."""
    from fleetrl_amd import FleetVecNormalize

    env = make_env(E, N)
    vn = FleetVecNormalize(env, clip_reward=10.0)
    D = env.core.obs_dim
    pi = LinearPolicy(D, N, seed=E + N)
    rew = torch.empty(E, device=DEV, dtype=torch.float64)
    if in_place:
        buf = make(E, K, D, N)
        obs, start = buf.slot(0).obs, buf.slot(0).episode_start
        vn.reset_torch(obs_out=obs)
        start.fill_(1)
        spare_obs, spare_done = torch.empty((E, D), device=DEV), torch.empty(E, device=DEV, dtype=torch.uint8)
        for t in range(K):
            act, value, logp = pi(obs)
            nxt = buf.slot(t + 1) if t + 1 < K else None
            nobs, ndone = (nxt.obs, nxt.episode_start) if nxt else (spare_obs, spare_done)
            vn.step_torch(act, obs_out=nobs, reward_out=rew, done_out=ndone)
            buf.add(obs, act, rew, start, value, logp)
            obs, start = nobs, ndone
        _, last_values, _ = pi(obs)
        buf.compute_returns_and_advantage(last_values, start)
        buf.check_errors()
        out = {n: getattr(buf, "observations" if n == "obs" else n).cpu().numpy() for n in rm.ARRAYS}
        out["last_values"], out["dones"] = last_values.cpu().numpy(), start.cpu().numpy()
        buf.close()
    else:
        obs = vn.reset_torch()
        start = torch.ones(E, device=DEV, dtype=torch.uint8)
        rows = {n: [] for n in rm.ARRAYS[:6]}
        for t in range(K):
            act, value, logp = pi(obs)
            nobs, _, ndone = vn.step_torch(act, reward_out=rew)
            for n, v in zip(rm.ARRAYS[:6], (obs, act, rew.float(), start, value, logp)):
                rows[n].append(v.clone())
            obs, start = nobs, ndone
        _, last_values, _ = pi(obs)
        out = {n: torch.stack(v).cpu().numpy() for n, v in rows.items()}
        out["last_values"], out["dones"] = last_values.cpu().numpy(), start.cpu().numpy()
    vn.close()
    return out


@pytest.mark.parametrize("E,N,K", [(4096, 50, 192), (7, 3, 5)])
def test_rollout_through_the_buffer_equals_cloning_every_step(E, N, K):
    a = rollout(E, N, K, in_place=True)
    b = rollout(E, N, K, in_place=False)
    for n in rm.ARRAYS[:6]:
        assert a[n].dtype == b[n].dtype and a[n].shape == b[n].shape, n
        assert same(a[n], b[n]), n
    assert same(a["last_values"], b["last_values"]) and same(a["dones"], b["dones"])
    assert a["episode_starts"][0].all() and a["obs"].shape[:2] == (K, E) and np.isfinite(a["rewards"]).all()
    if K == 192:
        assert a["dones"].all()  # the 192-step episodes end on the rollout's last step: the GAE sees the time limit
    adv, ret = rm.gae(b["rewards"], b["values"], b["episode_starts"], b["last_values"], b["dones"], 0.99, 0.95)
    assert same(a["advantages"], adv) and same(a["returns"], ret)
    c = rollout(E, N, K, in_place=True)  # a second run reproduces the first
    for n in a:
        assert a[n].tobytes() == c[n].tobytes(), n


def test_example_ppo_device_loop_runs():
    """examples/ppo_device_loop.py as a child process under a time limit of its own: exit 0, finite losses."""
    import json

    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "ppo_device_loop.py"), "--iterations", "2",
           "--envs", "64", "--steps", "16"]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 2
    for ln in lines:
        for k in ("policy_loss", "value_loss", "mean_reward"):
            assert np.isfinite(ln[k]), ln
