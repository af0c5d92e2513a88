"""Rollout collection on the device (fleet_collect.hip): the episode ring's kernel on given arrays against tests/collect_model.py bit for
bit, the PPO call and the TD3 call against the existing pieces run step by step (the loops of examples/ppo_device_train.py and
examples/td3_pink_noise.py) bit for bit, what a result may not depend on, the launch counts, the refusals that need handles, and the
two examples."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import collect_model as cm
import policy_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
SEED = 0x1234567890ABCDEF  # (both key words in use)
EP_HOURS = 2               # episodes of 8 steps: they end inside a rollout of 9, twice inside two


def dev():
    return torch.device("cuda", 0)


def host(t):
    return t.detach().cpu().numpy().copy()


def same(a, b) -> bool:
    """Bit equality of two arrays of one dtype and shape."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_env(E, N, with_norm, seed=1):
    from bench import bench_config

    from fleetrl_amd import FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    venv = FleetVecEnv(dict(bench_config(E, N, "ct"), episode_length=EP_HOURS), E, tables=synth_tables("ct", N, seed=3), seed=seed)
    return FleetVecNormalize(venv, clip_reward=10.0) if with_norm else venv


def stagger(env, raw):
    """Envs at different points of their episodes: three zero-action steps, a quarter of the envs reset (masked fleet_reset_dev) after
    each.  `raw` f32 [E, D] ends up holding every env's current raw observation."""
    venv = getattr(env, "venv", env)
    batch, E, N = venv.core.batch, venv.num_envs, venv.core.batch.N
    batch.use_torch_stream()
    venv._torch_stream = torch.cuda.current_stream(dev()).cuda_stream
    zeros = torch.zeros((E, N), device=dev())
    reward, done = torch.empty(E, device=dev(), dtype=torch.float64), torch.empty(E, device=dev(), dtype=torch.uint8)
    batch.reset_dev(raw.data_ptr())
    for j in range(3):
        batch.step_dev(zeros.data_ptr(), raw.data_ptr(), reward.data_ptr(), done.data_ptr())
        mask = (torch.arange(E, device=dev()) % 4 == j).to(torch.uint8)
        batch.reset_dev(raw.data_ptr(), mask.data_ptr())
    torch.cuda.synchronize()


def env_state(env):
    """The env's fleet_state_save blob, section by section, and the normaliser's state.  Of a rainflow row only the live words are
    state -- the 6 header words and the stack entries below the top one, which the header holds; the words beyond were never written
    and hold what the allocation held (include/fleet_hip.h fleet_fork_envs; tests/test_state_gpu.py) -- so those are blanked."""
    from fleetrl_amd import _capi

    batch = getattr(env, "venv", env).core.batch
    out = {"blob_" + k: np.array(v) for k, v in _capi.state_views(batch.save_state()).items()}
    if "blob_rf_rows" in out:
        rows, live = out["blob_rf_rows"].view(np.uint64), 6 + np.maximum(batch.get("rf_stack") - 1, 0)
        rows[np.arange(rows.shape[2])[None, None, :] >= live[:, :, None]] = 0
    if hasattr(env, "norm"):
        st = env.norm.get_state()
        out.update(obs_mean=st.obs_rms.mean, obs_var=st.obs_rms.var, obs_count=np.float64(st.obs_rms.count), ret_mean=np.float64(st.ret_rms.mean),
                   ret_var=np.float64(st.ret_rms.var), ret_count=np.float64(st.ret_rms.count), returns=st.returns)
    return out


def assert_same_dict(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert same(a[k], b[k]), (what, k)


def episode_fields(env):
    batch = getattr(env, "venv", env).core.batch
    return batch.get("last_ep_return"), batch.get("last_ep_len")


# ---- 1. the ring kernel on given arrays ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    """One env of one EV and a one-layer policy: what a collect handle needs to exist."""
    from fleetrl_amd import DevicePolicy

    env = make_env(1, 1, False)
    D = env.core.obs_dim
    rng = np.random.default_rng(5)
    pol = DevicePolicy(pm.random_layers(rng, (D, 1)), critic_layers=pm.random_layers(rng, (D, 1)), activation="tanh", output="clip")
    yield env, pol
    pol.close(), env.close()


def ring_bits(col):
    W = col.stats_window
    ret, length, count = np.zeros(W, np.float64), np.zeros(W, np.int32), C.c_uint64()
    col._check(col.lib.fleet_collect_episodes_read(col.h, ret.ctypes.data, length.ctypes.data, C.byref(count)))
    return ret, length, count.value


@pytest.mark.parametrize("W", [1, 7, 100])
@pytest.mark.parametrize("E", [1, 3, 64, 65, 1023, 1025, 2049])
def test_the_ring_kernel_places_given_episodes_as_the_model_does(tiny, E, W):
    from fleetrl_amd import DevicePPOCollect

    col = DevicePPOCollect(*tiny, stats_window=W)
    ring = cm.Ring(W)
    empty = host(col.finish(3, 4))
    assert np.isnan(empty[0]) and np.isnan(empty[1]) and empty[2:5].tolist() == [0.0, 0.0, 7.0] and not empty[5:].any()
    assert same(empty, ring.finish(3, 4))
    rng = np.random.default_rng(E * 1009 + W)
    none, every, one, exactly_w = np.zeros(E, bool), np.ones(E, bool), np.zeros(E, bool), np.zeros(E, bool)
    one[E // 2] = True
    exactly_w[rng.permutation(E)[:min(W, E)]] = True
    last = np.zeros(E, bool)
    last[E - 1] = True
    patterns = [none, one, every, exactly_w, every, none, last, every, one] + [rng.random(E) < p for p in (0.01, 0.5, 0.97)]
    for step, done in enumerate(patterns):
        ret, length = rng.standard_normal(E) * 1e3, rng.integers(1, 10 ** 6, E).astype(np.int32)
        col.episodes_dev(torch.from_numpy(done.astype(np.uint8)).to(dev()), torch.from_numpy(ret).to(dev()), torch.from_numpy(length).to(dev()))
        ring.step(done, ret, length)
        got = ring_bits(col)
        assert got[2] == ring.count and same(got[0], ring.ret) and same(got[1], ring.len), (E, W, step)
        if step % 4 == 3:
            assert same(host(col.finish(step, 1)), ring.finish(step, 1)), (E, W, step)
    r, n, count = col.episodes()
    want = ring.window()
    assert count == ring.count and same(r, want[0]) and same(n, want[1])
    assert same(host(col.finish(0, 0)), ring.finish(0, 0))
    assert ring.count > 3 * W or E < W  # the ring wrapped several times
    col.close()


# ---- 2. PPO: the one call against the pieces --------------------------------------------------------------------------------------------
class PpoRig:
    """An env (staggered), a two-head policy, a rollout buffer and the collect handle, identically initialised per shape."""

    def __init__(self, E, N, K, with_norm, W=100, heads=2):
        from fleetrl_amd import DevicePolicy, DevicePPOCollect, DeviceRolloutBuffer

        self.E, self.N, self.K, self.with_norm = E, N, K, with_norm
        self.env = make_env(E, N, with_norm)
        self.venv = getattr(self.env, "venv", self.env)
        self.D = D = self.venv.core.obs_dim
        rng = np.random.default_rng(E * 100 + N)
        actor, critic = pm.random_layers(rng, (D, 8, 8, N)), pm.random_layers(rng, (D, 8, 8, 1))
        self.pol = DevicePolicy(actor, critic_layers=critic if heads == 2 else None, activation="tanh", output="clip")
        self.log_std = torch.from_numpy((-0.5 + 0.1 * rng.standard_normal(N)).astype(F32)).to(dev())
        self.buf = DeviceRolloutBuffer(E, K, D, N, gamma=0.99, gae_lambda=0.95)
        self.col = DevicePPOCollect(self.env, self.pol, stats_window=W)
        raw = torch.empty((E, D), device=dev())
        stagger(self.env, raw)
        # the carry: the current observation (normalised by the normaliser's reset), episode_start = 1
        self.obs, self.start = self.col.carry_obs, self.col.carry_start
        if with_norm:
            self.env.norm.reset_torch(raw, out=self.obs)
        else:
            self.obs.copy_(raw)
        self.start.fill_(1)
        self.steps = 0
        self.model = cm.Ring(W)
        torch.cuda.synchronize()

    def result(self, stats, obs, start):
        b = self.buf
        out = {n: host(getattr(b, n)) for n in ("observations", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")}
        out.update(carry_obs=host(obs), carry_start=host(start), stats=host(stats), **env_state(self.env))
        return out

    def one_call(self):
        stats = self.col.collect(self.buf, self.log_std, seed=SEED, first_step=self.steps)
        self.steps += self.K
        assert self.buf.full and self.buf.pos == self.K
        return self.result(stats, self.col.carry_obs, self.col.carry_start)

    def step_by_step(self):
        """The loop of examples/ppo_device_train.py; the episode ring from the model fed with every step's done flags and the env's
        FLEET_F_LAST_EP_RETURN / FLEET_F_LAST_EP_LEN."""
        E, N, K, D = self.E, self.N, self.K, self.D
        buf, pol, env = self.buf, self.pol, self.env
        if self.steps == 0:  # (own tensors: the handle's are not this arm's to write)
            self.obs, self.start = self.obs.clone(), self.start.clone()
        carry_obs, carry_start = self.obs, self.start
        env_act, last_value = torch.empty((E, N), device=dev()), torch.empty((E, 1), device=dev())
        reward = torch.empty(E, device=dev(), dtype=torch.float64)
        buf.reset()
        obs, start = carry_obs, carry_start
        first = self.steps
        for t in range(K):
            row = buf.slot(t)
            pol.sample(obs, self.log_std, seed=SEED, step=self.steps, actions_out=row.actions, env_actions_out=env_act, log_prob_out=row.log_prob,
                       values_out=row.value)
            self.steps += 1
            nxt = buf.slot(t + 1) if t + 1 < K else None
            nobs, ndone = (nxt.obs, nxt.episode_start) if nxt else (carry_obs, carry_start)
            if nobs is obs:  # (K = 1: the carry buffers are still being read)
                obs, start = obs.clone(), start.clone()
            env.step_torch(env_act, obs_out=nobs, reward_out=reward, done_out=ndone)
            buf.add(obs, row.actions, reward, start, row.value, row.log_prob)
            self.model.step(host(ndone).astype(bool), *episode_fields(env))
            obs, start = nobs, ndone
        pol.act(obs, out=env_act, values_out=last_value)
        buf.compute_returns_and_advantage(last_value, start)
        stats = torch.from_numpy(self.model.finish(first, K)).to(dev())
        return self.result(stats, carry_obs, carry_start)

    def close(self):
        for h in (self.col, self.buf, self.pol, self.env):
            h.close()


@pytest.mark.parametrize("with_norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("K", [1, 2, 9])
@pytest.mark.parametrize("E,N", [(1, 1), (3, 2), (65, 5)])
def test_the_ppo_call_equals_the_pieces_called_step_by_step(E, N, K, with_norm):
    a, b = PpoRig(E, N, K, with_norm), PpoRig(E, N, K, with_norm)
    for call in range(2):  # the second call starts from the first one's carry
        got, want = a.one_call(), b.step_by_step()
        assert_same_dict(got, want, (E, N, K, with_norm, call))
        assert a.col.describe()["launches"] == cm.launches_ppo(K, with_norm) == (5 if with_norm else 4) * K + 3
    r, n, count = a.col.episodes()
    mr, mn = b.model.window()
    assert count == b.model.count and same(r, mr) and same(n, mn)
    if K == 9:  # 18 steps over episodes of 8: every env finished two, and not all in one step
        assert count == 2 * E and np.array_equal(n, np.full(min(count, 100), 8 * 1, np.int32))
        starts = got["episode_starts"]
        assert E == 1 or len({tuple(np.flatnonzero(starts[:, e])) for e in range(E)}) > 1
    a.col.check_errors()
    a.close(), b.close()


def test_reset_is_the_envs_and_the_normalisers_reset_and_clears_the_ring_only_when_asked():
    a, b = PpoRig(3, 2, 9, True), PpoRig(3, 2, 9, True)
    a.one_call()
    assert a.col.episodes()[2] > 0
    a.col.reset()
    obs = torch.empty((3, a.D), device=dev())
    b.step_by_step()
    b.env.reset_torch(obs_out=obs)
    assert a.col.describe()["cur"] == 0 and a.col.describe()["launches"] == 3
    assert same(host(a.col.carry_obs), host(obs)) and host(a.col.carry_start).tolist() == [1, 1, 1]
    assert_same_dict(env_state(a.env), env_state(b.env), "reset")
    kept = a.col.episodes()
    assert kept[2] == b.model.count
    a.col.reset(clear_episodes=True)
    assert a.col.episodes()[2] == 0 and np.isnan(host(a.col.finish())[:2]).all()
    a.close(), b.close()


# ---- 3. TD3: the one call against the pieces ------------------------------------------------------------------------------------------
SIGMA, LEARNING_STARTS = 0.1, 3


def make_noise(kind, E, N):
    from fleetrl_amd import DeviceOUNoise, DevicePinkNoise

    if kind == "pink":
        return DevicePinkNoise(E, N, 4 * EP_HOURS, seed=SEED)  # seq_len = the episode's steps
    if kind == "ou":
        return DeviceOUNoise(E, N, sigma=0.2, seed=SEED)
    return None


class Td3Rig:
    def __init__(self, E, N, with_norm, noise, R=16):
        from fleetrl_amd import DevicePolicy, DeviceReplayBuffer, DeviceTD3Collect

        self.E, self.N, self.with_norm = E, N, with_norm
        self.env = make_env(E, N, with_norm)
        self.venv = getattr(self.env, "venv", self.env)
        self.D = D = self.venv.core.obs_dim
        rng = np.random.default_rng(E * 100 + N + 7)
        self.pol = DevicePolicy(pm.random_layers(rng, (D, 8, 8, N)), activation="relu", output="tanh")
        self.buf = DeviceReplayBuffer(R * E, E, D, N, seed=3)
        self.noise = make_noise(noise, E, N)
        self.col = DeviceTD3Collect(self.env, self.pol, stats_window=7)
        self.raw = self.col.raw_obs
        stagger(self.env, self.raw)
        self.obs, self.done = self.col.carry_obs, self.col.carry_start
        if with_norm:
            self.env.norm.reset_torch(self.raw, out=self.obs)
        self.done.zero_()
        self.steps = 0
        self.model = cm.Ring(7)
        torch.cuda.synchronize()

    def result(self, stats):
        b = self.buf
        out = {n: host(getattr(b, n)) for n in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")}
        out.update(pos=np.int64(b.pos), full=np.int64(b.full), stats=host(stats), **env_state(self.env))
        if self.noise is not None:
            out.update({"noise_" + k: (host(v) if isinstance(v, torch.Tensor) else np.int64(v)) for k, v in self.noise.state_dict().items() if k != "kind"})
        return out

    def one_call(self, n_steps):
        stats = self.col.collect(self.buf, n_steps, learning_starts=LEARNING_STARTS, sigma=SIGMA, noise=self.noise, seed=SEED, first_step=self.steps)
        self.steps += n_steps
        out = self.result(stats)
        out.update(carry_obs=host(self.col.carry_obs), carry_done=host(self.col.carry_start), raw_obs=host(self.col.raw_obs))
        return out

    def step_by_step(self, n_steps):
        """The loop of examples/td3_pink_noise.py (white noise: examples/td3_device_explore.py's `explore` with seed and step)."""
        E, N, D = self.E, self.N, self.D
        pol, env, buf = self.pol, self.env, self.buf
        if self.steps == 0:
            self.obs, self.done, self.raw = self.obs.clone(), self.done.clone(), self.raw.clone()
        obs, done, last_raw = self.obs, self.done, self.raw
        act, reward, terminal = torch.empty((E, N), device=dev()), torch.empty(E, device=dev(), dtype=torch.float64), torch.empty((E, D), device=dev())
        first = self.steps
        for _ in range(n_steps):
            s = self.steps
            if s < LEARNING_STARTS:
                pol.sample_uniform(E, seed=SEED, step=s, actions_out=act, env_actions_out=act)
            elif self.noise is not None:
                pol.explore(obs, SIGMA, action_noise=self.noise, done=done, actions_out=act, env_actions_out=act)
            else:
                pol.explore(obs, SIGMA, seed=SEED, step=s, actions_out=act, env_actions_out=act)
            if self.with_norm:
                env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
                raw = env.original_torch()
                buf.add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
                last_raw.copy_(raw.obs)
            else:
                nobs = torch.empty_like(obs)
                env.step_torch(act, obs_out=nobs, reward_out=reward, done_out=done, terminal_out=terminal)
                buf.add(obs, nobs, act, reward, done, terminal=terminal)
                obs.copy_(nobs)
                last_raw.copy_(nobs)
            self.model.step(host(done).astype(bool), *episode_fields(env))
            self.steps += 1
        out = self.result(torch.from_numpy(self.model.finish(first, n_steps)).to(dev()))
        out.update(carry_obs=host(obs), carry_done=host(done), raw_obs=host(last_raw))
        return out

    def close(self):
        for h in (self.col, self.noise, self.buf, self.pol, self.env):
            if h is not None:
                h.close()


@pytest.mark.parametrize("noise,with_norm", [("white", True), ("pink", True), ("ou", True), ("white", False), ("pink", False)])
@pytest.mark.parametrize("E,N", [(1, 1), (3, 2), (65, 5)])
def test_the_td3_call_equals_the_pieces_called_step_by_step(E, N, noise, with_norm):
    a, b = Td3Rig(E, N, with_norm, noise), Td3Rig(E, N, with_norm, noise)
    for call, n_steps in enumerate((5, 1, 12)):  # the first call straddles learning_starts; the ring of 16 rows wraps in the third
        got, want = a.one_call(n_steps), b.step_by_step(n_steps)
        assert_same_dict(got, want, (E, N, noise, with_norm, call))
        first = a.steps - n_steps
        assert a.col.describe()["launches"] == cm.launches_offpolicy(n_steps, with_norm, first, LEARNING_STARTS, noise != "white")
    assert got["full"] == 1 and got["pos"] == 2 and b.model.count == 2 * E
    r, n, count = a.col.episodes()
    mr, mn = b.model.window()
    assert count == b.model.count and same(r, mr) and same(n, mn)
    a.col.check_errors()
    a.close(), b.close()


# ---- 4. purity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["white", "pink"])
def test_a_call_of_k_steps_equals_two_of_half_on_any_stream(noise):
    a, b, c = (Td3Rig(65, 5, True, noise) for _ in range(3))
    whole = a.one_call(10)
    b.one_call(5)
    halves = b.one_call(5)
    other = torch.cuda.Stream(dev())
    with torch.cuda.stream(other):
        c.one_call(4)
        moved = c.one_call(6)
        other.synchronize()
    for got, what in ((halves, "two calls"), (moved, "another stream")):
        for k in whole:
            if k != "stats":
                assert same(whole[k], got[k]), (what, k)
        assert same(whole["stats"][[0, 1, 3, 4]], got["stats"][[0, 1, 3, 4]]), what  # ([2] counts the episodes of the CALL)
    for rig in (a, b, c):
        rig.close()


def test_a_ppo_result_does_not_depend_on_the_stream_or_on_the_ring():
    a, b = PpoRig(65, 5, 9, True, W=100), PpoRig(65, 5, 9, True, W=3)
    want = a.one_call()
    other = torch.cuda.Stream(dev())
    with torch.cuda.stream(other):
        got = b.one_call()
        other.synchronize()
    for k in want:
        if k != "stats":
            assert same(want[k], got[k]), k
    assert want["stats"][2] == got["stats"][2] == want["stats"][3] and got["stats"][4] == 9
    a.close(), b.close()


# ---- 6. refusals that need handles --------------------------------------------------------------------------------------------------
def ppo_args(rig, buf=None, n_steps=None):
    from fleetrl_amd import _capi

    buf = buf or rig.buf
    a = _capi.FleetCollectPpoArgs()
    a.n_steps, a.buffer, a.log_std = (buf.n_steps if n_steps is None else n_steps), buf.h.value, rig.log_std.data_ptr()
    a.seed, a.first_step = SEED, 0
    rig.stats = torch.zeros(16, device=dev(), dtype=torch.float64)
    a.stats = rig.stats.data_ptr()
    return a


def test_the_run_calls_refuse_what_needs_the_handles_and_launch_nothing_then():
    from fleetrl_amd import DevicePPOCollect, DeviceReplayBuffer, DeviceRolloutBuffer, DeviceTD3Collect, FleetHipError, _capi

    rig = PpoRig(3, 2, 2, True)
    rig.col.use_torch_stream()
    rig.buf.use_torch_stream()
    E, D, N = 3, rig.D, 2
    rig.buf.observations.fill_(7.0)
    rig.buf.rewards.fill_(-3.0)
    batch = rig.venv.core.batch
    before = {"obs": host(rig.buf.observations), "rew": host(rig.buf.rewards), "episodes": batch.get("episodes"), "ep_len": batch.get("ep_len"),
              "carry": host(rig.col.carry_obs), "norm": env_state(rig.env)["obs_count"], "cur": rig.col.describe()["cur"]}

    def refused(fn, word):
        with pytest.raises(FleetHipError) as err:
            fn()
        assert err.value.status == _capi.ERR_INVALID and word in str(err.value), str(err.value)
        torch.cuda.synchronize()
        assert same(host(rig.buf.observations), before["obs"]) and same(host(rig.buf.rewards), before["rew"])
        assert same(batch.get("episodes"), before["episodes"]) and same(batch.get("ep_len"), before["ep_len"])
        assert same(host(rig.col.carry_obs), before["carry"]) and env_state(rig.env)["obs_count"] == before["norm"]
        assert rig.col.describe()["cur"] == before["cur"] and not rig.stats.any()

    others = {"num_envs": DeviceRolloutBuffer(E + 1, 2, D, N), "obs_dim": DeviceRolloutBuffer(E, 2, D + 1, N), "act_dim": DeviceRolloutBuffer(E, 2, D, N + 1)}
    for what, buf in others.items():
        buf.use_torch_stream()
        refused(lambda: rig.col.collect_dev(ppo_args(rig, buf)), f"fleet_collect_ppo_dev: the rollout buffer's {what} is")
    refused(lambda: rig.col.collect_dev(ppo_args(rig, n_steps=3)), "fleet_collect_ppo_dev: n_steps must be the rollout buffer's 2, got 3")
    # handles on different streams: the buffer, the policy, the normaliser
    side = torch.cuda.Stream(dev())
    for h, word in ((rig.buf, "the rollout buffer launches on another stream than the env"), (rig.pol, "the policy launches on another stream than the env"),
                    (rig.env.norm, "the normaliser launches on another stream than the env")):
        h.set_stream(side.cuda_stream)
        refused(lambda: rig.col.collect_dev(ppo_args(rig)), "fleet_collect_ppo_dev: " + word)
        h.use_torch_stream()
    # a one-head policy: the words of fleet_explore_act_dev
    one = PpoRig(3, 2, 2, True, heads=1)
    one.col.use_torch_stream(), one.buf.use_torch_stream()
    one_len = one.venv.core.batch.get("ep_len")
    with pytest.raises(FleetHipError) as err:
        one.col.collect_dev(ppo_args(one))
    assert "fleet_collect_ppo_dev: values asked of a policy without a critic head" in str(err.value)
    assert not one.stats.any() and same(one.venv.core.batch.get("ep_len"), one_len)
    # the off-policy call: a replay buffer and a noise process of other shapes, a noise process on another stream
    td3 = Td3Rig(3, 2, True, "ou")
    td3.col.use_torch_stream(), td3.buf.use_torch_stream(), td3.noise.use_torch_stream()
    stats = torch.zeros(16, device=dev(), dtype=torch.float64)

    def off_args(replay=None, noise=None):
        a = _capi.FleetCollectOffpolicyArgs()
        a.n_steps, a.learning_starts, a.replay = 2, 0, (replay or td3.buf).h.value
        a.sigma, a.noise_lo, a.noise_hi, a.noise = rig.log_std.data_ptr(), -1.0, 1.0, (noise or td3.noise).h.value
        a.seed, a.first_step, a.stats = SEED, 0, stats.data_ptr()
        return a

    ep_len = td3.venv.core.batch.get("ep_len")
    bad_replay, bad_noise = DeviceReplayBuffer(64, E, D + 2, N), make_noise("ou", E + 1, N)
    bad_replay.use_torch_stream(), bad_noise.use_torch_stream()
    for args, word in ((off_args(replay=bad_replay), "the replay buffer's obs_dim is"), (off_args(noise=bad_noise), "the noise handle was made for 4 envs x 2 actions")):
        with pytest.raises(FleetHipError) as err:
            td3.col.collect_dev(args)
        assert "fleet_collect_offpolicy_dev: " + word in str(err.value)
    td3.noise.set_stream(side.cuda_stream)
    with pytest.raises(FleetHipError) as err:
        td3.col.collect_dev(off_args())
    assert "fleet_collect_offpolicy_dev: the noise handle launches on another stream than the env" in str(err.value)
    td3.noise.use_torch_stream()
    torch.cuda.synchronize()
    assert td3.buf.pos == 0 and not stats.any() and same(td3.venv.core.batch.get("ep_len"), ep_len) and td3.noise.state_dict()["calls"] == 0
    # create: an env without auto_reset (gymnasium.Env semantics: FleetEnv's core), shapes that disagree, the window
    from bench import bench_config

    from fleetrl_amd import DevicePolicy
    from fleetrl_amd.synth import synth_tables
    from fleetrl_amd.vec_env import FleetCore

    core = FleetCore(dict(bench_config(3, N, "ct"), episode_length=EP_HOURS), 3, tables=synth_tables("ct", N, seed=3), auto_reset=False, seed=1)
    h, p = C.c_void_p(), _capi.FleetCollectParams(C.sizeof(_capi.FleetCollectParams), 100)
    lib = _capi.load_library()
    assert lib.fleet_collect_create(core.batch.h, None, rig.pol.h, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
    assert lib.fleet_collect_last_error(None).decode().startswith("fleet_collect_create: the env needs auto_reset = 1")
    core.close()

    wrong = DevicePolicy(pm.random_layers(np.random.default_rng(1), (D, 4, N + 1)), activation="relu", output="tanh")
    with pytest.raises(FleetHipError) as err:
        DeviceTD3Collect(rig.env, wrong)
    assert "fleet_collect_create: the policy's act_dim is 3, the env's 2" in str(err.value)
    with pytest.raises(FleetHipError) as err:
        DevicePPOCollect(one.venv, one.pol, stats_window=5000)
    assert "fleet_collect_create: stats_window must be in 1..4096, got 5000" in str(err.value)
    for h in (wrong, bad_replay, bad_noise, *others.values()):
        h.close()
    td3.close(), one.close(), rig.close()


# ---- 7. the examples ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script,args", [("ppo_device_collect.py", ["--iterations", "2", "--envs", "8", "--evs", "2", "--steps", "5", "--batch-size", "16", "--epochs", "1"]),
                                         ("td3_device_collect.py", ["--iterations", "3", "--envs", "8", "--evs", "2", "--train-freq", "4", "--learning-starts", "6",
                                                                    "--batch-size", "16", "--buffer-size", "256", "--log-interval", "1"])])
def test_the_examples_run_at_small_sizes_and_print_finite_statistics(script, args):
    root = cm.ROOT
    out = subprocess.run([sys.executable, os.path.join(root, "examples", script), *args, "--episode-hours", "1"], capture_output=True, text=True,
                         cwd=root, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == int(args[1])
    last = lines[-1]
    assert last["rollout/total_episodes"] > 0 and np.isfinite(last["rollout/ep_rew_mean"]) and last["rollout/ep_len_mean"] == 4.0
    assert all(np.isfinite(v) for k, v in last.items() if k.startswith("train/") and v is not None)
