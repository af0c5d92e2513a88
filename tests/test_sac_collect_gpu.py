"""SAC's collector on the device (include/fleet_hip_sac_loop.h, fleet_collect.hip): the uniform draw on a networks handle against the
policy's bit for bit, the one call against the pieces run step by step (the Python loop over sample_uniform / act, step_torch and add)
bit for bit, what a result may not depend on, the launch counts, the refusals that need handles, and the example.  Everything is bit
equality: no tolerance."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_model as pm
import sac_loop_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from sac_loop_rig import SEED, assert_same_dict, dev, env_state, episode_fields, host, make_env, sac_layers, same, stagger  # noqa: E402

F32 = np.float32
LEARNING_STARTS, W, R = 3, 7, 16


# ---- 1. the uniform draw against the existing path ------------------------------------------------------------------------------------
def uniform_pair(A, D=3):
    from fleetrl_amd import DevicePolicy, DeviceSACNetworks

    rng = np.random.default_rng(A)
    pol = DevicePolicy(pm.random_layers(rng, (D, A)), activation="tanh", output="clip")
    nets = DeviceSACNetworks(pm.random_layers(rng, (D, 2 * A)), [pm.random_layers(rng, (D + A, 1))], activation="relu")
    return pol, nets


@pytest.mark.parametrize("E", [1, 65])
@pytest.mark.parametrize("A", [1, 2, 5, 7])  # a Philox block of 4 columns that is partly used
def test_the_uniform_draw_is_the_policys_bit_for_bit(A, E):
    pol, nets = uniform_pair(A)
    for low, high in ((-1.0, 1.0), (0.25, 0.25), (-3.0, 0.5)):
        for step, offset in ((0, 0), (2 ** 32 + 5, 7)):
            want = pol.sample_uniform(E, low=low, high=high, seed=SEED, step=step, env_id_offset=offset)[0]
            got = nets.sample_uniform(E, low=low, high=high, seed=SEED, step=step, env_id_offset=offset)
            assert got.shape == (E, A) and same(host(got), host(want)), (A, E, low, high, step)
            g = host(got)
            assert (g >= low).all() and ((g < high).all() if low < high else (g == low).all())
    # defaults, an output of the caller's, and a key that matters
    out = torch.full((E, A), 9.0, device=dev())
    assert nets.sample_uniform(E, seed=SEED, step=3, actions_out=out) is out
    assert same(host(out), host(pol.sample_uniform(E, seed=SEED, step=3)[0]))
    assert not same(host(out), host(nets.sample_uniform(E, seed=SEED, step=4)))
    assert not same(host(out), host(nets.sample_uniform(E, seed=SEED + 1, step=3)))
    pol.close(), nets.close()


def test_the_uniform_draw_strides_past_the_capped_grid():
    """E = 262145, A = 16: 1 048 580 work items of 4 columns, 4 more than the capped grid of 4096 x 256 threads covers in one pass."""
    E, A = 262145, 16
    assert E * (A // 4) == 4096 * 256 + 4
    pol, nets = uniform_pair(A)
    want = pol.sample_uniform(E, low=-3.0, high=0.5, seed=SEED, step=11)[0]
    got = nets.sample_uniform(E, low=-3.0, high=0.5, seed=SEED, step=11)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    tail = host(got[-2:])
    assert (tail >= -3.0).all() and (tail < 0.5).all() and len(np.unique(tail)) > 16  # the last rows were written
    pol.close(), nets.close()


# ---- 2. the one call against the pieces --------------------------------------------------------------------------------------------------
class SacRig:
    """An env (staggered), a SAC agent, a replay ring of 16 rows and the collect handle, identically initialised per shape."""

    def __init__(self, E, N, with_norm, seed=SEED):
        from fleetrl_amd import DeviceReplayBuffer, DeviceSACCollect, DeviceSACNetworks

        self.E, self.N, self.with_norm, self.seed = E, N, with_norm, seed
        self.env = make_env(E, N, with_norm)
        self.venv = getattr(self.env, "venv", self.env)
        self.D = D = self.venv.core.obs_dim
        actor, critics = sac_layers(D, N)
        self.nets = DeviceSACNetworks(actor, critics, activation="relu")
        self.buf = DeviceReplayBuffer(R * E, E, D, N, seed=3)
        self.col = DeviceSACCollect(self.env, self.nets, stats_window=W)
        self.raw = self.col.raw_obs
        stagger(self.env, self.raw)
        self.obs, self.done = self.col.carry_obs, self.col.carry_start
        if with_norm:
            self.env.norm.reset_torch(self.raw, out=self.obs)
        self.done.zero_()
        self.steps = 0
        self.model = sm.Ring(W)
        torch.cuda.synchronize()

    def ring(self):
        ret, length, count = np.zeros(W, np.float64), np.zeros(W, np.int32), C.c_uint64()
        self.col._check(self.col.lib.fleet_collect_episodes_read(self.col.h, ret.ctypes.data, length.ctypes.data, C.byref(count)))
        return ret, length, count.value

    def result(self, stats):
        b = self.buf
        out = {n: host(getattr(b, n)) for n in ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")}
        out.update(pos=np.int64(b.pos), full=np.int64(b.full), stats=host(stats), **env_state(self.env))
        return out

    def one_call(self, n_steps):
        stats = self.col.collect(self.buf, n_steps, learning_starts=LEARNING_STARTS, seed=self.seed, first_step=self.steps)
        self.steps += n_steps
        out = self.result(stats)
        ret, length, count = self.ring()
        out.update(carry_obs=host(self.col.carry_obs), carry_start=host(self.col.carry_start), raw_obs=host(self.col.raw_obs), ring_return=ret,
                   ring_length=length, ring_count=np.int64(count))
        return out

    def step_by_step(self, n_steps):
        """The Python loop a SAC agent ran before (examples/sac_device_train.py): sample_uniform or act, step_torch, add; the episode ring
        from the model fed with every step's done flags and the env's FLEET_F_LAST_EP_RETURN / FLEET_F_LAST_EP_LEN."""
        E, N, D = self.E, self.N, self.D
        nets, env, buf = self.nets, self.env, self.buf
        if self.steps == 0:  # (own tensors: the handle's are not this arm's to write)
            self.obs, self.done, self.raw = self.obs.clone(), self.done.clone(), self.raw.clone()
        obs, done, last_raw = self.obs, self.done, self.raw
        act, reward, terminal = torch.empty((E, N), device=dev()), torch.empty(E, device=dev(), dtype=torch.float64), torch.empty((E, D), device=dev())
        first = self.steps
        for _ in range(n_steps):
            s = self.steps
            if sm.warm_up(s, LEARNING_STARTS):
                nets.sample_uniform(E, seed=self.seed, step=s, actions_out=act)
            else:
                nets.act(obs, seed=self.seed, step=s, actions_out=act)
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
        out.update(carry_obs=host(obs), carry_start=host(done), raw_obs=host(last_raw), ring_return=self.model.ret.copy(),
                   ring_length=self.model.len.copy(), ring_count=np.int64(self.model.count))
        return out

    def close(self):
        for h in (self.col, self.buf, self.nets, self.env):
            h.close()


@pytest.mark.parametrize("with_norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("E,N", [(1, 1), (3, 2), (65, 5)])
def test_the_sac_call_equals_the_pieces_called_step_by_step(E, N, with_norm):
    a, b = SacRig(E, N, with_norm), SacRig(E, N, with_norm)
    for call, n_steps in enumerate((5, 1, 12)):  # the first call straddles learning_starts; the ring of 16 rows wraps in the third
        got, want = a.one_call(n_steps), b.step_by_step(n_steps)
        assert_same_dict(got, want, (E, N, with_norm, call))
        assert a.col.describe()["launches"] == sm.launches_collect(n_steps, with_norm) == (5 if with_norm else 4) * n_steps + 1
    assert got["full"] == 1 and got["pos"] == 2
    assert b.model.count >= 2 * E and got["ring_count"] == b.model.count  # the ring comparison above was not of empty rings
    r, n, count = a.col.episodes()
    mr, mn = b.model.window()
    assert count == b.model.count and same(r, mr) and same(n, mn)
    # the warm-up rows hold uniform draws, the rows behind them squashed samples: both inside (-1, 1), and not one repeated
    actions = got["actions"].reshape(R, E, N)
    assert (np.abs(actions) <= 1.0).all() and len(np.unique(actions)) > min(R * E * N // 2, 8)
    a.col.check_errors()
    a.close(), b.close()


# ---- 3. purity ----------------------------------------------------------------------------------------------------------------------
def test_a_call_of_ten_steps_equals_two_of_five_on_any_stream_and_the_seed_matters():
    a, b, c, d = (SacRig(65, 5, True) for _ in range(4))
    whole = a.one_call(10)
    again = d.one_call(10)
    assert_same_dict(whole, again, "identical states")
    b.one_call(5)
    halves = b.one_call(5)
    other = torch.cuda.Stream(dev())
    with torch.cuda.stream(other):
        c.one_call(5)
        moved = c.one_call(5)
        other.synchronize()
    for got, what in ((halves, "two calls"), (moved, "another stream")):
        for k in whole:
            if k != "stats":
                assert same(whole[k], got[k]), (what, k)
        assert same(whole["stats"][[0, 1, 3, 4]], got["stats"][[0, 1, 3, 4]]), what  # ([2] counts the episodes of the CALL)
    e = SacRig(65, 5, True, seed=SEED ^ 0x5555)
    seeded = e.one_call(10)
    x, y = whole["actions"].reshape(R, 65, 5), seeded["actions"].reshape(R, 65, 5)
    for t in range(10):  # rows 0..2 are the warm-up's, rows 3..9 the actor's: another seed gives other actions in every one
        assert not same(x[t], y[t]), t
    assert same(x[10:], y[10:])  # (rows nobody wrote)
    for rig in (a, b, c, d, e):
        rig.close()


# ---- 4. refusals that need handles ------------------------------------------------------------------------------------------------------
def test_the_calls_refuse_what_needs_the_handles_and_launch_nothing_then():
    from fleetrl_amd import (DevicePolicy, DeviceReplayBuffer, DeviceRolloutBuffer, DeviceSACCollect, DeviceTD3Collect, DeviceTD3Target, FleetHipError,
                             _capi)

    rig = SacRig(3, 2, True)
    E, D, N = 3, rig.D, 2
    rig.one_call(2)
    lib = _capi.load_library()
    stats = torch.zeros(16, device=dev(), dtype=torch.float64)
    batch = rig.venv.core.batch

    def sac_args(replay=None):
        a = _capi.FleetSacCollectArgs()
        a.n_steps, a.learning_starts, a.replay = 2, 0, (replay or rig.buf).h.value
        a.noise_lo, a.noise_hi, a.seed, a.first_step, a.stats = -1.0, 1.0, SEED, 2, stats.data_ptr()
        return a

    def refused(col, buf, fn, word):
        before = (col.describe()["launches"], col.describe()["cur"], buf.pos, batch.get("ep_len"), env_state(rig.env)["obs_count"])
        with pytest.raises(FleetHipError) as err:
            fn()
        assert err.value.status == _capi.ERR_INVALID and word in str(err.value), str(err.value)
        torch.cuda.synchronize()
        after = (col.describe()["launches"], col.describe()["cur"], buf.pos, batch.get("ep_len"), env_state(rig.env)["obs_count"])
        assert before[:3] == after[:3] and same(before[3], after[3]) and before[4] == after[4] and not stats.any(), word
        assert before[0] > 0

    # a policy-made handle given to the SAC run call
    pol = DevicePolicy(pm.random_layers(np.random.default_rng(1), (D, 8, N)), activation="relu", output="tanh")
    td3 = DeviceTD3Collect(rig.env, pol, stats_window=W)
    td3.collect(rig.buf, 1, learning_starts=0, sigma=0.1, seed=SEED, first_step=2)
    stats.zero_()
    refused(td3, rig.buf, lambda: td3._check(lib.fleet_saccollect_sac_dev(td3.h, C.byref(_sized(sac_args())))),
            "fleet_saccollect_sac_dev: the handle borrows a policy (fleet_collect_create)")
    # a SAC-made handle given to the PPO call and to the off-policy call: each names the entry that serves it
    rollout = DeviceRolloutBuffer(E, 2, D, N)
    rollout.use_torch_stream()
    sigma = torch.full((N,), 0.1, device=dev())
    ppo = _capi.FleetCollectPpoArgs()
    ppo.n_steps, ppo.buffer, ppo.log_std, ppo.seed, ppo.stats = 2, rollout.h.value, sigma.data_ptr(), SEED, stats.data_ptr()
    off = _capi.FleetCollectOffpolicyArgs()
    off.n_steps, off.replay, off.sigma, off.noise_lo, off.noise_hi, off.seed, off.stats = 2, rig.buf.h.value, sigma.data_ptr(), -1.0, 1.0, SEED, stats.data_ptr()
    refused(rig.col, rig.buf, lambda: rig.col._check(lib.fleet_collect_ppo_dev(rig.col.h, C.byref(_sized(ppo)))),
            "fleet_collect_ppo_dev: the handle borrows SAC networks (fleet_saccollect_create): fleet_saccollect_sac_dev runs it")
    refused(rig.col, rig.buf, lambda: rig.col._check(lib.fleet_collect_offpolicy_dev(rig.col.h, C.byref(_sized(off)))),
            "fleet_collect_offpolicy_dev: the handle borrows SAC networks (fleet_saccollect_create): fleet_saccollect_sac_dev runs it")
    # a replay buffer of another shape; networks on another stream
    bad_replay = DeviceReplayBuffer(64, E, D + 2, N)
    bad_replay.use_torch_stream()
    refused(rig.col, rig.buf, lambda: rig.col.collect_dev(sac_args(bad_replay)), "fleet_saccollect_sac_dev: the replay buffer's obs_dim is")
    side = torch.cuda.Stream(dev())
    rig.nets.set_stream(side.cuda_stream)
    refused(rig.col, rig.buf, lambda: rig.col.collect_dev(sac_args()),
            "fleet_saccollect_sac_dev: the networks launch on another stream than the env: fleet_qtarget_set_stream them to the env's first")
    rig.nets.use_torch_stream()
    # create: TD3 networks (not squashed), a wrong act_dim
    actor, critics = sac_layers(D, N)
    plain = DeviceTD3Target(pm.random_layers(np.random.default_rng(2), (D, 8, N)), [critics[0]], activation="relu", output="tanh")
    h, p = C.c_void_p(), _capi.FleetCollectParams(C.sizeof(_capi.FleetCollectParams), W)
    assert lib.fleet_saccollect_create(batch.h, rig.env.norm.h, plain.h, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
    assert lib.fleet_saccollect_last_error(None).decode() == ("fleet_saccollect_create: the networks' actor is not a squashed Gaussian: "
                                                              "fleet_sac_create makes one")
    assert lib.fleet_saccollect_create(batch.h, rig.env.norm.h, pol.h, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
    assert lib.fleet_saccollect_last_error(None).decode() == "fleet_saccollect_create: the handle is not a networks handle"
    from fleetrl_amd import DeviceSACNetworks

    wide = DeviceSACNetworks(*sac_layers(D, N + 1), activation="relu")
    with pytest.raises(FleetHipError) as err:
        DeviceSACCollect(rig.env, wide)
    assert f"fleet_saccollect_create: the networks' act_dim is {N + 1}, the env's {N}" in str(err.value)
    # ... and the uniform entry on networks fleet_sac_create did not make
    u = _capi.FleetSacUniformArgs()
    u.struct_bytes, u.lo, u.hi, u.seed, u.actions = C.sizeof(u), -1.0, 1.0, SEED, stats.data_ptr()
    assert lib.fleet_saccollect_uniform_dev(plain.h, 1, C.byref(u)) == _capi.ERR_INVALID
    assert lib.fleet_qtarget_last_error(plain.h).decode().startswith("fleet_saccollect_uniform_dev: the handle's actor is not a squashed Gaussian")
    torch.cuda.synchronize()
    assert not stats.any()
    # the handle still works after all of it
    rig.col.collect(rig.buf, 1, learning_starts=0, seed=SEED, first_step=3)
    rig.col.check_errors()
    for x in (td3, pol, rollout, bad_replay, plain, wide):
        x.close()
    rig.close()


def _sized(a):
    a.struct_bytes = C.sizeof(a)
    return a


# ---- 5. the example --------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_at_its_default_sizes_checks_itself_and_prints_finite_statistics():
    root = sm.ROOT
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "sac_device_collect.py"), "--check"], capture_output=True, text=True, cwd=root,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert lines and all(line["check"] == "bit-equal" for line in lines)
    last = lines[-1]
    assert last["rollout/total_episodes"] > 0 and np.isfinite(last["rollout/ep_rew_mean"]) and np.isfinite(last["rollout/ep_len_mean"])
    assert all(np.isfinite(v) for k, v in last.items() if k.startswith("train/") and v is not None)
    evals = [line for line in lines if "eval/mean_reward" in line]
    assert evals and all(np.isfinite(e["eval/mean_reward"]) for e in evals) and evals[0]["new_best"] is True
