"""The agent's evaluation on the device (fleet_eval.hip): the bookkeeping kernel on given arrays against tests/eval_model.py bit for bit,
the normaliser sync against the host's set_state, the one call against the existing pieces (sync_normalization, then evaluate_policy) bit
for bit, the Monitor source against a step-by-step loop, the snapshot and its gate, what a result may not depend on, the launch counts
and the refusals that need handles."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import eval_model as em
import policy_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
EP_HOURS = 2  # episodes of 8 steps
U = 2.0 ** -53


def dev():
    return torch.device("cuda", 0)


def host(t):
    return t.detach().cpu().numpy().copy()


def same(a, b) -> bool:
    """Bit equality of two arrays of one dtype and shape."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_env(E, N, with_norm, seed=1, **kw):
    from bench import bench_config

    from fleetrl_amd import FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    venv = FleetVecEnv(dict(bench_config(E, N, "ct"), episode_length=EP_HOURS), E, tables=synth_tables("ct", N, seed=3), seed=seed, **kw)
    return FleetVecNormalize(venv, clip_reward=10.0) if with_norm else venv


def env_state(env):
    """The env's fleet_state_save blob, section by section, and the normaliser's state.  Of a rainflow row only the live words are
    state -- the 6 header words and the stack entries below the top one, which the header holds; the words beyond were never written
    and hold what the allocation held (include/fleet_hip.h fleet_fork_envs) -- so those are blanked."""
    from fleetrl_amd import _capi

    batch = getattr(env, "venv", env).core.batch
    out = {"blob_" + k: np.array(v) for k, v in _capi.state_views(batch.save_state()).items()}
    if "blob_rf_rows" in out:
        rows, live = out["blob_rf_rows"].view(np.uint64), 6 + np.maximum(batch.get("rf_stack") - 1, 0)
        rows[np.arange(rows.shape[2])[None, None, :] >= live[:, :, None]] = 0
    if hasattr(env, "norm"):
        out.update(norm_state(env.norm))
    return out


def norm_state(norm):
    st = norm.get_state()
    return dict(obs_mean=st.obs_rms.mean, obs_var=st.obs_rms.var, obs_count=np.float64(st.obs_rms.count), ret_mean=np.float64(st.ret_rms.mean),
                ret_var=np.float64(st.ret_rms.var), ret_count=np.float64(st.ret_rms.count), returns=st.returns)


def assert_same_dict(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert same(a[k], b[k]), (what, k)


def trained_normalizer(D, seed, E=4, **settings):
    """A normaliser with statistics of its own: three training steps on random data."""
    from fleetrl_amd import DeviceNormalizer

    n = DeviceNormalizer(E, D, **settings)
    feed(n, seed, 3)
    return n


def feed(n, seed, steps):
    rng = np.random.default_rng(seed)
    n.use_torch_stream()
    out = None
    for _ in range(steps):
        raw = torch.from_numpy((rng.standard_normal((n.E, n.D)) * 3 + 1).astype(F32)).to(dev())
        rew = torch.from_numpy(rng.standard_normal(n.E) * 5).to(dev())
        done = torch.from_numpy((rng.random(n.E) < 0.3).astype(np.uint8)).to(dev())
        out = n.step_torch(raw, rew, done)
    torch.cuda.synchronize()
    return host(out[0]), host(out[1])


# ---- 1. the bookkeeping kernel on given arrays ---------------------------------------------------------------------------------------
MAX_E = 2049


@pytest.fixture(scope="module")
def wide():
    """2049 envs of one EV and a one-layer policy: what an evaluation handle with per-env arrays for every tested E needs to exist."""
    from fleetrl_amd import DeviceEvalCallback, DevicePolicy

    env = make_env(MAX_E, 1, False)
    D = env.core.obs_dim
    pol = DevicePolicy(pm.random_layers(np.random.default_rng(5), (D, 1)), activation="tanh", output="clip")
    cb = DeviceEvalCallback(pol, env, max_episodes=2 * MAX_E + 3)
    yield cb
    cb.close(), pol.close(), env.close()


def device_bookkeeping(cb, E):
    a = cb.arrays()
    torch.cuda.synchronize()
    return host(a["sums"])[:E], host(a["lengths"])[:E], host(a["counts"])[:E], host(a["ep_reward"]), host(a["ep_length"]), int(host(a["listed"])[0])


@pytest.mark.parametrize("monitor", [False, True], ids=["sums", "monitor"])
@pytest.mark.parametrize("E", [1, 3, 64, 65, 1023, 1025, 2049])
def test_the_bookkeeping_kernel_lists_given_episodes_as_the_model_does(wide, E, monitor):
    """12 hostile steps: nobody, one env, everybody, the last env, random patterns; the quotas are met early, in the middle, or never."""
    cb = wide
    for n_eval in sorted({n for n in (1, E - 1, E, 2 * E + 3) if n >= 1}):
        cb.clear()
        ev = em.Evaluation(E, cb.max_episodes)
        # (the model's lists start from the device's: slots a case does not reach keep what an earlier case left)
        ev.ep_reward[:], ev.ep_length[:] = host(cb.arrays()["ep_reward"]), host(cb.arrays()["ep_length"])
        rng = np.random.default_rng(E * 1009 + n_eval + 7 * monitor)
        none, every, one, last = np.zeros(E, bool), np.ones(E, bool), np.zeros(E, bool), np.zeros(E, bool)
        one[E // 2] = True
        last[E - 1] = True
        patterns = [none, one, every, last, rng.random(E) < 0.5, every, none, rng.random(E) < 0.97, one, rng.random(E) < 0.01, every, rng.random(E) < 0.5]
        assert len(patterns) == 12
        for step, done in enumerate(patterns):
            reward = rng.standard_normal(E) * 1e3
            ret, length = rng.standard_normal(E) * 1e3, rng.integers(1, 10 ** 6, E).astype(np.int32)
            to = lambda x: torch.from_numpy(x).to(dev())  # noqa: E731
            cb.episodes_dev(to(done.astype(np.uint8)), to(reward), to(ret) if monitor else None, to(length) if monitor else None, n_eval_episodes=n_eval,
                            monitor=monitor)
            ev.step(done, reward, n_eval, int(monitor), ret, length)
            sums, lengths, counts, ep_r, ep_n, listed = device_bookkeeping(cb, E)
            assert listed == ev.listed, (E, n_eval, step)
            assert same(sums, ev.sums) and same(lengths, ev.lengths) and same(counts, ev.counts), (E, n_eval, step)
            assert same(ep_r, ev.ep_reward) and same(ep_n, ev.ep_length), (E, n_eval, step)
        r, n = cb.episodes()
        assert same(r, ev.lists()[0]) and same(n, ev.lists()[1])
        if n_eval <= 3 * E:  # (three steps in which everybody finishes)
            assert ev.listed == n_eval and same(ev.counts, em.targets(n_eval, E).astype(np.int32))


# ---- 2. the normaliser sync --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other_stream", [False, True], ids=["one-stream", "src-elsewhere"])
@pytest.mark.parametrize("D", [1, 5, 257, 388])
def test_the_sync_copies_the_six_statistics_and_derives_what_set_state_derives(D, other_stream):
    from fleetrl_amd import DeviceNormalizer, _capi

    lib = _capi.load_library()
    side = torch.cuda.Stream(dev())
    src = DeviceNormalizer(4, D, epsilon=1e-8)
    if other_stream:
        with torch.cuda.stream(side):
            feed(src, D, 3)
            src.use_torch_stream()
            # (left unsynchronised work behind: one more step whose end the sync has to wait for)
            rng = np.random.default_rng(D + 1)
            raw = torch.from_numpy((rng.standard_normal((4, D)) * 2).astype(F32)).to(dev())
            rew, done = torch.from_numpy(rng.standard_normal(4)).to(dev()), torch.zeros(4, device=dev(), dtype=torch.uint8)
            src.step_torch(raw, rew, done)
    else:
        feed(src, D, 4)
    # two destinations with a history of their own (returns that are not zero) and another epsilon
    dst, ref = (trained_normalizer(D, 99, E=3, epsilon=1e-2, gamma=0.9) for _ in range(2))
    dst.use_torch_stream(), ref.use_torch_stream()
    before = norm_state(dst)
    assert before["returns"].any()
    assert lib.fleet_eval_sync_norm_dev(dst.h, src.h) == _capi.OK, lib.fleet_eval_last_error(None).decode()
    want = src.get_state()
    ref.set_state(obs_rms=want.obs_rms, ret_rms=want.ret_rms)
    got, src_state = norm_state(dst), norm_state(src)
    for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count"):
        assert same(got[k], src_state[k]), k
    assert same(got["returns"], before["returns"]) and dst.settings.epsilon == 1e-2
    assert not same(got["obs_mean"], before["obs_mean"])
    a, b = feed(dst, 7, 1), feed(ref, 7, 1)  # a step after the sync and one after the host's set_state of the same values
    assert same(a[0], b[0]) and same(a[1], b[1])
    assert_same_dict(norm_state(dst), norm_state(ref), "after a step")
    other = DeviceNormalizer(3, D + 1)
    assert lib.fleet_eval_sync_norm_dev(dst.h, other.h) == _capi.ERR_INVALID
    assert lib.fleet_eval_last_error(None).decode() == (f"fleet_eval_sync_norm_dev: the source normaliser has obs_dim {D + 1} on device 0, "
                                                        f"the destination {D} on device 0")
    for n in (src, dst, ref, other):
        n.close()


# ---- 3. the one call against the pieces ----------------------------------------------------------------------------------------------
class Rig:
    """An evaluation env, a policy, (with a normaliser) a trained training normaliser, and the callback; identically initialised per shape."""

    def __init__(self, E, N, with_norm, n_eval, monitor=False, max_episodes=None, **env_kw):
        from fleetrl_amd import DeviceEvalCallback, DevicePolicy

        self.E, self.N, self.with_norm, self.n_eval = E, N, with_norm, n_eval
        self.env = make_env(E, N, with_norm, **env_kw)
        self.venv = getattr(self.env, "venv", self.env)
        self.D = D = self.venv.core.obs_dim
        rng = np.random.default_rng(E * 100 + N)
        self.layers = pm.random_layers(rng, (D, 8, 8, N))
        self.pol = DevicePolicy(self.layers, activation="tanh", output="clip")
        self.train_norm = trained_normalizer(D, 11) if with_norm else None
        self.cb = DeviceEvalCallback(self.pol, self.env, n_eval_episodes=n_eval, monitor=monitor, train_normalizer=self.train_norm,
                                     max_episodes=max_episodes)
        torch.cuda.synchronize()

    def one_call(self, num_timesteps=1000):
        stats = self.cb.evaluate(num_timesteps)
        r, n = self.cb.episodes()
        return dict(rewards=r, lengths=n, stats=host(stats), **env_state(self.env))

    def pieces(self):
        """What a training loop does today: sync_normalization, then evaluate_policy."""
        from fleetrl_amd import evaluate_policy, sync_normalization

        if self.with_norm:
            st = self.train_norm.get_state()
            sync_normalization(types.SimpleNamespace(obs_rms=st.obs_rms, ret_rms=st.ret_rms), self.env)
        r, n = evaluate_policy(self.pol, self.env, n_eval_episodes=self.n_eval, return_episode_rewards=True)
        torch.cuda.synchronize()
        return dict(rewards=np.array(r, np.float64), lengths=np.array(n, np.int32), **env_state(self.env))

    def close(self):
        for h in (self.cb, self.pol, self.train_norm, self.env):
            if h is not None:
                h.close()


def check_stats(stats, rewards, lengths, num_timesteps, evaluations):
    """stats[0..4] are the model's bits; np.mean / np.std lie within the bounds tests/test_eval_cpu.py derives."""
    n = rewards.size
    want = np.array(em.mean_std(rewards) + em.mean_std(lengths.astype(np.float64)) + (np.float64(n),))
    assert same(stats[:5], want), (stats[:5], want)
    for x, mean, std in ((rewards, stats[0], stats[1]), (lengths.astype(np.float64), stats[2], stats[3])):
        tot, sd = float(np.sum(np.abs(x))), float(np.std(x))
        assert abs(mean - np.mean(x)) <= 2 * ((n - 1) * U * tot / n + U * abs(np.mean(x)))
        dm = U * (tot + abs(np.mean(x)))
        assert abs(std - sd) <= (2 * (sd * (n / 2 + 4) * U + dm * dm / sd) if sd > 0 else 0.0)
    assert stats[7] == num_timesteps and stats[8] == evaluations and not stats[9:].any()


@pytest.mark.parametrize("with_norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("n_eval", ["1", "5", "E+1", "2E+3"])
@pytest.mark.parametrize("E,N", [(1, 1), (3, 2), (65, 5)])
def test_the_one_call_equals_sync_normalization_and_evaluate_policy(E, N, n_eval, with_norm, tmp_path):
    n_eval ={"1": 1, "5": 5, "E+1": E + 1, "2E+3": 2 * E + 3}[n_eval]
    a, b = Rig(E, N, with_norm, n_eval), Rig(E, N, with_norm, n_eval)
    for call in range(2):  # (the second evaluation starts from the first one's env and normaliser)
        got, want = a.one_call(1000 + call), b.pieces()
        stats = got.pop("stats")
        assert got["rewards"].size == n_eval
        assert_same_dict(got, want, (E, N, n_eval, with_norm, call))
        check_stats(stats, got["rewards"], got["lengths"], 1000 + call, call + 1)
        assert stats[5] == max(stats[0], prev_best) if call else stats[5] == stats[0] and stats[6] == 1.0
        prev_best = stats[5]
        n_steps = -(-n_eval // E) * 8
        assert a.cb.n_steps() == n_steps and (got["lengths"] == 8).all()
        assert a.cb.describe()["launches"] == em.launches(n_steps, with_norm, with_norm) == (4 if with_norm else 3) * n_steps + (6 if with_norm else 4)
    res = a.cb.results()
    assert res["eval/mean_reward"] == stats[0] and res["eval/mean_ep_length"] == 8.0 and res["num_timesteps"] == 1001
    assert a.cb.evaluations_timesteps == [1001] and a.cb.evaluations_results == [got["rewards"].tolist()] and a.cb.evaluations_length == [[8] * n_eval]
    a.cb.save_npz(tmp_path / "evaluations.npz")  # SB3's keys and shapes: [evaluations], [evaluations, episodes] twice
    with np.load(tmp_path / "evaluations.npz") as z:
        assert sorted(z) == ["ep_lengths", "results", "timesteps"] and z["timesteps"].tolist() == [1001]
        assert same(z["results"], got["rewards"][None, :]) and z["ep_lengths"].tolist() == [[8] * n_eval]
    a.cb.check_errors()
    a.close(), b.close()


# ---- 4. the Monitor source -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,N,with_norm,n_eval", [(3, 2, True, 9), (65, 5, False, 5), (1, 1, False, 3)])
def test_the_monitor_source_lists_the_envs_own_episode_records(E, N, with_norm, n_eval):
    a, b = Rig(E, N, with_norm, n_eval, monitor=True), Rig(E, N, with_norm, n_eval, monitor=True)
    got = a.one_call()
    # the pieces step by step, the env's records read through fleet_get_dev after every step
    if with_norm:
        b.cb.sync_normalization()
    obs, act = torch.empty((E, b.D), device=dev()), torch.empty((E, N), device=dev())
    reward, done = torch.empty(E, device=dev(), dtype=torch.float64), torch.empty(E, device=dev(), dtype=torch.uint8)
    ret, length = torch.empty(E, device=dev(), dtype=torch.float64), torch.empty(E, device=dev(), dtype=torch.int32)
    ev = em.Evaluation(E, n_eval)
    if with_norm:
        b.env.reset_torch(obs_out=obs)
    else:
        b.venv.core.batch.use_torch_stream()
        b.venv._torch_stream = torch.cuda.current_stream(dev()).cuda_stream
        b.venv.core.batch.reset_dev(obs.data_ptr())
    for _ in range(b.cb.n_steps()):
        b.pol.act(obs, out=act)
        b.env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done)
        b.venv.core.batch.get_dev("last_ep_return", ret.data_ptr())
        b.venv.core.batch.get_dev("last_ep_len", length.data_ptr())
        r = host(reward) if with_norm else host(reward).astype(F32).astype(np.float64)
        ev.step(host(done).astype(bool), r, n_eval, 1, host(ret), host(length))
    want = dict(rewards=ev.lists()[0], lengths=ev.lists()[1], **env_state(b.env))
    stats = got.pop("stats")
    assert_same_dict(got, want, (E, N, with_norm))
    assert same(stats, ev.finish(1000)) and got["rewards"].size == n_eval and (got["lengths"] == 8).all()
    assert same(host(a.cb.arrays()["sums"]), ev.sums) and same(host(a.cb.arrays()["counts"]), ev.counts)
    a.close(), b.close()


# ---- 5. the snapshot ------------------------------------------------------------------------------------------------------------------
def constant_actor(D, N, value):
    """An actor whose deterministic action is `value` in every column, whatever it observes."""
    return [(np.zeros((8, D), F32), np.zeros(8, F32)), (np.zeros((N, 8), F32), np.full(N, value, F32))]


def test_the_snapshot_keeps_the_best_weights_and_only_those():
    from fleetrl_amd import DeviceEvalCallback, DevicePolicy, evaluate_policy

    E, N, n_eval = 3, 2, 5
    starts = np.array([[40, 136, 232]], np.int32)  # one scheduled start per env: every evaluation meets the same episodes
    env, twin = make_env(E, N, False, start_rows=starts), make_env(E, N, False, start_rows=starts)
    D = env.core.obs_dim
    # two agents that differ by construction: one charges every EV at full power whenever it can, one discharges it
    cand = {v: constant_actor(D, N, v) for v in (1.0, -1.0)}
    probe = DevicePolicy(cand[1.0], activation="tanh", output="clip")
    means = {}
    for v, layers in cand.items():
        probe.load_host(layers)
        means[v] = evaluate_policy(probe, twin, n_eval_episodes=n_eval)[0]  # (the existing path, on an env of its own)
    good = max(means, key=means.get)
    assert means[good] - means[-good] > 1e-6 * abs(means[good]), means
    A, B = cand[good], cand[-good]  # B is strictly worse
    pol, second = DevicePolicy(A, activation="tanh", output="clip"), DevicePolicy(pm.random_layers(np.random.default_rng(1), (D, 8, N)), activation="tanh", output="clip")
    cb = DeviceEvalCallback(pol, env, n_eval_episodes=n_eval, monitor=False)
    from fleetrl_amd import FleetHipError, _capi
    with pytest.raises(FleetHipError) as err:
        cb.load_best_into(second)
    assert err.value.status == _capi.ERR_STATE and "no evaluation has run" in str(err.value)
    # 1. A is a new best; the snapshot loaded into a second policy acts as A does
    s1 = host(cb.evaluate(10))
    # (evaluate_policy's np.mean adds in another order than S: equal to rounding, not to the bit)
    assert s1[6] == 1.0 and s1[5] == s1[0] and np.isclose(s1[0], means[good], rtol=1e-12, atol=0) and host(cb.arrays()["gate"])[0] == 1
    cb.load_best_into(second)
    obs = torch.from_numpy(np.random.default_rng(2).standard_normal((7, D)).astype(F32)).to(dev())
    probe.load_host(A)
    assert same(host(second.act(obs)), host(probe.act(obs)))
    snap = host(cb.arrays()["snapshot"])
    assert snap.any()
    # 2. B is worse: the gate stays shut, the snapshot's bits and the best stay
    pol.load_host(B)
    s2 = host(cb.evaluate(20))
    assert np.isclose(s2[0], means[-good], rtol=1e-12, atol=0) and s2[0] < s1[0] and s2[6] == 0.0 and s2[5] == s1[5] and host(cb.arrays()["gate"])[0] == 0
    assert same(host(cb.arrays()["snapshot"]), snap)
    # 3. A again: an equal mean is not a new best
    pol.load_host(A)
    s3 = host(cb.evaluate(30))
    assert s3[0] == s1[0] and s3[6] == 0.0 and s3[5] == s1[5] and s3[8] == 3 and same(host(cb.arrays()["snapshot"]), snap)
    # 4. the export is A's tensors, bit for bit; and the best goes back into the evaluated policy
    out = cb.best_parameters()
    flat = [t for w, b in A for t in (w, b)]
    assert len(out) == len(flat) and all(same(host(g), w) for g, w in zip(out, flat))
    pol.load_host(B)
    cb.load_best_into()
    assert same(host(pol.act(obs)), host(probe.act(obs)))
    res = cb.results()
    assert res["best_mean_reward"] == s1[0] and res["new_best"] is False and res["num_timesteps"] == 30
    for h in (cb, pol, second, probe, env, twin):
        h.close()


# ---- 6. purity -----------------------------------------------------------------------------------------------------------------------
def test_a_result_depends_on_the_state_alone_not_on_the_stream_or_on_max_episodes():
    E, N, n_eval = 65, 5, 70
    rigs = [Rig(E, N, True, n_eval), Rig(E, N, True, n_eval), Rig(E, N, True, n_eval), Rig(E, N, True, n_eval, max_episodes=4 * n_eval)]
    want = rigs[0].one_call()
    again = rigs[1].one_call()
    other = torch.cuda.Stream(dev())
    with torch.cuda.stream(other):
        moved = rigs[2].one_call()
        other.synchronize()
    longer = rigs[3].one_call()
    for got, what in ((again, "a second handle"), (moved, "another stream"), (longer, "a longer list")):
        assert_same_dict(want, got, what)
    for rig in rigs:
        rig.close()


# ---- 7. refusals that need handles ----------------------------------------------------------------------------------------------------
def test_the_calls_refuse_what_needs_the_handles_and_launch_nothing_then():
    from bench import bench_config

    from fleetrl_amd import DeviceEvalCallback, DeviceNormalizer, DevicePolicy, FleetHipError, _capi
    from fleetrl_amd.synth import synth_tables
    from fleetrl_amd.vec_env import FleetCore

    rig = Rig(3, 2, True, 5)
    cb, E, D, N = rig.cb, 3, rig.D, 2
    cb.use_torch_stream()
    batch = rig.venv.core.batch
    stats = torch.zeros(16, device=dev(), dtype=torch.float64)
    before = {"ep_len": batch.get("ep_len"), "episodes": batch.get("episodes"), "norm": norm_state(rig.env.norm)}

    def args(**kw):
        a = _capi.FleetEvalArgs()
        a.n_eval_episodes, a.n_steps, a.reward_source, a.stats = 5, 16, 0, stats.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(fn, word, status=_capi.ERR_INVALID):
        with pytest.raises(FleetHipError) as err:
            fn()
        assert err.value.status == status and word in str(err.value), str(err.value)
        torch.cuda.synchronize()
        assert same(batch.get("ep_len"), before["ep_len"]) and same(batch.get("episodes"), before["episodes"]) and not stats.any()
        assert_same_dict(norm_state(rig.env.norm), before["norm"], word)

    refused(lambda: cb.run_dev(args(n_eval_episodes=6)), "fleet_eval_run_dev: n_eval_episodes must be <= the handle's max_episodes 5, got 6")
    side = torch.cuda.Stream(dev())
    for h, word in ((rig.pol, "the policy launches on another stream than the env"), (rig.env.norm, "the normaliser launches on another stream than the env")):
        h.set_stream(side.cuda_stream)
        refused(lambda: cb.run_dev(args()), "fleet_eval_run_dev: " + word)
        h.use_torch_stream()
    other = DeviceNormalizer(3, D + 2)
    refused(lambda: cb.run_dev(args(sync_from=other.h.value)), f"fleet_eval_run_dev: the source normaliser has obs_dim {D + 2} on device 0")
    one = torch.zeros(4, device=dev(), dtype=torch.uint8)
    refused(lambda: cb.episodes_dev(one, torch.zeros(4, device=dev(), dtype=torch.float64), n_eval_episodes=5),
            "fleet_eval_episodes_dev: E must be <= the handle's num_envs 3, got 4")
    refused(lambda: cb.load_best_into(rig.pol), "fleet_eval_best_load_dev: no evaluation has run on this handle", _capi.ERR_STATE)
    refused(lambda: cb.best_parameters(), "fleet_eval_best_export_dev: no evaluation has run on this handle", _capi.ERR_STATE)
    wrong = DevicePolicy(pm.random_layers(np.random.default_rng(1), (D, 4, N)), activation="tanh", output="clip")
    wrong.use_torch_stream()
    refused(lambda: cb._check(cb.lib.fleet_eval_best_load_dev(cb.h, wrong.h)), "fleet_eval_best_load_dev: the destination policy's layout differs")
    # a handle without a normaliser takes no sync_from
    raw = Rig(3, 2, False, 5)
    raw.cb.use_torch_stream()
    with pytest.raises(FleetHipError) as err:
        raw.cb.run_dev(args(sync_from=other.h.value))
    assert "fleet_eval_run_dev: sync_from given to a handle without a normaliser" in str(err.value) and not stats.any()
    with pytest.raises(ValueError):
        DeviceEvalCallback(raw.pol, raw.env, train_normalizer=other)
    # create: an env without auto_reset, shapes that disagree, the lists' length
    core = FleetCore(dict(bench_config(3, N, "ct"), episode_length=EP_HOURS), 3, tables=synth_tables("ct", N, seed=3), auto_reset=False, seed=1)
    h, p = C.c_void_p(), _capi.FleetEvalParams(C.sizeof(_capi.FleetEvalParams), 5)
    lib = _capi.load_library()
    assert lib.fleet_eval_create(core.batch.h, None, rig.pol.h, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
    assert lib.fleet_eval_last_error(None).decode().startswith("fleet_eval_create: the env needs auto_reset = 1")
    core.close()
    bad = DevicePolicy(pm.random_layers(np.random.default_rng(1), (D, 4, N + 1)), activation="tanh", output="clip")
    with pytest.raises(FleetHipError) as err:
        DeviceEvalCallback(bad, rig.env)
    assert "fleet_eval_create: the policy's act_dim is 3, the env's 2" in str(err.value)
    with pytest.raises(FleetHipError) as err:
        DeviceEvalCallback(rig.pol, rig.env, max_episodes=70000)
    assert "fleet_eval_create: max_episodes must be in 1..65536, got 70000" in str(err.value)
    for h in (wrong, bad, other):
        h.close()
    raw.close(), rig.close()


# ---- 8. the example -------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_at_a_small_size_and_reports_evaluations():
    root = em.ROOT
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "ppo_device_eval.py"), "--iterations", "4", "--eval-every", "2", "--envs", "8",
                          "--eval-envs", "3", "--evs", "2", "--steps", "5", "--batch-size", "16", "--epochs", "1", "--episode-hours", "1"],
                         capture_output=True, text=True, cwd=root, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    evals = [line for line in lines if "eval/mean_reward" in line]
    assert len(evals) == 2 and [e["num_timesteps"] for e in evals] == [80, 160]
    assert all(np.isfinite(e["eval/mean_reward"]) and e["eval/mean_ep_length"] == 4.0 for e in evals)
    assert evals[0]["new_best"] is True and evals[1]["best_mean_reward"] >= evals[0]["best_mean_reward"]
