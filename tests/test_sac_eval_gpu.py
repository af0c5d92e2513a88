"""The evaluation of a SAC agent on the device (include/fleet_hip_sac_loop.h, fleet_eval.hip): the one call against
sync_normalization + the unchanged fleetrl_amd.evaluate_policy driven through a three-line adapter, bit for bit; the Monitor source
against the env's own records read step by step; the gate and the snapshot of the WHOLE image against what the host decides from the
means; the refusals that tell the two kinds of handle apart.  Everything is bit equality: no tolerance."""
import types

import numpy as np
import pytest

import sac_loop_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from sac_loop_rig import assert_same_dict, dev, env_state, flat, host, make_env, sac_layers, same  # noqa: E402

em = sm.em
F32 = np.float32
U = 2.0 ** -53


class Deterministic:
    """The adapter evaluate_policy is driven through: a SAC agent's deterministic action behind a policy's `act`."""

    def __init__(self, nets):
        self.nets, self.obs_dim, self.act_dim = nets, nets.obs_dim, nets.act_dim

    def act(self, obs, out):
        return self.nets.act(obs, deterministic=True, actions_out=out)


def trained_normalizer(D, seed, E=4):
    """A normaliser with statistics of its own: three training steps on random data."""
    from fleetrl_amd import DeviceNormalizer

    n = DeviceNormalizer(E, D)
    rng = np.random.default_rng(seed)
    n.use_torch_stream()
    for _ in range(3):
        raw = torch.from_numpy((rng.standard_normal((E, D)) * 3 + 1).astype(F32)).to(dev())
        rew = torch.from_numpy(rng.standard_normal(E) * 5).to(dev())
        done = torch.from_numpy((rng.random(E) < 0.3).astype(np.uint8)).to(dev())
        n.step_torch(raw, rew, done)
    torch.cuda.synchronize()
    return n


class Rig:
    """An evaluation env, a SAC agent, (with a normaliser) a trained training normaliser, and the callback."""

    def __init__(self, E, N, with_norm, n_eval, monitor=False, layers=None, **env_kw):
        from fleetrl_amd import DeviceEvalCallback, DeviceSACNetworks

        self.E, self.N, self.with_norm, self.n_eval = E, N, with_norm, n_eval
        self.env = make_env(E, N, with_norm, **env_kw)
        self.venv = getattr(self.env, "venv", self.env)
        self.D = D = self.venv.core.obs_dim
        self.layers = layers or sac_layers(D, N)
        self.nets = DeviceSACNetworks(*self.layers, activation="relu")
        self.train_norm = trained_normalizer(D, 11) if with_norm else None
        self.cb = DeviceEvalCallback(self.nets, self.env, n_eval_episodes=n_eval, monitor=monitor, train_normalizer=self.train_norm)
        torch.cuda.synchronize()

    def one_call(self, num_timesteps=1000):
        stats = self.cb.evaluate(num_timesteps)
        r, n = self.cb.episodes()
        return dict(rewards=r, lengths=n, stats=host(stats), **env_state(self.env))

    def sync(self):
        from fleetrl_amd import sync_normalization

        if self.with_norm:
            st = self.train_norm.get_state()
            sync_normalization(types.SimpleNamespace(obs_rms=st.obs_rms, ret_rms=st.ret_rms), self.env)

    def pieces(self):
        """What a training loop did before: sync_normalization, then evaluate_policy."""
        from fleetrl_amd import evaluate_policy

        self.sync()
        r, n = evaluate_policy(Deterministic(self.nets), self.env, n_eval_episodes=self.n_eval, return_episode_rewards=True)
        torch.cuda.synchronize()
        return dict(rewards=np.array(r, np.float64), lengths=np.array(n, np.int32), **env_state(self.env))

    def monitor_pieces(self):
        """The same loop step by step with the env's own episode records (what Monitor reports) read after every step."""
        E, N, D, batch = self.E, self.N, self.D, self.venv.core.batch
        self.sync()
        obs, act = torch.empty((E, D), device=dev()), torch.empty((E, N), device=dev())
        reward, done = torch.empty(E, device=dev(), dtype=torch.float64), torch.empty(E, device=dev(), dtype=torch.uint8)
        ret, length = torch.empty(E, device=dev(), dtype=torch.float64), torch.empty(E, device=dev(), dtype=torch.int32)
        ev = em.Evaluation(E, self.n_eval)
        if self.with_norm:
            self.env.reset_torch(obs_out=obs)
        else:
            batch.use_torch_stream()
            self.venv._torch_stream = torch.cuda.current_stream(dev()).cuda_stream
            batch.reset_dev(obs.data_ptr())
        for _ in range(self.cb.n_steps()):
            self.nets.act(obs, deterministic=True, actions_out=act)
            self.env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done)
            batch.get_dev("last_ep_return", ret.data_ptr())
            batch.get_dev("last_ep_len", length.data_ptr())
            r = host(reward) if self.with_norm else host(reward).astype(F32).astype(np.float64)
            ev.step(host(done).astype(bool), r, self.n_eval, 1, host(ret), host(length))
        return dict(rewards=ev.lists()[0], lengths=ev.lists()[1], **env_state(self.env)), ev

    def close(self):
        for h in (self.cb, self.nets, self.train_norm, self.env):
            if h is not None:
                h.close()


def check_stats(stats, rewards, lengths, num_timesteps, evaluations):
    """stats[0..4] are the model's bits (the ordered sum S over the lists); np.mean / np.std, which add in another order, lie within the
    bounds tests/test_eval_cpu.py derives for S."""
    n = rewards.size
    want = np.array(em.mean_std(rewards) + em.mean_std(lengths.astype(np.float64)) + (np.float64(n),))
    assert same(stats[:5], want), (stats[:5], want)
    for x, mean, std in ((rewards, stats[0], stats[1]), (lengths.astype(np.float64), stats[2], stats[3])):
        tot, sd = float(np.sum(np.abs(x))), float(np.std(x))
        assert abs(mean - np.mean(x)) <= 2 * ((n - 1) * U * tot / n + U * abs(np.mean(x)))
        dm = U * (tot + abs(np.mean(x)))
        assert abs(std - sd) <= (2 * (sd * (n / 2 + 4) * U + dm * dm / sd) if sd > 0 else 0.0)
    assert stats[7] == num_timesteps and stats[8] == evaluations and not stats[9:].any()


# ---- 1. bit equality with the existing path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("monitor", [False, True], ids=["sums", "monitor"])
@pytest.mark.parametrize("with_norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("E,N,n_eval", [(3, 2, 5), (65, 5, 7)])
def test_the_one_call_equals_sync_normalization_and_evaluate_policy(E, N, n_eval, with_norm, monitor):
    """monitor False: the lists are evaluate_policy's.  monitor True: evaluate_policy is SB3's loop on an env WITHOUT Monitor -- its
    rewards are sums of step rewards, not the env's raw episode returns -- so its lengths and the state it leaves are compared, and the
    rewards against the env's own records read after every step of the same loop."""
    a, b = Rig(E, N, with_norm, n_eval, monitor), Rig(E, N, with_norm, n_eval, monitor)
    n_steps = -(-n_eval // E) * 8
    assert em.targets(n_eval, E).tolist() == ([1, 2, 2] if E == 3 else [0] * 58 + [1] * 7)
    for call in range(2):  # (the second evaluation starts from the first one's env and normaliser)
        got = a.one_call(1000 + call)
        stats = got.pop("stats")
        if monitor:
            want, ev = b.monitor_pieces()
            assert_same_dict(got, want, (E, N, n_eval, with_norm, call))
            assert same(stats[:5], ev.finish(1000 + call)[:5])
            c = Rig(E, N, with_norm, n_eval, monitor) if call == 0 else None
            if c is not None:  # evaluate_policy itself: the same lengths, the same env and normaliser afterwards
                plain = c.pieces()
                assert same(plain["lengths"], got["lengths"])
                assert_same_dict({k: v for k, v in plain.items() if k != "rewards"}, {k: v for k, v in got.items() if k != "rewards"}, "monitor")
                c.close()
        else:
            want = b.pieces()
            assert_same_dict(got, want, (E, N, n_eval, with_norm, call))
        assert got["rewards"].size == n_eval and (got["lengths"] == 8).all()
        check_stats(stats, got["rewards"], got["lengths"], 1000 + call, call + 1)
        assert a.cb.n_steps() == n_steps
        assert a.cb.describe()["launches"] == sm.launches_eval(n_steps, with_norm, with_norm) == (4 if with_norm else 3) * n_steps + (6 if with_norm else 4)
    res = a.cb.results()
    assert res["eval/mean_reward"] == stats[0] and res["eval/mean_ep_length"] == 8.0 and res["num_timesteps"] == 1001
    a.cb.check_errors()
    a.close(), b.close()


# ---- 2. the gate and the snapshot -----------------------------------------------------------------------------------------------------
def constant_agent(D, N, value, salt):
    """SAC weights whose deterministic action is tanh(value) in every column, whatever it observes; random critics of their own."""
    actor, critics = sac_layers(D, N, salt=salt)
    w, b = actor[-1]
    actor[-1] = (np.zeros_like(w), np.concatenate([np.full(N, value, F32), np.zeros(N, F32)]))
    return actor, critics


def load(nets, layers):
    nets.load_torch([torch.from_numpy(t).to(dev()) for t in flat(*layers)])


def test_the_gate_and_the_snapshot_follow_the_means_in_either_order():
    from fleetrl_amd import DeviceEvalCallback, DeviceSACNetworks, FleetHipError, _capi

    E, N, n_eval = 3, 2, 5
    starts = np.array([[40, 136, 232]], np.int32)  # one scheduled start per env: every evaluation meets the same episodes
    envs = [make_env(E, N, False, start_rows=starts) for _ in range(2)]
    D = envs[0].core.obs_dim
    X, Y = constant_agent(D, N, 3.0, salt=1), constant_agent(D, N, -3.0, salt=2)  # charge whenever possible / discharge
    obs = torch.from_numpy(np.random.default_rng(2).standard_normal((7, D)).astype(F32)).to(dev())
    means = {}
    for env, order in zip(envs, (("X", "Y"), ("Y", "X"))):
        weights = {"X": X, "Y": Y}
        nets = DeviceSACNetworks(*weights[order[0]], activation="relu")
        third = DeviceSACNetworks(*sac_layers(D, N, salt=9), activation="relu")
        cb = DeviceEvalCallback(nets, env, n_eval_episodes=n_eval, monitor=False)
        with pytest.raises(FleetHipError) as err:  # before any evaluation has run
            cb.load_best_into(third)
        assert err.value.status == _capi.ERR_STATE and "fleet_saceval_best_load_dev: no evaluation has run on this handle" in str(err.value)
        best, winner = -np.inf, None
        for k, name in enumerate(order):
            if k:
                load(nets, weights[name])
            s = host(cb.evaluate(10 * (k + 1)))
            mean = s[0]
            means.setdefault(name, mean)
            assert mean == means[name]  # (the scheduled starts: the same episodes on either handle)
            new_best = bool(mean > best)  # what the host decides, SB3's strict comparison
            if new_best:
                best, winner = mean, name
            assert s[6] == float(new_best) and s[5] == best and host(cb.arrays()["gate"])[0] == int(new_best), (order, k)
            out = cb.best_parameters()
            want = flat(*weights[winner])
            assert len(out) == len(want) == 18 and all(same(host(g), w) for g, w in zip(out, want)), (order, k)
        assert winner == max(means, key=means.get)
        # the whole image goes into a third handle: the actor AND the critics, bit for bit, and it acts as the winner does
        cb.load_best_into(third)
        got, want = third.export_torch(), flat(*weights[winner])
        assert all(same(host(g), w) for g, w in zip(got, want))
        ref = DeviceSACNetworks(*weights[winner], activation="relu")
        for kw in (dict(deterministic=True), dict(seed=5, step=3)):
            assert same(host(third.act(obs, **kw)), host(ref.act(obs, **kw)))
        assert not same(host(third.act(obs, deterministic=True)), host(nets.act(obs, deterministic=True))) or winner == order[1]
        res = cb.results()
        assert res["best_mean_reward"] == best and res["num_timesteps"] == 20
        for h in (cb, nets, third, ref):
            h.close()
    # the two agents differ by construction; X then Y and Y then X: in exactly one order the second evaluation is a new best
    assert means["X"] != means["Y"], means
    for env in envs:
        env.close()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
def test_the_load_entries_refuse_the_other_kind_of_handle_and_another_layout():
    import policy_model as pm
    from fleetrl_amd import DeviceEvalCallback, DevicePolicy, DeviceSACNetworks, DeviceTD3Target, FleetHipError, _capi

    rig = Rig(3, 2, False, 5)
    cb, D, N = rig.cb, rig.D, 2
    lib = _capi.load_library()
    pol = DevicePolicy(pm.random_layers(np.random.default_rng(1), (D, 8, N)), activation="tanh", output="clip")
    plain_cb = DeviceEvalCallback(pol, rig.env, n_eval_episodes=5)
    twin = DeviceSACNetworks(*sac_layers(D, N, salt=4), activation="relu")
    other = DeviceSACNetworks(*sac_layers(D, N, salt=4, hidden=(8,)), activation="relu")
    for h in (cb, plain_cb, pol, twin, other):
        h.use_torch_stream()
    before = host(twin.export_torch()[0])

    def refused(fn, word, status=_capi.ERR_INVALID):
        with pytest.raises(FleetHipError) as err:
            fn()
        assert err.value.status == status and word in str(err.value), str(err.value)

    refused(lambda: cb._check(lib.fleet_saceval_best_load_dev(cb.h, twin.h)), "fleet_saceval_best_load_dev: no evaluation has run on this handle",
            _capi.ERR_STATE)
    refused(lambda: cb.best_parameters(), "fleet_eval_best_export_dev: no evaluation has run on this handle", _capi.ERR_STATE)
    cb.evaluate(10)
    plain_cb.evaluate(10)
    refused(lambda: cb._check(lib.fleet_eval_best_load_dev(cb.h, pol.h)),
            "fleet_eval_best_load_dev: the handle evaluates SAC networks (fleet_saceval_create): fleet_saceval_best_load_dev loads its snapshot")
    refused(lambda: plain_cb._check(lib.fleet_saceval_best_load_dev(plain_cb.h, twin.h)),
            "fleet_saceval_best_load_dev: the handle evaluates a policy (fleet_eval_create): fleet_eval_best_load_dev loads its snapshot")
    refused(lambda: cb.load_best_into(other), "fleet_saceval_best_load_dev: the destination networks handle's layout differs from the evaluated networks'")
    refused(lambda: cb._check(lib.fleet_saceval_best_load_dev(cb.h, pol.h)), "fleet_saceval_best_load_dev: the handle is not a networks handle")
    td3 = DeviceTD3Target(pm.random_layers(np.random.default_rng(3), (D, 8, 8, N)), rig.layers[1], activation="relu", output="tanh")  # no squashed actor
    td3.use_torch_stream()
    refused(lambda: cb._check(lib.fleet_saceval_best_load_dev(cb.h, td3.h)), "the destination networks handle's actor is not a squashed Gaussian")
    side = torch.cuda.Stream(dev())
    twin.set_stream(side.cuda_stream)
    refused(lambda: cb._check(lib.fleet_saceval_best_load_dev(cb.h, twin.h)),
            "the destination networks handle launches on another stream than the env: fleet_qtarget_set_stream it to the env's first")
    twin.use_torch_stream()
    torch.cuda.synchronize()
    assert same(host(twin.export_torch()[0]), before)  # nothing was copied by any of it
    # create: networks that are not squashed, a wrong act_dim; the policy's callback still refuses what is neither
    with pytest.raises(FleetHipError) as err:
        DeviceEvalCallback(DeviceSACNetworks(*sac_layers(D, N + 1), activation="relu"), rig.env)
    assert f"fleet_saceval_create: the networks' act_dim is {N + 1}, the env's {N}" in str(err.value)
    import ctypes as C

    h, p = C.c_void_p(), _capi.FleetEvalParams(C.sizeof(_capi.FleetEvalParams), 5)
    assert lib.fleet_saceval_create(rig.venv.core.batch.h, None, td3.h, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
    assert lib.fleet_eval_last_error(None).decode() == "fleet_saceval_create: the networks' actor is not a squashed Gaussian: fleet_sac_create makes one"
    cb.load_best_into(twin)  # ... and the proper call goes through
    assert all(same(host(g), w) for g, w in zip(twin.export_torch(), flat(*rig.layers)))
    for x in (plain_cb, pol, twin, other, td3):
        x.close()
    rig.close()
