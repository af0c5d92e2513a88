"""VecNormalize on the device (fleet_norm.hip) against the float64 model of tests/vecnorm_model.py.  Needs an MI355X."""
import contextlib

import numpy as np
import pytest

from vecnorm_model import VecNormModel, check_stats, close_f32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def set_model_state(norm, model):
    from fleetrl_amd.vec_normalize import RunningStats

    norm.set_state(RunningStats(model.obs_rms.mean, model.obs_rms.var, model.obs_rms.count),
                   RunningStats(np.float64(model.ret_rms.mean), np.float64(model.ret_rms.var), model.ret_rms.count), model.returns)


def adversarial_batch(gen, E, D, dev):
    x = torch.randn((E, D), device=dev, generator=gen, dtype=torch.float32) * 3 + 1
    x[:, 0] = 7.0                                                                       # constant column
    x[:, 1] = 1e4 + 0.1 * torch.randn(E, device=dev, generator=gen)                     # large mean, var 1e-2
    spikes = torch.rand((E,), device=dev, generator=gen) < 0.02
    x[:, 2] = torch.where(spikes, torch.full_like(x[:, 2], 1e3), x[:, 2])                # rare values far past the clip
    if D > 3:
        x[:, 3] = 50 * torch.randn(E, device=dev, generator=gen)                          # hits +-clip_obs
    return x


@pytest.mark.parametrize("E", [1, 5, 64, 65, 4096])
@pytest.mark.parametrize("D", [1, 17, 388])
@pytest.mark.parametrize("in_place", [False, True])
def test_apply_is_bit_exact(E, D, in_place):
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    rng = np.random.default_rng(E * 1000 + D)
    model = VecNormModel(E, D, training=False, clip_obs=4.0, clip_reward=2.0)
    model.obs_rms.mean = rng.normal(0, 5, D)
    model.obs_rms.var = rng.uniform(0, 9, D)
    model.obs_rms.var[0] = 0.0
    model.obs_rms.count = 1234.0001
    model.ret_rms.mean, model.ret_rms.var, model.ret_rms.count = np.float64(0.3), np.float64(2.5), 99.0001
    model.returns = rng.normal(0, 3, E)
    norm = DeviceNormalizer(E, D, training=False, clip_obs=4.0, clip_reward=2.0)
    set_model_state(norm, model)
    dev = torch.device("cuda", 0)
    for step in range(3):
        obs = rng.normal(0, 10, (E, D)).astype(np.float32)
        rew = rng.normal(0, 5, E)
        done = rng.random(E) < 0.3
        term = rng.normal(0, 10, (E, D)).astype(np.float32)
        t_obs, t_rew, t_term = (torch.from_numpy(a).to(dev) for a in (obs, rew, term))
        t_done = torch.from_numpy(done.astype(np.uint8)).to(dev)
        if in_place:
            o, r, t = norm.step_torch(t_obs, t_rew, t_done, t_term, obs_out=t_obs, reward_out=t_rew, terminal_out=t_term)
        else:
            o, r, t = norm.step_torch(t_obs, t_rew, t_done, t_term)
        torch.cuda.synchronize()
        mo, mr, mt = model.step(obs, rew, done, term)
        assert np.array_equal(u32(o.cpu().numpy()), u32(mo)), step
        assert np.array_equal(r.cpu().numpy().view(np.uint64), mr.view(np.uint64)), step
        tt = t.cpu().numpy()
        assert np.array_equal(u32(tt[done]), u32(mt[done])), step
        st = norm.get_state()
        assert np.array_equal(st.returns.view(np.uint64), model.returns.view(np.uint64))
        assert st.obs_rms.count == model.obs_rms.count and st.ret_rms.count == model.ret_rms.count
    # after an in-place step the raw observations are gone
    with pytest.raises(Exception) if in_place else contextlib.nullcontext():
        norm.original(obs=True, reward=False)
    norm.close()


@pytest.mark.parametrize("E,D", [(4096, 388), (4096, 1407), (8192, 388), (8192, 1407)])
def test_training_statistics_follow_the_model(E, D):
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(E + D)
    norm = DeviceNormalizer(E, D)
    model = VecNormModel(E, D)
    x = adversarial_batch(gen, E, D, dev)
    o = norm.reset_torch(x)
    mo = model.reset(x.cpu().numpy())
    assert close_f32(o.cpu().numpy(), mo)
    check_stats(norm, model, "reset")
    for k in range(200):
        x = adversarial_batch(gen, E, D, dev)
        rew = (torch.randn(E, device=dev, generator=gen, dtype=torch.float64) * 20 - 5)
        done = (torch.rand(E, device=dev, generator=gen) < 0.05).to(torch.uint8)
        term = adversarial_batch(gen, E, D, dev)
        o, r, t = norm.step_torch(x, rew, done, term)
        dn = done.cpu().numpy().astype(bool)
        check = k % 20 == 0 or k == 199
        mo, mr, mt = model.step(x.cpu().numpy(), rew.cpu().numpy(), dn, term.cpu().numpy() if check else None, outputs=check)
        if check:
            check_stats(norm, model, k)
            assert close_f32(o.cpu().numpy(), mo), k
            rr = r.cpu().numpy()
            assert np.all((np.abs(rr - mr) <= 1e-6) | (np.abs(rr - mr) <= 2 * np.spacing(np.abs(mr).astype(np.float32)))), k
            assert close_f32(t.cpu().numpy()[dn], mt[dn]), k
    norm.close()


def make_env(E=4096, N=50, seed=5):
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv
    from fleetrl_amd.synth import synth_tables

    return FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=seed)


def test_through_the_env_with_c3_flags():
    """FleetVecNormalize(FleetVecEnv) over two episodes and more, at every step against the model fed the raw outputs of an
    identically seeded plain FleetVecEnv."""
    from fleetrl_amd import FleetVecNormalize

    E = 4096
    raw_env, env = make_env(E), make_env(E)
    vn = FleetVecNormalize(env, norm_obs=True, norm_reward=True, clip_reward=10.0)
    model = VecNormModel(E, env.core.obs_dim, clip_reward=10.0)
    ro = raw_env.reset()
    o = vn.reset()
    assert np.array_equal(vn.get_original_obs(), ro)
    assert close_f32(o, model.reset(ro))
    rng = np.random.default_rng(0)
    episodes = 0
    for k in range(2 * 192 + 20):
        a = rng.uniform(-1, 1, size=(E, env.core.num_cars)).astype(np.float32)
        ro, rr, rd, rinfo = raw_env.step(a)
        o, r, d, info = vn.step(a)
        assert np.array_equal(d, rd), k
        rterm = np.zeros_like(ro)
        for i in np.flatnonzero(rd):
            rterm[i] = rinfo[i]["terminal_observation"]
        mo, mr, mt = model.step(ro, rr, rd, rterm)
        assert close_f32(o, mo), k
        assert np.all((np.abs(r - mr) <= 1e-6) | (np.abs(r - mr) <= 2 * np.spacing(np.abs(mr).astype(np.float32)))), k
        for i in np.flatnonzero(rd):
            assert close_f32(info[i]["terminal_observation"], mt[i]), (k, i)
            assert info[i]["episode"] == rinfo[i]["episode"], (k, i)
        episodes += int(rd.sum())
        if k % 50 == 0:
            assert np.array_equal(vn.get_original_obs(), ro) and np.array_equal(vn.get_original_reward(), rr)
            check_stats(vn.norm, model, k)
    assert episodes >= 2 * E
    check_stats(vn.norm, model, "end")
    vn.close()
    raw_env.close()


def run_pair(steps=60, E=512, use_torch=False, seed=3):
    from fleetrl_amd import FleetVecNormalize

    env = make_env(E, seed=seed)
    vn = FleetVecNormalize(env)
    rng = np.random.default_rng(1)
    dev = torch.device("cuda", 0)
    outs = []
    if use_torch:
        term = torch.zeros((E, env.core.obs_dim), device=dev)
        outs.append(vn.reset_torch().cpu().numpy())
    else:
        outs.append(vn.reset())
    for _ in range(steps):
        a = rng.uniform(-1, 1, size=(E, env.core.num_cars)).astype(np.float32)
        if use_torch:
            o, r, d = vn.step_torch(torch.from_numpy(a).to(dev), terminal_out=term)
            o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy().astype(bool)
            t = term.cpu().numpy()[d]
        else:
            o, r, d, info = vn.step(a)
            t = np.array([info[i]["terminal_observation"] for i in np.flatnonzero(d)], dtype=np.float32).reshape(-1, env.core.obs_dim)
        outs += [o, r, d, t]
    st = vn.norm.get_state()
    outs += [st.obs_rms.mean, st.obs_rms.var, np.float64(st.obs_rms.count), np.float64(st.ret_rms.mean), np.float64(st.ret_rms.var),
             st.returns]
    vn.close()
    return outs


def test_host_path_equals_torch_path_and_runs_repeat():
    a = run_pair(steps=250)
    b = run_pair(steps=250)
    c = run_pair(steps=250, use_torch=True)
    for x, y, z in zip(a, b, c):
        x, y, z = (np.ascontiguousarray(v) for v in (x, y, z))
        assert x.dtype == y.dtype == z.dtype and x.shape == y.shape == z.shape
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_modes_and_persistence(tmp_path):
    from fleetrl_amd import FleetVecNormalize, sync_normalization
    from fleetrl_amd import _capi

    E = 256
    raw_env, env = make_env(E, seed=9), make_env(E, seed=9)
    vn = FleetVecNormalize(env, gamma=0.9)
    model = VecNormModel(E, env.core.obs_dim, gamma=0.9)
    rng = np.random.default_rng(2)
    model.reset(raw_env.reset())
    vn.reset()
    schedule = {20: ("norm_reward", False), 40: ("norm_obs", False), 60: ("training", False), 80: ("norm_obs", True),
                100: ("training", True), 120: ("norm_reward", True)}
    saved_at = 140
    for k in range(200):
        if k in schedule:
            name, val = schedule[k]
            setattr(vn, name, val)
            setattr(model, name, val)
            assert getattr(vn, name) == val
        if k == saved_at:
            p = tmp_path / "vn.npz"
            vn.save(p)
            vn.close()
            vn = FleetVecNormalize.load(p, env := make_env(E, seed=9))
            # the new env starts over: replay the raw env from its start too, with the statistics carried over and zero returns
            raw_env.close()
            raw_env = make_env(E, seed=9)
            model.returns = np.zeros(E)
            vn.training = False
            model.training = False
            assert close_f32(vn.reset(), model.reset(raw_env.reset()))
            vn.training = True
            model.training = True
        a = rng.uniform(-1, 1, size=(E, env.core.num_cars)).astype(np.float32)
        ro, rr, rd, rinfo = raw_env.step(a)
        o, r, d, info = vn.step(a)
        mo, mr, _ = model.step(ro, rr, rd)
        assert np.array_equal(d, rd)
        assert close_f32(o, mo), k
        assert np.all((np.abs(r - mr) <= 1e-6) | (np.abs(r - mr) <= 2 * np.spacing(np.abs(mr).astype(np.float32)))), k
        if k % 10 == 0:
            check_stats(vn.norm, model, k)
    # an eval env takes the training env's statistics
    ev = FleetVecNormalize(make_env(E, seed=11), training=False, norm_reward=False)
    sync_normalization(vn, ev)
    a, b = vn.obs_rms, ev.obs_rms
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.var, b.var) and a.count == b.count
    assert vn.ret_rms.count == ev.ret_rms.count
    # a normaliser of another shape is refused by the host path
    other = FleetVecNormalize(make_env(64, seed=1))
    lib = env.core.batch.lib
    acts = np.zeros((E, env.core.num_cars), np.float32)
    obs = np.zeros((E, env.core.obs_dim), np.float32)
    rew, done = np.zeros(E), np.zeros(E, np.uint8)
    rc = lib.fleet_step_host_norm(env.core.batch.h, other.norm.h, acts.ctypes.data, _capi.ACT_F32, obs.ctypes.data, rew.ctypes.data,
                                  done.ctypes.data, None)
    assert rc == _capi.ERR_INVALID and b"64" in lib.fleet_last_error(env.core.batch.h)
    assert lib.fleet_reset_host_norm(env.core.batch.h, other.norm.h, obs.ctypes.data) == _capi.ERR_INVALID
    for x in (vn, ev, other):
        x.close()
    raw_env.close()
