"""What the GPU tests of SAC's collector and of its evaluation share (tests/test_sac_collect_gpu.py, tests/test_sac_eval_gpu.py): the
env of tests/test_collect_gpu.py -- episodes of 8 steps, staggered -- the state it is compared by, and a small SAC agent."""
import numpy as np
import torch

import policy_model as pm

F32 = np.float32
SEED = 0x1234567890ABCDEF  # (both key words in use)
EP_HOURS = 2               # episodes of 8 steps


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
    and hold what the allocation held (include/fleet_hip.h fleet_fork_envs) -- so those are blanked."""
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


def sac_layers(D, N, salt=0, hidden=(8, 8)):
    """(actor layers (D, 8, 8, 2N), [two critics (D + N, 8, 8, 1)]) of a small SAC agent."""
    rng = np.random.default_rng(1000 * salt + 10 * D + N + 11)
    actor = pm.random_layers(rng, (D,) + tuple(hidden) + (2 * N,))
    critics = [pm.random_layers(rng, (D + N,) + tuple(hidden) + (1,)) for _ in range(2)]
    return actor, critics


def flat(actor, critics):
    """The tensors in the image's order: W, b per layer of the actor, then of critic 0, then of critic 1."""
    return [t for net in [actor] + list(critics) for w, b in net for t in (w, b)]
