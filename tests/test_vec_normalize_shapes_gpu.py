"""The reduction half of fleet_norm.hip (norm_moments -> norm_finalize) off the aligned shapes, and what hangs on it: ragged last
slabs, slab counts off the multiples of 4 and 64, masked column tiles, hostile columns (a row 0 that is an outlier: the shift),
column independence bit for bit, the choice between the 16-byte and the scalar apply path, the modes at a ragged shape, and the
env at small sizes.  Against the float64 model of tests/vecnorm_model.py, with `check_stats`'s tolerances.  Needs an MI355X.
tests/test_vec_normalize_order_cpu.py runs the summation scheme's NumPy restatement on the same inputs."""
import numpy as np
import pytest

from vecnorm_cases import (HOSTILE_D, HOSTILE_E, RAGGED_D, RAGGED_E, hostile_batch, hostile_dones, hostile_rewards, hostile_start,
                           ragged_batch, ragged_step)
from vecnorm_model import VecNormModel, check_stats, close_f32, close_reward

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = torch.device("cuda", 0)


def up(a):
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8) if a.dtype == bool else a)).to(DEV)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def set_model_state(norm, model):
    from fleetrl_amd.vec_normalize import RunningStats

    norm.set_state(RunningStats(model.obs_rms.mean, model.obs_rms.var, model.obs_rms.count),
                   RunningStats(np.float64(model.ret_rms.mean), np.float64(model.ret_rms.var), model.ret_rms.count), model.returns)


def step_and_check(norm, model, obs, rew, done, term, tag):
    """One step on both; the statistics by `check_stats`, the outputs by the criteria of tests/test_vec_normalize_gpu.py."""
    o, r, t = norm.step_torch(up(obs), up(rew), up(done), None if term is None else up(term))
    mo, mr, mt = model.step(obs, rew, done, term)
    check_stats(norm, model, tag)
    assert close_f32(o.cpu().numpy(), mo), tag
    assert close_reward(r.cpu().numpy(), mr), tag
    if term is not None:
        assert close_f32(t.cpu().numpy()[done], mt[done]), tag
    return o.cpu().numpy(), r.cpu().numpy()


# ---- a. the ragged shape matrix --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", RAGGED_D)
@pytest.mark.parametrize("E", RAGGED_E)
def test_training_statistics_over_the_ragged_shape_matrix(E, D):
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    rng = np.random.default_rng([7, E, D])
    norm, model = DeviceNormalizer(E, D), VecNormModel(E, D)
    x = ragged_batch(rng, E, D)
    o = norm.reset_torch(up(x))
    assert close_f32(o.cpu().numpy(), model.reset(x))
    check_stats(norm, model, "reset")
    dones = 0
    for k in range(6):
        obs, rew, done, term = ragged_step(rng, E, D)
        if k == 2:
            done[E - 1] = True  # (the last row of the last slab: E = 1 .. 5 would rarely see a done otherwise)
        dones += int(done.sum())
        step_and_check(norm, model, obs, rew, done, term, k)
    assert dones > 0
    norm.close()


# ---- b. hostile inputs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", HOSTILE_E)
def test_hostile_columns(E):
    """A constant column (started at its own mean with variance 0: the batch variance must be EXACTLY 0.0), far-from-zero columns
    with a typical and with a zero row 0, outliers in row 0 (the shift K), all rows equal but the last, 1e-30, +-3e38 (squares
    past float32, not float64)."""
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    D = HOSTILE_D
    norm, model = DeviceNormalizer(E, D), VecNormModel(E, D)
    hostile_start(model)
    set_model_state(norm, model)
    x = hostile_batch(E, 0)
    const = float(x[0, 0])
    o = norm.reset_torch(up(x))
    assert close_f32(o.cpu().numpy(), model.reset(x))
    check_stats(norm, model, "reset")
    for k in range(1, 6):
        step_and_check(norm, model, hostile_batch(E, k), hostile_rewards(E, k), hostile_dones(E, k), hostile_batch(E, k + 100), k)
        st = norm.get_state()
        assert st.obs_rms.var[0] == 0.0 and st.obs_rms.mean[0] == const, k
        assert u64(st.obs_rms.var[:1]) == u64(model.obs_rms.var[:1]) and u64(st.obs_rms.mean[:1]) == u64(model.obs_rms.mean[:1]), k
        assert np.all(np.isfinite(st.obs_rms.mean)) and np.all(np.isfinite(st.obs_rms.var)), k
    norm.close()


@pytest.mark.parametrize("E", HOSTILE_E)
def test_hostile_returns(E):
    """gamma = 1 with rewards near 1e6 over 50 steps without a done; gamma = 0; a step where every env is done."""
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    D = HOSTILE_D
    norm, model = DeviceNormalizer(E, D, gamma=1.0), VecNormModel(E, D, gamma=1.0)
    for k in range(50):
        step_and_check(norm, model, hostile_batch(E, k % 6), hostile_rewards(E, k, 1e3, 1e6), np.zeros(E, bool), None, ("gamma 1", k))
    assert model.returns.min() > 4e7
    norm.close()
    norm, model = DeviceNormalizer(E, D, gamma=0.0), VecNormModel(E, D, gamma=0.0)
    for k in range(6):
        step_and_check(norm, model, hostile_batch(E, k), hostile_rewards(E, k), hostile_dones(E, k), hostile_batch(E, k + 100), ("gamma 0", k))
    norm.close()
    norm, model = DeviceNormalizer(E, D), VecNormModel(E, D)
    for k in range(6):
        done = np.ones(E, bool) if k == 2 else hostile_dones(E, k)
        step_and_check(norm, model, hostile_batch(E, k), hostile_rewards(E, k), done, hostile_batch(E, k + 100), ("all done", k))
        assert k != 2 or not norm.get_state().returns.any()
    norm.close()


# ---- c. column independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [65, 4161])
def test_a_column_s_statistics_do_not_depend_on_where_it_sits(E):
    """Each column is summed in an order fixed by E alone: the same data in another column, tile or width gives the same bits."""
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    rng = np.random.default_rng([11, E])
    updates = 5
    cols = np.empty((updates, E, 4), np.float32)
    cols[..., 0] = 1 + 3 * rng.standard_normal((updates, E))
    cols[..., 1] = 1e4 + 0.1 * rng.standard_normal((updates, E))
    cols[..., 2] = -300 + 50 * rng.standard_normal((updates, E))
    cols[..., 3] = np.where(rng.random((updates, E)) < 0.02, 1e3, rng.standard_normal((updates, E)))
    cols[:, 0, 3] = 1e3  # (and an outlier as the shift)
    layouts = [(388, (0, 63, 64, 387)), (5, (4, 0, 2, 1)), (65, (64, 0, 63, 1)), (1407, (1406, 64, 1, 703))]
    got = []
    for D, pos in layouts:
        fill = np.random.default_rng([12, E, D])
        norm = DeviceNormalizer(E, D)
        rows = []
        for k in range(updates):
            x = ragged_batch(fill, E, D)
            x[:, list(pos)] = cols[k]
            if k == 0:
                norm.reset_torch(up(x))
            else:
                norm.step_torch(up(x), up(fill.standard_normal(E)), up(fill.random(E) < 0.2))
            st = norm.get_state()
            rows.append(np.stack([u64(st.obs_rms.mean[list(pos)]), u64(st.obs_rms.var[list(pos)])]))
        got.append(np.stack(rows))
        norm.close()
    for (D, pos), g in zip(layouts[1:], got[1:]):
        assert np.array_equal(g, got[0]), (D, np.argwhere(g != got[0])[:4])


# ---- d. the 16-byte path against the scalar path of norm_apply --------------------------------------------------------------
SENTINEL = -77.25


def one_off(a, misaligned, fill=None):
    """A device copy of `a` (or an output buffer of its shape pre-filled with `fill`) starting 16-byte aligned, or one float into a
    larger allocation of its own."""
    a = np.asarray(a, np.float32)
    flat = torch.full((a.size + 4,), SENTINEL, device=DEV, dtype=torch.float32)
    view = flat[1:1 + a.size] if misaligned else flat[:a.size]
    view = view.view(a.shape)
    if fill is None:
        view.copy_(up(a))
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 == (4 if misaligned else 0) and view.is_contiguous()
    return view, flat


def run_apply_variant(E, D, training, mis=(), obs_in_place=False, term_in_place=False, with_terminal=True):
    """A reset and two steps on a normaliser with given statistics; returns every output and the final state as bytes, plus the
    guard words around each buffer."""
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    rng = np.random.default_rng([13, E, D])
    model = VecNormModel(E, D)
    model.obs_rms.mean = rng.normal(0, 5, D)
    model.obs_rms.var = rng.uniform(0, 9, D)
    model.obs_rms.count = 1234.0001
    model.ret_rms.mean, model.ret_rms.var, model.ret_rms.count = np.float64(0.3), np.float64(2.5), 99.0001
    model.returns = rng.normal(0, 3, E)
    norm = DeviceNormalizer(E, D, training=training)
    set_model_state(norm, model)
    out = []
    x = ragged_batch(rng, E, D)
    raw, raw_flat = one_off(x, "raw_obs" in mis)
    if obs_in_place:
        o = norm.reset_torch(raw, out=raw)
    else:
        o = norm.reset_torch(raw, out=one_off(x, "obs_out" in mis, fill=SENTINEL)[0])
    out.append(o.cpu().numpy())
    for k in range(2):
        obs, rew, done, term = ragged_step(rng, E, D, p_done=0.4)
        if k == 1:
            done[0], done[E - 1] = True, False
        raw, raw_flat = one_off(obs, "raw_obs" in mis)
        obs_out, obs_flat = (raw, raw_flat) if obs_in_place else one_off(obs, "obs_out" in mis, fill=SENTINEL)
        kw = {}
        if with_terminal:
            raw_term, raw_term_flat = one_off(term, "raw_terminal" in mis)
            term_out, term_flat = (raw_term, raw_term_flat) if term_in_place else one_off(term, "terminal_out" in mis, fill=SENTINEL)
            kw = dict(raw_terminal=raw_term, terminal_out=term_out)
        o, r, t = norm.step_torch(raw, up(rew), up(done), obs_out=obs_out, **kw)
        assert o is obs_out and (not with_terminal or t is term_out)
        out += [o.cpu().numpy(), r.cpu().numpy()]
        for flat, view in ((raw_flat, raw), (obs_flat, obs_out)) + (((raw_term_flat, raw_term), (term_flat, term_out)) if with_terminal else ()):
            guard = np.ones(flat.numel(), bool)
            first = (view.data_ptr() - flat.data_ptr()) // 4
            guard[first:first + view.numel()] = False
            assert np.all(flat.cpu().numpy()[guard] == np.float32(SENTINEL)), "a write outside the buffer"
        if not obs_in_place:
            assert np.array_equal(u32(raw.cpu().numpy()), u32(obs)), "the raw observations were written"
        if with_terminal:
            tt = t.cpu().numpy()
            out.append(tt[done])
            # rows of envs that are not done are untouched: the sentinel, or the raw rows when in place
            assert np.array_equal(u32(tt[~done]), u32(term[~done] if term_in_place else np.full_like(term[~done], SENTINEL)))
            if not term_in_place:
                assert np.array_equal(u32(raw_term.cpu().numpy()), u32(term)), "the raw terminal rows were written"
    st = norm.get_state()
    out += [st.obs_rms.mean, st.obs_rms.var, np.float64(st.obs_rms.count), np.float64(st.ret_rms.mean), np.float64(st.ret_rms.var),
            np.float64(st.ret_rms.count), st.returns]
    norm.close()
    return [np.ascontiguousarray(a).tobytes() for a in out]


BUFFERS = ("raw_obs", "obs_out", "raw_terminal", "terminal_out")


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("E", [5, 300])
def test_misaligned_buffers_take_the_scalar_path_and_give_the_same_bits(E, training):
    D = 388
    ref = run_apply_variant(E, D, training)
    for mis in [(b,) for b in BUFFERS] + [BUFFERS]:
        assert run_apply_variant(E, D, training, mis=mis) == ref, mis
    for mis in [(), ("raw_obs",), ("raw_terminal",), ("raw_obs", "raw_terminal")]:
        assert run_apply_variant(E, D, training, mis=mis, obs_in_place=True) == ref, ("obs in place", mis)
        assert run_apply_variant(E, D, training, mis=mis, term_in_place=True) == ref, ("terminal in place", mis)
        assert run_apply_variant(E, D, training, mis=mis, obs_in_place=True, term_in_place=True) == ref, ("both in place", mis)
    # without terminal rows: the same outputs but for the terminal entries (index 3 and 6 of reset, (obs, reward, terminal) x 2, state)
    ref_nt = [a for i, a in enumerate(ref) if i not in (3, 6)]
    for mis in [(), ("raw_obs",), ("obs_out",), ("raw_obs", "obs_out")]:
        assert run_apply_variant(E, D, training, mis=mis, with_terminal=False) == ref_nt, ("no terminal", mis)
    assert run_apply_variant(E, D, training, mis=("raw_obs",), obs_in_place=True, with_terminal=False) == ref_nt


def test_the_aligned_reference_run_is_the_model_s():
    """... so that (d) compares with something right: the aligned run without training equals the model bit for bit."""
    E, D = 300, 388
    ref = run_apply_variant(E, D, False)
    rng = np.random.default_rng([13, E, D])
    model = VecNormModel(E, D, training=False)
    model.obs_rms.mean = rng.normal(0, 5, D)
    model.obs_rms.var = rng.uniform(0, 9, D)
    model.returns = rng.normal(0, 3, E)
    model.ret_rms.var = np.float64(2.5)
    want = [model.reset(ragged_batch(rng, E, D))]
    for k in range(2):
        obs, rew, done, term = ragged_step(rng, E, D, p_done=0.4)
        if k == 1:
            done[0], done[E - 1] = True, False
        o, r, t = model.step(obs, rew, done, term)
        want += [o, r, t[done]]
    for i, w in enumerate(want):
        assert ref[i] == np.ascontiguousarray(w).tobytes(), i
    assert ref[-1] == model.returns.tobytes()


# ---- e. the modes at a ragged shape -----------------------------------------------------------------------------------------
def mode_pair(**kw):
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    E, D = 65, 17
    return E, D, DeviceNormalizer(E, D, **kw), VecNormModel(E, D, **kw), np.random.default_rng([17, len(kw)])


def test_returns_only_training_copies_the_observations():
    """training without norm_obs (the returns-only grid): observations and done terminal rows are bit copies, obs_rms stands still,
    ret_rms advances; a training reset changes nothing but the returns."""
    E, D, norm, model, rng = mode_pair(norm_obs=False)
    x = ragged_batch(rng, E, D)
    assert np.array_equal(u32(norm.reset_torch(up(x)).cpu().numpy()), u32(x))
    for k in range(6):
        obs, rew, done, term = ragged_step(rng, E, D)
        t_out = torch.full((E, D), SENTINEL, device=DEV)
        o, r, t = norm.step_torch(up(obs), up(rew), up(done), up(term), terminal_out=t_out)
        _, mr, _ = model.step(obs, rew, done, term)
        check_stats(norm, model, k)
        assert close_reward(r.cpu().numpy(), mr), k
        assert np.array_equal(u32(o.cpu().numpy()), u32(obs)), k
        tt = t.cpu().numpy()
        assert np.array_equal(u32(tt[done]), u32(term[done])) and np.all(tt[~done] == np.float32(SENTINEL)), k
        st = norm.get_state()
        assert np.all(st.obs_rms.mean == 0) and np.all(st.obs_rms.var == 1) and st.obs_rms.count == 1e-4, k
        assert st.ret_rms.count == 1e-4 + (k + 1) * E
    before = norm.get_state()
    assert before.returns.any()
    x = ragged_batch(rng, E, D)
    assert np.array_equal(u32(norm.reset_torch(up(x)).cpu().numpy()), u32(x))
    after = norm.get_state()
    for a, b in ((before.obs_rms, after.obs_rms), (before.ret_rms, after.ret_rms)):
        assert np.array_equal(u64(a.mean), u64(b.mean)) and np.array_equal(u64(a.var), u64(b.var)) and a.count == b.count
    assert not after.returns.any()
    model.reset(x)
    check_stats(norm, model, "reset")
    norm.close()


def test_without_norm_reward_the_reward_passes_through():
    E, D, norm, model, rng = mode_pair(norm_reward=False)
    for k in range(6):
        obs, rew, done, term = ragged_step(rng, E, D)
        _, r = step_and_check(norm, model, obs, rew, done, term, k)
        assert np.array_equal(u64(r), u64(rew.astype(np.float32).astype(np.float64))), k
    assert norm.get_state().ret_rms.count == 1e-4 + 6 * E
    norm.close()


def test_evaluation_after_training_and_a_changed_epsilon():
    """Three training steps, then `training=False`: nothing moves any more but the returns.  Then `configure(epsilon=...)` between
    two steps: sd = sqrt(var + epsilon) must be derived again -- without training no finalize does it --, for the observations
    and for the reward."""
    E, D, norm, model, rng = mode_pair()
    norm.reset_torch(up(x := ragged_batch(rng, E, D)))
    model.reset(x)
    for k in range(3):
        step_and_check(norm, model, *ragged_step(rng, E, D), k)
    norm.configure(training=False)
    model.training = False
    frozen = norm.get_state()
    for k in range(3):
        step_and_check(norm, model, *ragged_step(rng, E, D), ("eval", k))
    st = norm.get_state()
    for a, b in ((frozen.obs_rms, st.obs_rms), (frozen.ret_rms, st.ret_rms)):
        assert np.array_equal(u64(a.mean), u64(b.mean)) and np.array_equal(u64(a.var), u64(b.var)) and a.count == b.count
    obs, rew, done, term = ragged_step(rng, E, D)
    old = norm.step_torch(up(obs), up(rew), up(done), up(term))
    model.step(obs, rew, done, term)
    norm.configure(epsilon=0.5)
    model.epsilon = 0.5
    o, r, t = norm.step_torch(up(obs), up(rew), up(done), up(term))
    mo, mr, mt = model.step(obs, rew, done, term)
    assert close_f32(o.cpu().numpy(), mo) and close_reward(r.cpu().numpy(), mr) and close_f32(t.cpu().numpy()[done], mt[done])
    # ... and the new epsilon shows: column 1 (variance 1e-2) shrinks by a factor of 7, the reward by sqrt(1 + 0.5 / var)
    assert not close_f32(o.cpu().numpy(), old[0].cpu().numpy()) and not close_reward(r.cpu().numpy(), old[1].cpu().numpy())
    norm.configure(training=True)
    model.training = True
    for k in range(2):
        step_and_check(norm, model, *ragged_step(rng, E, D), ("training again", k))
    norm.close()


# ---- f. through the env at small ragged sizes --------------------------------------------------------------------------------
def make_env(E, N, seed=5):
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv
    from fleetrl_amd.synth import synth_tables

    return FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=seed)


@pytest.mark.parametrize("E,N", [(1, 3), (65, 3), (300, 7)])
def test_through_the_env_at_small_ragged_sizes(E, N):
    """FleetVecNormalize(FleetVecEnv) past an episode boundary: the host path (NumPy in and out) against the model fed by an
    identically seeded plain env at every step, and `step_torch` byte-identical to the host path."""
    from fleetrl_amd import FleetVecNormalize

    steps = 192 + 30
    raw_env, env, env_t = make_env(E, N), make_env(E, N), make_env(E, N)
    vn, vt = FleetVecNormalize(env), FleetVecNormalize(env_t)
    D = env.core.obs_dim
    model = VecNormModel(E, D)
    ro = raw_env.reset()
    o = vn.reset()
    assert np.array_equal(vn.get_original_obs(), ro)
    assert close_f32(o, model.reset(ro))
    assert vt.reset_torch().cpu().numpy().tobytes() == o.tobytes()
    check_stats(vn.norm, model, "reset")
    term_t = torch.zeros((E, D), device=DEV)
    rng = np.random.default_rng(0)
    episodes = 0
    for k in range(steps):
        a = rng.uniform(-1, 1, size=(E, N)).astype(np.float32)
        ro, rr, rd, rinfo = raw_env.step(a)
        o, r, d, info = vn.step(a)
        assert np.array_equal(d, rd), k
        rterm = np.zeros_like(ro)
        for i in np.flatnonzero(rd):
            rterm[i] = rinfo[i]["terminal_observation"]
        mo, mr, mt = model.step(ro, rr, rd, rterm)
        assert close_f32(o, mo) and close_reward(r, mr), k
        for i in np.flatnonzero(rd):
            assert close_f32(info[i]["terminal_observation"], mt[i]), (k, i)
        check_stats(vn.norm, model, k)
        to, tr, td = vt.step_torch(up(a), terminal_out=term_t)
        assert to.cpu().numpy().tobytes() == o.tobytes() and tr.cpu().numpy().tobytes() == np.asarray(r, np.float64).tobytes(), k
        assert np.array_equal(td.cpu().numpy().astype(bool), d), k
        tt = term_t.cpu().numpy()
        for i in np.flatnonzero(rd):
            assert tt[i].tobytes() == np.asarray(info[i]["terminal_observation"], np.float32).tobytes(), (k, i)
        episodes += int(rd.sum())
    assert episodes >= E
    a, b = vn.norm.get_state(), vt.norm.get_state()
    for x, y in ((a.obs_rms.mean, b.obs_rms.mean), (a.obs_rms.var, b.obs_rms.var), (a.ret_rms.mean, b.ret_rms.mean),
                 (a.ret_rms.var, b.ret_rms.var), (a.returns, b.returns)):
        assert u64(x).tobytes() == u64(y).tobytes()
    assert a.obs_rms.count == b.obs_rms.count and a.ret_rms.count == b.ret_rms.count
    vn.close()
    vt.close()
    raw_env.close()
