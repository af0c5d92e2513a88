"""Correlated action noise on the device (fleet_noise_*, fleet_noise.hip) against the float64 model of tests/noise_model.py: the pink
sequences, what a row may depend on, the (t, q) state machine, checkpoints, the Ornstein-Uhlenbeck process, the way through
`DevicePolicy.explore`, the ensemble statistics at the benchmark's shape, and the refusals.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import explore_model as em
import noise_model as nm
import policy_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ES, ACTS = (1, 3, 65), (1, 2, 5, 50)
NOISE_BOUND = 1e-5  # |eps_dev - eps_model| of one Box-Muller normal, as test_explore_gpu.test_drawn_noise_equals_the_model states it
# |y_dev - y_model| of one pink sample: three times the largest device error measured over every case of
# test_pink_sequences_equal_the_model (PINK_MEASURED, on an MI355X: 5.47e-6, at n = 193), and below the worst case `pink_bound`
# derives for every case (3.9e-5 at n = 3 .. 1.1e-3 at n = 193)
PINK_MEASURED = 5.47e-6
PINK_TOL = 1.6e-5
# ... and of one OU sample after 50 calls, the same way (test_ou_equals_the_model: 5.32e-7 measured; `ou_bound` gives 2e-5 and more)
OU_MEASURED = 5.32e-7
OU_TOL = 1.6e-6


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def pink(E, A, n, beta=1.0, seed=nm.SEED, offset=0):
    from fleetrl_amd import DevicePinkNoise

    return DevicePinkNoise(E, A, n, beta=beta, seed=seed, env_id_offset=offset)


def run(proc, calls, done=None):
    """[calls, E, A] rows of `calls` calls of next; done: None or u8 [calls, E]."""
    out = torch.full((calls, proc.num_envs, proc.act_dim), 9.0, device=dev())
    d = None if done is None else on_device(np.asarray(done, np.uint8))
    for c in range(calls):
        proc.next(None if d is None else d[c], out=out[c])
    torch.cuda.synchronize()
    return out


def state(proc):
    s = proc.state_dict()
    return s["t"].cpu().numpy(), s["q"].cpu().numpy().view(np.uint32)


def pink_bound(n, beta):
    """Worst case of the float32 chain against the float64 sum over the same float32 tables, per sample: every coefficient off by
    NOISE_BOUND (2K coefficients, each times a gain and a |cos| or |sin| <= 1); the staged product and the fused multiply-add round
    once each, 2^-24 relative, on terms of at most gain x 5.77 and on partial sums of at most sqrt(2) x 5.77 x sum(gain)."""
    g = nm.tables32(n, beta)[0].astype(np.float64)
    K, z = len(g), em.EPS_MAX
    return 2 * NOISE_BOUND * g.sum() + 2.0 ** -24 * z * g.sum() * (2 + 2 * K * np.sqrt(2.0))


# ---- 1. the sequences against the model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nm.NS)
def test_pink_sequences_equal_the_model(n):
    """n + 2 calls (the wrap-around is crossed) at every E, A and beta, against the model's float64 sum over the float32 tables.
    The tolerance is PINK_TOL = 1.6e-5, three times the largest error measured on the device (5.47e-6 at n = 193; 2.6e-6 at n = 2,
    1.3e-6 at n = 7, 3.0e-6 at n = 64, 5.2e-6 at n = 192), and never above `pink_bound`: Box-Muller's ~3e-6 per coefficient adds up
    in quadrature over the 2K terms weighted by the gains (sum gain^2 ~ 1), the 2K roundings of the chain likewise."""
    worst, case = 0.0, 0
    for beta in nm.BETAS:
        bound = pink_bound(n, beta)
        for E in ES:
            for A in ACTS:
                offset = (0, 5, 2 ** 31 - 70)[case % 3]
                case += 1
                proc = pink(E, A, n, beta, offset=offset)
                got = run(proc, n + 2).cpu().numpy().astype(np.float64)
                model = nm.PinkModel(E, A, n, beta, env_id_offset=offset)
                want = np.stack([model.next() for _ in range(n + 2)])
                err = float(np.abs(got - want).max())
                worst = max(worst, err)
                t, q = state(proc)
                assert np.array_equal(t, model.t) and np.array_equal(q, model.q) and q.tolist() == [1] * E and t.tolist() == [2] * E
                assert PINK_TOL <= bound and err <= PINK_TOL, (n, beta, E, A, err, bound)
                assert proc.describe()["cache_bytes"] == E * n * A * 4
                proc.close()
    print(f"n={n}: max |y_dev - y_model| {worst:.3g}; worst-case bounds {[float(f'{pink_bound(n, b):.3g}') for b in nm.BETAS]}")


# ---- 2. what a row depends on -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,n", [(5, 7), (50, 65), (3, 192)])
def test_a_row_depends_on_seed_env_id_column_and_its_own_history_bit_for_bit(A, n):
    E, calls = 65, n + 3
    rng = np.random.default_rng(n)
    done = (rng.random((calls, E)) < 0.1).astype(np.uint8)
    done[2] = 1  # one call in which every env regenerates
    full = bits(run(pink(E, A, n), calls, done))
    assert (full != bits(torch.full((1,), 9.0))[0]).all()
    # a shard with env_id_offset, and an env alone
    assert np.array_equal(bits(run(pink(21, A, n, offset=16), calls, done[:, 16:37])), full[:, 16:37])
    for g in (0, 36, 64):
        assert np.array_equal(bits(run(pink(1, A, n, offset=g), calls, done[:, g:g + 1])), full[:, g:g + 1]), g
    # the same env with other envs regenerating at other times, or never
    g = 11
    for others in (0, 1):
        d = np.full_like(done, others)
        d[:, g] = done[:, g]
        assert np.array_equal(bits(run(pink(E, A, n), calls, d))[:, g], full[:, g]), others
    # on another stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        proc = pink(E, A, n)
        assert np.array_equal(bits(run(proc, calls, done)), full)
    side.synchronize()
    assert np.array_equal(bits(run(proc, 1)), bits(run(pink(E, A, n), calls + 1, np.concatenate([done, np.zeros((1, E), np.uint8)])))[-1:])
    # another seed, another sequence number: other rows
    assert not np.array_equal(bits(run(pink(E, A, n, seed=nm.SEED + 1), 1)), full[:1])
    assert not np.array_equal(full[0], full[2])


# ---- 3. the state machine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,A,n", [(5, 3, 7), (4, 50, 12)])
def test_staggered_done_flags_follow_the_models_state_machine(E, A, n):
    calls = 2 * n
    done = np.zeros((calls, E), np.uint8)
    for e in range(E - 1):  # env e is done at call 3e + 1; the last env never is
        done[3 * e + 1, e] = 1
    proc, model = pink(E, A, n), nm.PinkModel(E, A, n)
    for c in range(calls):
        got = proc.next(on_device(done[c])).cpu().numpy()
        want = model.next(done[c])
        t, q = state(proc)
        assert np.array_equal(t, model.t) and np.array_equal(q, model.q), c
        assert np.abs(got - want).max() <= PINK_TOL, c
    assert model.q[-1] == 1 and model.q[0] == 2  # the wrap alone; a done flag and later the wrap
    if n == 7:
        assert model.q[2] == 1  # done and used up in the same call (call 7): one new sequence, not two
    # reset(mask) is next(done=mask) without the row
    mask = (np.arange(E) % 2).astype(np.uint8)
    twin = pink(E, A, n)
    twin.load_state_dict(proc.state_dict())
    proc.reset(on_device(mask))
    model.reset(mask)
    t, q = state(proc)
    assert np.array_equal(t, model.t) and np.array_equal(q, model.q) and (t[1::2] == 0).all()
    assert np.array_equal(bits(proc.next()), bits(twin.next(on_device(mask))))
    model.next()
    for other in (state(twin), (model.t, model.q)):
        assert all(np.array_equal(a, b) for a, b in zip(state(proc), other))
    proc.reset()
    model.reset()
    t, q = state(proc)
    assert t.tolist() == [0] * E and np.array_equal(q, model.q)
    proc.close(), twin.close()


# ---- 4. checkpoints ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pink", "ou"])
def test_a_loaded_state_continues_the_stream_bit_for_bit(kind):
    from fleetrl_amd import DeviceOUNoise

    E, A, n, k = 17, 5, 12, 8

    def make():
        return pink(E, A, n) if kind == "pink" else DeviceOUNoise(E, A, mu=0.1, sigma=np.linspace(0.2, 0.6, A), seed=nm.SEED, env_id_offset=3)

    rng = np.random.default_rng(2)
    done = (rng.random((k + n + 1, E)) < 0.15).astype(np.uint8)
    first = make()
    run(first, k, done[:k])
    saved = first.state_dict()
    want = bits(run(first, n + 1, done[k:]))
    fresh = make()
    run(fresh, 2)  # (a fresh handle that has moved: the loaded state replaces all of it)
    fresh.load_state_dict({key: (v.clone() if isinstance(v, torch.Tensor) else v) for key, v in saved.items()})
    assert np.array_equal(bits(run(fresh, n + 1, done[k:])), want)
    assert saved["calls"] == (0 if kind == "pink" else k)
    with pytest.raises(ValueError):
        fresh.load_state_dict({**saved, "kind": "ou" if kind == "pink" else "pink"})
    first.close(), fresh.close()


# ---- 5. Ornstein-Uhlenbeck ----------------------------------------------------------------------------------------------------------
def ou_bound(model_abs_max, ss_max, calls):
    """Per call the error of x grows by at most ss x NOISE_BOUND (the draw) plus three float32 roundings (the difference and the
    two fused multiply-adds) at the magnitude of x; the recursion's factor 1 - theta dt <= 1 does not amplify what is there."""
    return calls * (ss_max * NOISE_BOUND + 3 * 2.0 ** -24 * max(model_abs_max, 1e-3))


def test_ou_equals_the_model():
    """50 calls with done flags at every E and A; OU_TOL = 1.6e-6 is three times the largest error measured on the device (5.32e-7),
    and never above `ou_bound`."""
    from fleetrl_amd import DeviceOUNoise

    calls, worst, case = 50, 0.0, 0
    for E in ES:
        for A in ACTS:
            offset = (0, 5, 2 ** 31 - 70)[case % 3]
            case += 1
            rng = np.random.default_rng(100 * E + A)
            mu, sigma = rng.uniform(-0.2, 0.2, A), rng.uniform(0.2, 0.8, A)
            theta, dt = (0.15, 1e-2) if case % 2 else (1.5, 0.25)
            done = (rng.random((calls, E)) < 0.1).astype(np.uint8)
            proc = DeviceOUNoise(E, A, mu=mu, sigma=sigma, theta=theta, dt=dt, seed=nm.SEED, env_id_offset=offset)
            got = run(proc, calls, done).cpu().numpy().astype(np.float64)
            model = nm.OUModel(E, A, mu, sigma, theta, dt, env_id_offset=offset)
            want = np.stack([model.next(done[c]) for c in range(calls)])
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            bound = ou_bound(float(np.abs(want).max()), float(model.ss.max()), calls)
            assert OU_TOL <= bound and err <= OU_TOL, (E, A, err, bound)
            s = proc.state_dict()
            assert s["calls"] == calls and np.array_equal(s["x"].cpu().numpy(), got[-1].astype(np.float32))
            proc.reset(on_device((np.arange(E) % 2).astype(np.uint8)))
            x = proc.state_dict()["x"].cpu().numpy()
            assert not x[1::2].any() and np.array_equal(x[0::2], got[-1, 0::2].astype(np.float32))
            proc.reset()
            assert not proc.state_dict()["x"].any() and proc.state_dict()["calls"] == calls
            proc.close()
    print(f"OU: max |x_dev - x_model| after {calls} calls {worst:.3g}")


# ---- 6. through explore -----------------------------------------------------------------------------------------------------------
def make_policy(D, A, seed=0):
    from fleetrl_amd import DevicePolicy

    rng = np.random.default_rng(1000 * seed + 7 * D + A)
    return DevicePolicy(pm.random_layers(rng, (D, 64, A)), activation="relu", output="tanh")


@pytest.mark.parametrize("kind,E,A", [("pink", 17, 5), ("pink", 37, 50), ("ou", 17, 5)])
def test_explore_with_a_process_is_the_given_noise_path(kind, E, A):
    from fleetrl_amd import DeviceOUNoise

    D, n, lo, hi = 45, 6, -0.5, 0.75
    pol = make_policy(D, A)
    sigma = np.random.default_rng(A).uniform(0.2, 0.6, A).astype(np.float32) if kind == "pink" else np.ones(A, np.float32)
    shift = np.random.default_rng(A + 1).uniform(-0.1, 0.1, A).astype(np.float32)

    def make():
        return pink(E, A, n) if kind == "pink" else DeviceOUNoise(E, A, sigma=0.5, seed=nm.SEED)

    proc, twin = make(), make()
    model = nm.PinkModel(E, A, n) if kind == "pink" else nm.OUModel(E, A, 0.0, 0.5)
    eps_tol = PINK_TOL if kind == "pink" else OU_TOL
    rng = np.random.default_rng(E)
    for c in range(n + 2):
        x = on_device(np.clip(rng.standard_normal((E, D)) * 3, -10, 10).astype(np.float32))
        done = on_device((rng.random(E) < 0.2).astype(np.uint8))
        d, eps = torch.empty((E, A), device=dev()), torch.empty((E, A), device=dev())
        a, env, lp, _ = pol.explore(x, on_device(sigma), shift=on_device(shift), low=lo, high=hi, action_noise=proc, done=done, mean_out=d,
                                    noise=eps)
        given = twin.next(done)
        b, env_b, _, _ = pol.explore(x, on_device(sigma), shift=on_device(shift), low=lo, high=hi, seed=0, step=0, noise=given, noise_given=True)
        assert lp is None and np.array_equal(bits(a), bits(b)) and np.array_equal(bits(env), bits(env_b)) and np.array_equal(bits(a), bits(env))
        assert np.array_equal(bits(eps), bits(given))
        want_eps = model.next(done.cpu().numpy())
        assert np.abs(eps.cpu().numpy() - want_eps).max() <= eps_tol
        want = em.action_noise(d.cpu().numpy(), sigma, shift, want_eps, lo, hi)
        # three float32 roundings at magnitudes below 8 (test_explore_gpu), and sigma <= 1 times the error of eps
        assert np.abs(a.cpu().numpy() - want).max() <= 3 * 2.0 ** -24 * 8 + eps_tol
    with pytest.raises(ValueError):
        pol.explore(x, 0.1, action_noise=proc, noise=given, noise_given=True)
    with pytest.raises(TypeError):
        pol.explore(x, 0.1)
    pol.close(), proc.close(), twin.close()


def test_env_actions_from_pink_noise_are_accepted_by_step_torch():
    from bench import bench_config

    from fleetrl_amd import DevicePolicy, FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    E, N = 17, 5
    env = FleetVecNormalize(FleetVecEnv(dict(bench_config(E, N, "ct"), episode_length=24), E, tables=synth_tables("ct", N, seed=3), seed=1))
    D, n = env.norm.D, int(env.venv.core.params.episode_steps)  # 24 hours of 15-minute steps
    pol = DevicePolicy(pm.random_layers(np.random.default_rng(8), (D, 64, 64, N)), activation="relu", output="tanh")
    proc = pink(E, N, n)  # the reference's recipe: seq_len = the episode's steps
    obs, reward, done = torch.empty((E, D), device=dev()), torch.empty(E, device=dev(), dtype=torch.float64), torch.zeros(E, device=dev(), dtype=torch.uint8)
    env.reset_torch(obs_out=obs)
    flags = []
    for _ in range(n + 4):  # past the episode's end: the env's done flags restart the process
        flags.append(done.clone())
        _, env_a, _, _ = pol.explore(obs, 0.3, action_noise=proc, done=done)
        env.step_torch(env_a, obs_out=obs, reward_out=reward, done_out=done)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(reward).all()) and float(env_a.abs().max()) <= 1.0
    t, q = np.zeros(E, np.int32), np.zeros(E, np.uint32)
    for f in flags:  # the state machine on the flags the env gave
        again = (t >= n) | f.cpu().numpy().astype(bool)
        q[again] += 1
        t[again] = 0
        t += 1
    got_t, got_q = state(proc)
    assert np.array_equal(got_t, t) and np.array_equal(got_q, q) and q.min() >= 1 and n == 96
    assert sum(int(f.sum()) for f in flags) == E  # every env ended one episode inside the loop
    pol.close(), proc.close(), env.close()


# ---- 7. statistics ------------------------------------------------------------------------------------------------------------------
def test_the_ensemble_of_one_fill_has_the_tables_moments():
    """4096 x 50 at n = 192: one fill is N = 204800 independent sequences.  Every bound is 5 standard errors of the model's exact
    value: mean 1 / sqrt(N); variance sqrt(2 / N) around sum gain^2; correlation (1 - rho^2) / sqrt(N) around the tables' rho;
    periodogram sd / sqrt(N) with sd = E|Y_k|^2 inside (chi^2_2) and sqrt(2) E|Y_k|^2 at 2k = n (chi^2_1)."""
    E, A, n = em.STAT_SHAPE + (192,)
    N = E * A
    ks = [1, 2, 8, 48, 96]
    proc = pink(E, A, n, 1.0)
    ang = 2.0 * np.pi * np.outer(np.arange(n), ks) / n
    cos, sin = on_device(np.cos(ang)), on_device(np.sin(ang))
    re, im = torch.zeros((len(ks), E, A), device=dev(), dtype=torch.float64), torch.zeros((len(ks), E, A), device=dev(), dtype=torch.float64)
    keep = {}
    for t in range(n):
        y = proc.next().double()
        re += cos[t][:, None, None] * y
        im -= sin[t][:, None, None] * y
        if t in (10, 11):
            keep[t] = y.cpu().numpy()
    power = (re ** 2 + im ** 2).mean(dim=(1, 2)).cpu().numpy()
    t_, q_ = state(proc)
    assert t_.tolist() == [n] * E and not q_.any()
    proc.close()
    var, rho = nm.variance(n, 1.0), nm.correlation(n, 1.0, 1)
    want, sd = nm.periodogram_expectation(n, 1.0)
    got = {"mean": float(keep[10].mean()), "var": float(keep[10].var()), "corr": em.lag1(keep[10], keep[11]), "power": power.tolist()}
    print(got, {"var": var, "rho": rho, "power": want[ks].tolist()})
    assert var > 1.0 and 0.0 < rho < 1.0
    assert abs(got["mean"]) <= 5 / np.sqrt(N)
    assert abs(got["var"] - var) <= 5 * np.sqrt(2 / N)
    assert abs(got["corr"] - rho) <= 5 * (1 - rho ** 2) / np.sqrt(N)
    assert np.all(np.abs(power - want[ks]) <= 5 * sd[ks] / np.sqrt(N)), (power, want[ks])
    # beta = 0: white
    white = pink(E, A, n, 0.0)
    rows = run(white, 12).cpu().numpy().astype(np.float64)
    white.close()
    c0 = em.lag1(rows[10], rows[11])
    print({"white_corr": c0, "white_var": float(rows[10].var()), "want_var": nm.variance(n, 0.0)})
    assert abs(c0) <= 5 / np.sqrt(N) and abs(rows[10].var() - nm.variance(n, 0.0)) <= 5 * np.sqrt(2 / N)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_reason_and_launch_nothing():
    from fleetrl_amd import DeviceOUNoise, FleetHipError, _capi

    lib = _capi.load_library()
    A = 5
    mu, sigma = np.zeros(A), np.full(A, 0.5)

    def params(**over):
        p = _capi.FleetNoiseParams()
        p.struct_bytes, p.kind, p.num_envs, p.act_dim, p.seq_len, p.beta, p.seed = C.sizeof(p), _capi.NOISE_PINK, 8, A, 12, 1.0, 3
        p.theta, p.dt, p.mu, p.sigma = 0.15, 1e-2, mu.ctypes.data, sigma.ctypes.data
        for k, v in over.items():
            setattr(p, k, v)
        return p

    nan, inf, OU = float("nan"), float("inf"), _capi.NOISE_OU
    bad_mu, bad_sigma = np.array([0, 0, nan, 0, 0.0]), np.array([0.5, inf, 0.5, 0.5, 0.5])
    cases = [(params(struct_bytes=8), "struct_bytes"), (params(kind=2), "kind"), (params(kind=-1), "kind"), (params(num_envs=0), "num_envs"),
             (params(act_dim=0), "act_dim"), (params(act_dim=513), "act_dim"), (params(seq_len=1), "seq_len"), (params(seq_len=4097), "seq_len"),
             (params(beta=-0.5), "beta"), (params(beta=nan), "beta"), (params(env_id_offset=-1), "env_id_offset"),
             (params(kind=OU, theta=nan), "theta"), (params(kind=OU, dt=inf), "dt"), (params(kind=OU, dt=-1.0), "dt"),
             (params(kind=OU, mu=bad_mu.ctypes.data), "mu"), (params(kind=OU, sigma=bad_sigma.ctypes.data), "sigma"),
             (params(kind=OU, mu=None), "null mu"), (params(num_envs=2 ** 31 - 1, act_dim=512, seq_len=4096), "too large")]
    for p, word in cases:
        h = C.c_void_p()
        assert lib.fleet_noise_create(0, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h, word
        why = lib.fleet_noise_last_error(None).decode()
        assert why.startswith("fleet_noise_create: ") and word in why, (word, why)
    assert lib.fleet_noise_create(0, None, C.byref(C.c_void_p())) == _capi.ERR_INVALID
    with pytest.raises(FleetHipError):
        pink(4, 3, 1)
    # a live handle: a null eps_out, positions outside 0..n
    proc, twin = pink(8, A, 12), pink(8, A, 12)
    run(proc, 3), run(twin, 3)
    assert lib.fleet_noise_next_dev(proc.h, None, None) == _capi.ERR_INVALID
    assert lib.fleet_noise_last_error(proc.h).decode().startswith("fleet_noise_next_dev: null eps_out")
    s = proc.state_dict()
    for bad in (-1, 13):
        t = s["t"].clone()
        t[5] = bad
        with pytest.raises(FleetHipError) as ei:
            proc.load_state_dict({**s, "t": t})
        assert ei.value.status == _capi.ERR_INVALID and "fleet_noise_set_state_dev: t of env 5" in str(ei.value)
    assert lib.fleet_noise_set_state_dev(proc.h, None, s["q"].data_ptr(), None, 0) == _capi.ERR_INVALID
    assert lib.fleet_noise_last_error(proc.h).decode().startswith("fleet_noise_set_state_dev: ")
    assert lib.fleet_noise_get_state_dev(proc.h, None, None, None, None) == _capi.ERR_INVALID
    assert lib.fleet_noise_last_error(proc.h).decode().startswith("fleet_noise_get_state_dev: ")
    t = s["t"].clone()
    t[0] = 12  # n itself is a position: the next call wraps
    proc.load_state_dict({**s, "t": t})
    proc.load_state_dict(s)
    # nothing of the refused calls happened: the state and the next rows are the twin's
    assert all(np.array_equal(a, b) for a, b in zip(state(proc), state(twin)))
    assert np.array_equal(bits(run(proc, 2)), bits(run(twin, 2)))
    ou = DeviceOUNoise(8, A, sigma=0.5, seed=1)
    assert lib.fleet_noise_set_state_dev(ou.h, None, None, None, 0) == _capi.ERR_INVALID
    with pytest.raises(ValueError):
        proc.next(out=torch.empty((8, A + 1), device=dev()))
    with pytest.raises(ValueError):
        proc.next(done=torch.zeros(7, device=dev(), dtype=torch.uint8))
    proc.close(), twin.close(), ou.close()
