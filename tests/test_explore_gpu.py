"""Exploration on the device (fleet_explore_act_dev, fleet_policy.hip) against the float64 model of tests/explore_model.py: the drawn
noise, what a row may depend on, the mean against the deterministic forward, the arithmetic on given noise, the log-probability,
the action-noise and uniform modes, sampling into a rollout slot, the refusals, and the moments of the noise.  Needs an MI355X."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import explore_model as em
import policy_bits as pb
import policy_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(pm.ROOT, "profiles", "explore_parity.json")
_parity = {}
ES = (1, 15, 16, 17, 37)  # around the 16-row tile
ACTS = (1, 3, 4, 5, 50, 63, 64, 65, 130, 512)  # the 4-column Philox block, the 64-column group, a sum that crosses wavefronts
SEEDS = (em.SEED, 3, (1 << 63) | 12345)
STEPS = (0, 1, 2 ** 32 - 1, 2 ** 32)


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def write_parity():
    """The figures are printed; they go to profiles/explore_parity.json only when FLEET_WRITE_PARITY=1 asks for it (a test run leaves
    the tree as it found it), merged into the cases the file already holds so that a partial run does not drop the others."""
    if os.environ.get("FLEET_WRITE_PARITY") != "1":
        return
    cases = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as fh:
            cases = json.load(fh).get("cases", {})
    cases.update(_parity)
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as fh:
        json.dump({"noise_bound": 1e-5, "log_prob_bound": "8 * max(eps_ref, 2^-24 * max|log_prob|)", "cases": dict(sorted(cases.items()))},
                  fh, indent=1)
        fh.write("\n")


def layers_for(kind, D, A, seed=0):
    """one: a one-layer head; tanh: D-64-64-A; relu: D-130-70-A (wider than 64).  (actor, critic, activation)"""
    rng = np.random.default_rng(1000 * seed + 7 * D + A)
    sizes = {"one": (D, A), "tanh": (D, 64, 64, A), "relu": (D, 130, 70, A)}[kind]
    actor = pm.random_layers(rng, sizes)
    critic = pm.random_layers(rng, sizes[:-1] + (1,))
    return actor, critic, "relu" if kind == "relu" else "tanh"


def make_policy(kind, D, A, output="clip", critic=True, seed=0, scale_last=1.0, low=-1.0, high=1.0):
    from fleetrl_amd import DevicePolicy

    actor, crit, activation = layers_for(kind, D, A, seed)
    actor[-1] = ((actor[-1][0] * np.float32(scale_last)).astype(np.float32), actor[-1][1])
    return DevicePolicy(actor, critic_layers=crit if critic else None, activation=activation, output=output, low=low, high=high)


def observations(E, D, seed=0):
    return on_device(np.clip(np.random.default_rng(77 + seed + 13 * E + D).standard_normal((E, D)) * 3, -10, 10).astype(np.float32))


def normalizer_for(E, D):
    from fleetrl_amd import DeviceNormalizer

    norm = DeviceNormalizer(E, D, clip_obs=4.0)
    gen = torch.Generator(device=dev())
    gen.manual_seed(D)
    rew, done = torch.zeros(E, device=dev(), dtype=torch.float64), torch.zeros(E, device=dev(), dtype=torch.uint8)
    for _ in range(3):
        norm.step_torch(torch.randn((E, D), device=dev(), generator=gen) * 3 + 1, rew, done)
    norm.configure(training=False)
    return norm


# ---- 1. the noise against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ACTS)
def test_drawn_noise_equals_the_model(A):
    """|eps_dev - eps_model| <= 1e-5 absolute: the float32 angle 2 pi u2 carries <= ~5e-7 rad of rounding, times r <= 5.77 that is
    ~3e-6, plus a few ulp of logf, sqrtf, sinf and cosf at the device library's <= 2 ulp: about 3x margin."""
    pol = make_policy("one", 7, A, critic=False)
    worst, case = 0.0, 0
    for seed in SEEDS:
        for step in STEPS:
            E, offset = ES[case % len(ES)], (0, 5, 2 ** 31 - 40)[case % 3]
            case += 1
            noise = torch.full((E, A), 9.0, device=dev())
            pol.sample(observations(E, 7), 0.0, seed=seed, step=step, env_id_offset=offset, noise=noise)
            want = em.normals(seed, np.arange(E) + offset, A, step)
            err = float(np.abs(noise.cpu().numpy().astype(np.float64) - want).max())
            worst = max(worst, err)
            assert err <= 1e-5, (seed, step, E, offset, err)
    _parity[f"noise/A{A}"] = {"max_abs_err": worst}
    print(f"A={A}: max |eps_dev - eps_model| {worst:.3g}")
    write_parity()
    pol.close()


# ---- 2. what a row depends on -----------------------------------------------------------------------------------------------------
def _run(pol, x, log_std, offset, values=True, noise=True, step=11):
    E, A = x.shape[0], pol.act_dim
    eps = torch.full((E, A), 9.0, device=dev()) if noise else None
    val = torch.full((E, 1), 9.0, device=dev()) if values else None
    a, env, lp, _ = pol.sample(x.contiguous(), log_std, seed=em.SEED, step=step, env_id_offset=offset, values_out=val, noise=eps)
    torch.cuda.synchronize()
    out = {"actions": bits(a), "env_actions": bits(env), "log_prob": bits(lp)}
    if values:
        out["values"] = bits(val)
    if noise:
        out["eps"] = bits(eps)
    return out


def _same(got, want, rows=slice(None), keys=None):
    for k in keys or want:
        assert np.array_equal(got[k], want[k][rows]), k


@pytest.mark.parametrize("kind,A", [("tanh", 5), ("relu", 65), ("one", 512)])
def test_a_row_depends_on_seed_env_id_step_and_column_and_on_nothing_else(kind, A):
    D = 45
    pol = make_policy(kind, D, A, scale_last=3.0)
    x = observations(37, D)
    log_std = on_device(np.random.default_rng(A).uniform(-1.0, 0.5, A).astype(np.float32))
    full = _run(pol, x, log_std, 0)
    assert (full["eps"] != bits(torch.full((1,), 9.0))[0]).all() and (full["values"] != bits(torch.full((1,), 9.0))[0]).all()
    # E = 37 at offset 0 against E = 16 at offset 0 and E = 21 at offset 16
    _same(_run(pol, x[:16], log_std, 0), full, slice(0, 16))
    _same(_run(pol, x[16:], log_std, 16), full, slice(16, 37))
    # alone, and anywhere in a batch
    for r in (0, 15, 16, 36):
        _same(_run(pol, x[r:r + 1], log_std, r), full, slice(r, r + 1))
    _same(_run(pol, x[10:30], log_std, 10), full, slice(10, 30))
    perm = np.random.default_rng(1).permutation(37)
    moved = _run(pol, x[on_device(perm)], log_std, 0)  # other rows under the same env ids: the noise stays, the means move
    assert np.array_equal(moved["eps"], full["eps"]) and np.array_equal(moved["values"], full["values"][perm])
    # on another stream
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _same(_run(pol, x, log_std, 0), full)
    side.synchronize()
    _same(_run(pol, x, log_std, 0), full)
    # with and without the critic's launch half, with and without the noise written
    _same(_run(pol, x, log_std, 0, values=False), full, keys=("actions", "env_actions", "log_prob", "eps"))
    _same(_run(pol, x, log_std, 0, noise=False), full, keys=("actions", "env_actions", "log_prob", "values"))
    # another step gives other noise
    assert not np.array_equal(_run(pol, x, log_std, 0, step=12)["eps"], full["eps"])
    # after load_host against after load_torch
    actor, critic, _ = layers_for(kind, D, A)
    actor[-1] = ((actor[-1][0] * np.float32(3.0)).astype(np.float32), actor[-1][1])
    host, devp = make_policy(kind, D, A, seed=5), make_policy(kind, D, A, seed=6)
    host.load_host(actor, critic)
    devp.load_torch([on_device(a) for pair in actor + critic for a in pair])
    _same(_run(host, x, log_std, 0), full)
    _same(_run(devp, x, log_std, 0), full)
    for p in (pol, host, devp):
        p.close()


# ---- 3. the mean ----------------------------------------------------------------------------------------------------------------
MEAN_CASES = [("one", 129, 1, True), ("one", 129, 3, False), ("one", 45, 4, False), ("one", 129, 64, True), ("one", 129, 512, True),
              ("tanh", 45, 5, False), ("tanh", 45, 50, False), ("tanh", 45, 65, False), ("tanh", 129, 63, True),
              ("relu", 129, 130, True), ("relu", 45, 512, False), ("relu", 129, 5, True)]


@pytest.mark.parametrize("kind,D,A,with_norm", MEAN_CASES)
def test_mean_is_the_deterministic_forward_bit_for_bit(kind, D, A, with_norm):
    """GAUSSIAN: the forward of the same weights built with output "none".  ACTION_NOISE: with output "tanh"."""
    sampler, plain = make_policy(kind, D, A, output="clip"), make_policy(kind, D, A, output="none")
    tanh = make_policy(kind, D, A, output="tanh")
    norm = normalizer_for(8, D) if with_norm else None
    for E in ES:
        x = observations(E, D)
        for critic in (False, True):
            mean = torch.full((E, A), 9.0, device=dev())
            val = torch.full((E, 1), 9.0, device=dev()) if critic else None
            sampler.sample(x, -0.5, seed=1, step=E, normalizer=norm, mean_out=mean, values_out=val)
            want_v = torch.empty((E, 1), device=dev())
            want = plain.act(x, normalizer=norm, values_out=want_v)
            assert np.array_equal(bits(mean), bits(want)), (E, critic)
            if critic:
                assert np.array_equal(bits(val), bits(want_v)), E
            d = torch.full((E, A), 9.0, device=dev())
            tanh.explore(x, 0.1, seed=1, step=E, normalizer=norm, mean_out=d, values_out=val)
            assert np.array_equal(bits(d), bits(tanh.act(x, normalizer=norm))), (E, critic)
    if norm is not None:
        norm.close()
    for p in (sampler, plain, tanh):
        p.close()


# ---- 4. given noise ---------------------------------------------------------------------------------------------------------------
def _given_eps(E, A, seed):
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal((E, A)).astype(np.float32)
    special = np.array([0.0, 1.0, -1.0, 5.77, -5.77], np.float32)
    flat = eps.reshape(-1)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    if E > 1:
        eps[-1, :] = special[np.arange(A) % special.size]
    return eps


@pytest.mark.parametrize("E,A", [(1, 1), (15, 3), (16, 4), (17, 5), (37, 50), (17, 63), (16, 64), (15, 65), (17, 130), (37, 512)])
def test_given_noise_goes_through_one_fma_and_the_heads_clip(E, A):
    lo, hi = -0.3, 0.7
    pol = make_policy("one", 45, A, critic=False, scale_last=2.0, low=lo, high=hi)
    x = observations(E, 45)
    eps = _given_eps(E, A, A)
    mean = torch.empty((E, A), device=dev())
    a, env, _, _ = pol.sample(x, torch.zeros(A, device=dev()), seed=0, step=0, noise=on_device(eps), noise_given=True, mean_out=mean)
    m = mean.cpu().numpy()
    want = pb.fma32(np.float32(1), eps, m)  # log_std = 0: std is exactly 1
    assert pb.same_bits(a.cpu().numpy(), want)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    clipped = np.where(want < lo32, lo32, np.where(want > hi32, hi32, want))
    assert pb.same_bits(env.cpu().numpy(), clipped)
    if E * A >= 15:
        inside = (want >= lo32) & (want <= hi32)
        assert inside.any() and (~inside).any()
        if E > 1 and A > 1:
            assert (inside.any(axis=1) & (~inside).any(axis=1)).any()  # a partly saturating row
    # random log_std in [-3, 1]: std = expf(log_std) may be 2 ulp off, which moves std * eps by 2 ulp of it; one more rounding of
    # the sum: within 4 ulp at the magnitude of max(|a|, |std * eps|).  (Not 4 ulp of the result alone: where mean ~ -std * eps the
    # sum cancels, and the 2 ulp of expf, which are ulps of std * eps, are many ulps of the small result -- no float32 evaluation
    # with a 2-ulp expf can meet that, so the bound is taken at the larger of the two magnitudes.)
    log_std = np.random.default_rng(A + 1).uniform(-3, 1, A).astype(np.float32)
    a2, _, _, _ = pol.sample(x, on_device(log_std), seed=0, step=0, noise=on_device(eps), noise_given=True)
    std = np.exp(log_std.astype(np.float64)).astype(np.float32)
    want2 = pb.fma32(std, eps, m)
    tol = 4 * np.spacing(np.maximum(np.abs(want2), np.abs(std * eps)).astype(np.float32))
    assert (np.abs(a2.cpu().numpy().astype(np.float64) - want2.astype(np.float64)) <= tol).all()
    pol.close()


# ---- 5. the log-probability -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 5, 65, 512])
def test_log_prob_stays_within_eight_times_the_float32_reference_error(A):
    """On the returned actions, mean and log_std: the float64 Normal(mean, std).log_prob(a).sum(-1), and the project's bound
    8 * max(eps_ref, 2^-24 * max |log_prob|), eps_ref torch-CPU float32's distance from the same model."""
    pol = make_policy("tanh", 45, A)
    log_std = np.random.default_rng(A).uniform(-3, 1, A).astype(np.float32)
    failures = []
    for E in ES:
        x = observations(E, 45)
        mean = torch.empty((E, A), device=dev())
        a, _, lp, _ = pol.sample(x, on_device(log_std), seed=em.SEED, step=E, mean_out=mean)
        a, m, lp = a.cpu().numpy(), mean.cpu().numpy(), lp.cpu().numpy().astype(np.float64)
        lp64 = em.log_prob64(a, m, log_std)
        eps_ref = float(np.abs(em.log_prob_torch32(a, m, log_std).astype(np.float64) - lp64).max())
        err = float(np.abs(lp - lp64).max())
        bound = 8 * max(eps_ref, 2.0 ** -24 * float(np.abs(lp64).max()))
        _parity[f"log_prob/A{A}/E{E}"] = {"eps_ref": eps_ref, "device_err": err, "bound": bound, "err_over_bound": err / bound}
        print(f"A={A} E={E}: eps_ref {eps_ref:.3g} device {err:.3g} bound {bound:.3g} ratio {err / bound:.3g}")
        if not err <= bound:
            failures.append((E, err, bound))
    write_parity()
    pol.close()
    assert not failures, failures


# ---- 6. action noise and the uniform warm-up --------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,A", [(1, 1), (17, 5), (37, 65), (16, 130)])
def test_action_noise_follows_the_model_and_hits_the_clip_exactly(E, A):
    lo, hi = -0.5, 0.75
    pol = make_policy("relu", 45, A, output="tanh", critic=False, scale_last=2.0)
    x = observations(E, 45)
    sigma = np.random.default_rng(A).uniform(0.2, 0.6, A).astype(np.float32)
    shift = np.random.default_rng(A + 1).uniform(-0.1, 0.1, A).astype(np.float32)
    d, eps = torch.empty((E, A), device=dev()), torch.empty((E, A), device=dev())
    a, env, lp, _ = pol.explore(x, on_device(sigma), shift=on_device(shift), low=lo, high=hi, seed=em.SEED, step=3, mean_out=d, noise=eps)
    assert lp is None and np.array_equal(bits(a), bits(env))
    got = a.cpu().numpy()
    assert np.abs(eps.cpu().numpy() - em.normals(em.SEED, np.arange(E), A, 3)).max() <= 1e-5
    want = em.action_noise(d.cpu().numpy(), sigma, shift, eps.cpu().numpy(), lo, hi)
    # three float32 roundings (sigma * eps, + shift, + d) at magnitudes up to 1 + 0.1 + 0.6 * 5.77 < 8
    assert np.abs(got - want).max() <= 3 * 2.0 ** -24 * 8
    raw = em.action_noise(d.cpu().numpy(), sigma, shift, eps.cpu().numpy(), -np.inf, np.inf)
    assert (got[raw > hi + 1e-3] == np.float32(hi)).all() and (got[raw < lo - 1e-3] == np.float32(lo)).all()
    assert got.min() >= np.float32(lo) and got.max() <= np.float32(hi)
    if E * A >= 85:
        assert (raw > hi + 1e-3).any() and (raw < lo - 1e-3).any() and got.min() == np.float32(lo) and got.max() == np.float32(hi)
    # a NULL shift is a zero shift; a float sigma is the tensor of that float
    b, _, _, _ = pol.explore(x, 0.25, low=lo, high=hi, seed=em.SEED, step=3)
    c, _, _, _ = pol.explore(x, torch.full((A,), 0.25, device=dev()), shift=torch.zeros(A, device=dev()), low=lo, high=hi, seed=em.SEED, step=3)
    assert np.array_equal(bits(b), bits(c)) and (E * A < 85 or not np.array_equal(bits(b), bits(a)))
    pol.close()


@pytest.mark.parametrize("E,A,lo,hi", [(1, 1, -1.0, 1.0), (17, 5, -1.0, 1.0), (37, 65, 0.0, 1.0), (16, 512, -0.5, 0.75)])
def test_uniform_actions_lie_in_the_range_and_follow_the_model(E, A, lo, hi):
    pol = make_policy("one", 3, A, critic=False)
    u = torch.empty((E, A), device=dev())
    a, env, lp, v = pol.sample_uniform(E, low=lo, high=hi, seed=em.SEED, step=2 ** 32 + 1, env_id_offset=4, noise=u)
    assert lp is None and v is None and np.array_equal(bits(a), bits(env))
    want_u = em.uniforms(em.SEED, np.arange(E) + 4, A, 2 ** 32 + 1)
    assert np.array_equal(u.cpu().numpy().astype(np.float64), want_u)  # the uniforms are exact in float32
    got = a.cpu().numpy()
    assert (got >= np.float32(lo)).all() and (got < np.float32(hi)).all()
    # two float32 roundings, the product's at magnitude <= hi - lo and the sum's at <= max(|lo|, |hi|): one ulp of the range's size
    assert np.abs(got - em.uniform(lo, hi, want_u)).max() <= np.spacing(np.float32(max(abs(lo), abs(hi), hi - lo)))
    pol.close()


# ---- 7. into the rollout buffer ---------------------------------------------------------------------------------------------------
def test_sample_writes_a_rollout_slot_in_place():
    from fleetrl_amd import DeviceRolloutBuffer

    E, K, D, A = 17, 3, 45, 5
    pol = make_policy("tanh", D, A, scale_last=3.0)
    log_std = on_device(np.full(A, -0.5, np.float32))
    in_place, copied = DeviceRolloutBuffer(E, K, D, A), DeviceRolloutBuffer(E, K, D, A)
    rng = np.random.default_rng(3)
    for t in range(K):
        x = observations(E, D, seed=t)
        reward = on_device(rng.standard_normal(E))
        start = on_device((rng.random(E) < 0.3).astype(np.uint8))
        s = in_place.slot(t)
        env_a = torch.empty((E, A), device=dev())
        pol.sample(x, log_std, seed=9, step=t, actions_out=s.actions, env_actions_out=env_a, log_prob_out=s.log_prob, values_out=s.value)
        in_place.add(x, s.actions, reward, start, s.value, s.log_prob)
        a, env_b, lp, v = pol.sample(x, log_std, seed=9, step=t, values_out=torch.empty((E, 1), device=dev()))
        copied.add(x, a, reward, start, v, lp)
        assert np.array_equal(bits(env_a), bits(env_b)) and float(env_a.abs().max()) <= 1.0
    torch.cuda.synchronize()
    for name in ("observations", "actions", "rewards", "values", "log_probs"):
        assert np.array_equal(bits(getattr(in_place, name)), bits(getattr(copied, name))), name
    assert torch.equal(in_place.episode_starts, copied.episode_starts)
    assert not torch.equal(in_place.actions[0], in_place.actions[1]) and bool((in_place.log_probs != 0).all())
    in_place.check_errors(), copied.check_errors()
    in_place.close(), copied.close(), pol.close()


def test_env_actions_are_accepted_by_step_torch():
    from bench import bench_config

    from fleetrl_amd import DevicePolicy, FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    E, N = 17, 5
    env = FleetVecNormalize(FleetVecEnv(dict(bench_config(E, N, "ct"), episode_length=48), E, tables=synth_tables("ct", N, seed=3), seed=1))
    D = env.norm.D
    pol = DevicePolicy(pm.random_layers(np.random.default_rng(8), (D, 64, 64, N)))
    obs, reward, done = torch.empty((E, D), device=dev()), torch.empty(E, device=dev(), dtype=torch.float64), torch.empty(E, device=dev(), dtype=torch.uint8)
    env.reset_torch(obs_out=obs)
    for t in range(3):
        _, env_a, lp, _ = pol.sample(obs, 0.5, seed=1, step=t)
        env.step_torch(env_a, obs_out=obs, reward_out=reward, done_out=done)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(reward).all()) and bool(torch.isfinite(lp).all())
    assert float(env_a.abs().max()) <= 1.0
    pol.close(), env.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_reason_and_launch_nothing():
    from fleetrl_amd import DeviceNormalizer, _capi

    E, D, A = 8, 45, 5
    two, one = make_policy("tanh", D, A), make_policy("tanh", D, A, critic=False)
    x = observations(E, D)
    scale = torch.zeros(A, device=dev())
    outs = {n: torch.full(s, 9.0, device=dev()) for n, s in (("noise", (E, A)), ("actions", (E, A)), ("env_actions", (E, A)),
                                                               ("log_prob", (E,)), ("values", (E, 1)), ("mean", (E, A)))}
    wrong_norm = DeviceNormalizer(E, 44)

    def args(**over):
        a = _capi.FleetExploreArgs()
        a.struct_bytes, a.mode, a.noise_mode = C.sizeof(_capi.FleetExploreArgs), _capi.EXPLORE_GAUSSIAN, _capi.EXPLORE_NOISE_DRAW
        a.seed, a.step, a.noise_lo, a.noise_hi = 1, 2, -1.0, 1.0
        a.scale = scale.data_ptr()
        for n in ("noise", "actions", "env_actions", "log_prob", "mean"):
            setattr(a, n, outs[n].data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    G, N, U = _capi.EXPLORE_GAUSSIAN, _capi.EXPLORE_ACTION_NOISE, _capi.EXPLORE_UNIFORM
    nan = float("nan")
    cases = [(two, x.data_ptr(), E, None, args(struct_bytes=8), "struct_bytes"), (two, x.data_ptr(), E, None, args(mode=3), "mode"),
             (two, x.data_ptr(), E, None, args(mode=-1), "mode"), (two, x.data_ptr(), E, None, args(noise_mode=2), "noise_mode"),
             (two, x.data_ptr(), 0, None, args(), "E must be >= 1"), (two, x.data_ptr(), -3, None, args(), "E must be >= 1"),
             (two, x.data_ptr(), E, None, args(actions=None), "null actions"), (two, None, E, None, args(), "null obs"),
             (two, None, E, None, args(mode=N, log_prob=None), "null obs"),
             (two, x.data_ptr(), E, None, args(scale=None), "null scale"), (two, x.data_ptr(), E, None, args(mode=N, log_prob=None, scale=None), "null scale"),
             (two, x.data_ptr(), E, None, args(mode=N), "log_prob"), (two, None, E, None, args(mode=U), "log_prob"),
             (one, x.data_ptr(), E, None, args(values=outs["values"].data_ptr()), "critic"),
             (two, None, E, None, args(mode=U, log_prob=None, values=outs["values"].data_ptr()), "UNIFORM"),
             (two, x.data_ptr(), E, None, args(noise_mode=_capi.EXPLORE_NOISE_GIVEN, noise=None), "null noise"),
             (two, x.data_ptr(), E, None, args(mode=N, log_prob=None, noise_lo=nan), "noise_lo <= noise_hi"),
             (two, x.data_ptr(), E, None, args(mode=N, log_prob=None, noise_hi=nan), "noise_lo <= noise_hi"),
             (two, None, E, None, args(mode=U, log_prob=None, noise_hi=nan), "noise_lo <= noise_hi"),
             (two, x.data_ptr(), E, None, args(mode=N, log_prob=None, noise_lo=0.5, noise_hi=0.25), "noise_lo <= noise_hi"),
             (two, None, E, None, args(mode=U, log_prob=None, noise_lo=0.5, noise_hi=0.25), "noise_lo <= noise_hi"),
             (two, x.data_ptr(), E, None, args(env_id_offset=-1), "env_id_offset"),
             (two, x.data_ptr(), E, None, args(mode=N, log_prob=None, env_id_offset=-2 ** 31), "env_id_offset"),
             (two, x.data_ptr(), E, wrong_norm.h, args(), "obs_dim 44")]
    assert G == 0
    for pol, obs_ptr, n, norm, a, word in cases:
        assert pol.lib.fleet_explore_act_dev(pol.h, obs_ptr, n, norm, C.byref(a)) == _capi.ERR_INVALID, word
        why = pol.lib.fleet_policy_last_error(pol.h).decode()
        assert why.startswith("fleet_explore_act_dev: ") and word in why, (word, why)
    assert two.lib.fleet_explore_act_dev(two.h, x.data_ptr(), E, None, None) == _capi.ERR_INVALID
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert bool((t == 9.0).all()), n  # nothing was launched
    # the Python methods refuse what the library refuses, and what it cannot see
    from fleetrl_amd import FleetHipError

    with pytest.raises(FleetHipError) as ei:
        one.sample(x, scale, seed=0, step=0, values_out=outs["values"])
    assert ei.value.status == _capi.ERR_INVALID and "critic" in str(ei.value)
    with pytest.raises(ValueError):
        two.sample(x, scale, seed=0, step=0, noise_given=True)
    with pytest.raises(ValueError):
        two.sample(x, torch.zeros(A + 1, device=dev()), seed=0, step=0)
    with pytest.raises(NotImplementedError):
        two.predict(x.cpu().numpy(), deterministic=False)
    # ... and the accepted call still works afterwards; GAUSSIAN does not read the bounds, so it takes any
    a = args(noise_lo=nan, noise_hi=-1.0)
    assert two.lib.fleet_explore_act_dev(two.h, x.data_ptr(), E, None, C.byref(a)) == _capi.OK
    torch.cuda.synchronize()
    assert bool((outs["actions"] != 9.0).all()) and bool((outs["values"] == 9.0).all())
    wrong_norm.close(), one.close(), two.close()


# ---- 9. statistics on the device -----------------------------------------------------------------------------------------------
def test_device_noise_has_the_moments_of_a_standard_normal():
    """The shape, the seed and the bounds of tests/test_explore_cpu.py's check of the model."""
    E, A = em.STAT_SHAPE
    pol = make_policy("one", 3, A, critic=False)
    x = observations(E, 3)
    eps = [torch.empty((E, A), device=dev()) for _ in range(2)]
    for step in range(2):  # (the second launch is for the correlation across steps)
        pol.sample(x, 0.0, seed=em.SEED, step=step, noise=eps[step])
    m = em.moments(eps[0].cpu().numpy().astype(np.float64), eps[1].cpu().numpy().astype(np.float64))
    _parity["moments"] = m
    print(m)
    write_parity()
    pol.close()
    assert em.check_moments(m) == []
