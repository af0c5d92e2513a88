"""The policy forward on the device (fleet_policy.hip) against the float64 model of tests/policy_model.py, its exact invariants, the
fused normalisation against the normaliser's own output, evaluate_policy against a host loop, and the refusals.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest

import policy_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(pm.ROOT, "profiles", "policy_parity.json")
_parity = {}


def dev():
    return torch.device("cuda", 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def make_policy(name):
    from fleetrl_amd import DevicePolicy

    actor, critic, activation, output = pm.network(name)
    return DevicePolicy(actor, critic_layers=critic, activation=activation, output=output)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


# ---- (a) parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pm.NETWORKS))
def test_forward_stays_within_eight_times_the_float32_reference_error(name):
    """Per case (network, E, head): eps_ref = max |torch-CPU float32 - float64 model|, the distance of the arithmetic SB3 itself runs;
    the device must stay within 8 * max(eps_ref, 2^-24 * max |output|) of the float64 model.  The factor covers another summation
    order and nothing else.  The figures of the run go to profiles/policy_parity.json."""
    pol = make_policy(name)
    T = pol.describe()["tile_rows"]
    assert T == pol.tile_rows >= 1
    failures = []
    for E in pm.batch_sizes(T):
        x = on_device(pm.inputs(name, E))
        values = torch.empty((E, pol.value_dim), device=dev()) if pol.value_dim else None
        got = [pol.act(x, values_out=values)] + ([values] if pol.value_dim else [])
        torch.cuda.synchronize()
        for head, (y, (y64, eps_ref)) in enumerate(zip(got, pm.reference(name, E))):
            y = y.cpu().numpy().astype(np.float64)
            assert y.shape == y64.shape
            err = float(np.max(np.abs(y - y64)))
            bound = 8 * max(eps_ref, 2.0 ** -24 * float(np.max(np.abs(y64))))
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
            _parity[f"{name}/E{E}/head{head}"] = {"eps_ref": eps_ref, "device_err": err, "bound": bound, "err_over_bound": ratio}
            print(f"{name} E={E} head {head}: eps_ref {eps_ref:.3g} device {err:.3g} bound {bound:.3g} ratio {ratio:.3g}")
            if not err <= bound:
                failures.append((E, head, err, bound))
    pol.close()
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as fh:
        json.dump({"tile_rows": T, "bound": "8 * max(eps_ref, 2^-24 * max|output|)", "cases": dict(sorted(_parity.items()))}, fh, indent=1)
        fh.write("\n")
    assert not failures, failures


# ---- (b) exact invariants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture", "388-400-300-50", "45-63-65-1", "389-512-512-3"])
def test_a_row_does_not_depend_on_the_batch_or_its_position(name):
    pol = make_policy(name)
    T = pol.tile_rows
    E = 16 * T + 1
    x = on_device(pm.inputs(name, E))
    full = pol.act(x)
    for r in (0, 5, 6, T - 1, T, 3 * T + 2, E - 1):
        alone = pol.act(x[r:r + 1].contiguous())
        assert np.array_equal(bits(alone)[0], bits(full)[r]), r
    perm = torch.from_numpy(np.random.default_rng(0).permutation(E)).to(dev())
    moved = pol.act(x[perm].contiguous())
    assert np.array_equal(bits(moved), bits(full[perm]))
    tail = pol.act(x[T + 3:].contiguous())  # other rows per tile, another last tile
    assert np.array_equal(bits(tail), bits(full[T + 3:]))
    pol.close()


def test_two_forwards_are_bit_identical_also_on_another_stream():
    pol = make_policy("388-64-64-50")
    x = on_device(pm.inputs("388-64-64-50", 16 * pol.tile_rows + 1))
    a, b = pol.act(x), pol.act(x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = pol.act(x)
    side.synchronize()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    d = pol.act(x)  # ... and back on the first stream
    assert np.array_equal(bits(a), bits(d))
    pol.close()


def test_clip_saturates_at_exactly_the_bounds():
    from fleetrl_amd import DevicePolicy

    rng = np.random.default_rng(4)
    layers = pm.random_layers(rng, (20, 70, 9))
    layers[-1] = (layers[-1][0] * 40, layers[-1][1])
    lo, hi = -0.3, 0.7
    pol = DevicePolicy(layers, activation="tanh", output="clip", low=lo, high=hi)
    x = on_device(pm.inputs("four-layers-20-33-130-70-4", 65))
    y = pol.act(x).cpu().numpy()
    y64 = pm.forward64(layers, x.cpu().numpy(), "tanh", "none")
    assert (y64 > hi + 0.01).any() and (y64 < lo - 0.01).any() and ((y64 > lo + 0.01) & (y64 < hi - 0.01)).any()
    assert (y[y64 > hi + 0.01] == np.float32(hi)).all() and (y[y64 < lo - 0.01] == np.float32(lo)).all()
    assert y.min() == np.float32(lo) and y.max() == np.float32(hi)
    pol.close()


def test_actor_outputs_do_not_depend_on_the_critic():
    from fleetrl_amd import DevicePolicy

    actor, critic, activation, output = pm.network("fixture")
    both, alone = DevicePolicy(actor, critic_layers=critic), DevicePolicy(actor)
    x = on_device(pm.inputs("fixture", 65))
    values = torch.empty((65, 1), device=dev())
    with_values, without_values, actor_only = both.act(x, values_out=values), both.act(x), alone.act(x)
    assert np.array_equal(bits(with_values), bits(without_values)) and np.array_equal(bits(with_values), bits(actor_only))
    assert np.abs(values.cpu().numpy() - pm.reference("fixture", 65)[1][0]).max() < 1e-3  # (the critic did run)
    both.close(), alone.close()


def test_load_dev_gives_the_bits_of_load_host():
    from fleetrl_amd import DevicePolicy

    actor, critic, _, _ = pm.network("fixture")
    rng = np.random.default_rng(6)
    new_actor = [((w + rng.normal(0, 0.05, w.shape)).astype(np.float32), (b + 0.1).astype(np.float32)) for w, b in actor]
    new_critic = [((w * 0.5).astype(np.float32), (b - 0.2).astype(np.float32)) for w, b in critic]
    host, devp, fresh = DevicePolicy(actor, critic_layers=critic), DevicePolicy(actor, critic_layers=critic), DevicePolicy(new_actor, critic_layers=new_critic)
    x = on_device(pm.inputs("fixture", 65))
    before = torch.empty((65, 1), device=dev())
    host.act(x, values_out=before)
    host.load_host(new_actor, new_critic)
    devp.load_torch([on_device(a) for pair in new_actor + new_critic for a in pair])
    outs = []
    for p in (host, devp, fresh):
        v = torch.empty((65, 1), device=dev())
        outs.append((bits(p.act(x, values_out=v)), bits(v)))
    assert not np.array_equal(outs[0][1], bits(before))
    for a, v in outs[1:]:
        assert np.array_equal(a, outs[0][0]) and np.array_equal(v, outs[0][1])
    with pytest.raises(ValueError):
        devp.load_torch([on_device(a) for pair in new_actor for a in pair])
    for p in (host, devp, fresh):
        p.close()


# ---- (c) fused normalisation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,norm_obs", [("fixture", True), ("388-64-64-50", True), ("389-512-512-3", True), ("fixture", False)])
def test_fused_normalisation_equals_the_normalisers_own_output(name, norm_obs):
    from fleetrl_amd import DeviceNormalizer

    pol = make_policy(name)
    E, D = 4 * pol.tile_rows + 1, pol.obs_dim
    norm = DeviceNormalizer(E, D, clip_obs=4.0)
    gen = torch.Generator(device=dev())
    gen.manual_seed(D)
    rew, done = torch.zeros(E, device=dev(), dtype=torch.float64), torch.zeros(E, device=dev(), dtype=torch.uint8)
    for _ in range(4):  # statistics of a few steps; column 0 constant (var 0), column 1 far from zero
        raw = torch.randn((E, D), device=dev(), generator=gen) * 3 + 1
        raw[:, 0] = 7.0
        if D > 1:
            raw[:, 1] += 1e4
        norm.step_torch(raw, rew, done)
    norm.configure(training=False, norm_obs=norm_obs)
    raw = torch.randn((E, D), device=dev(), generator=gen) * 5 + 1
    if D > 1:
        raw[:, 1] += 1e4
    applied, _, _ = norm.step_torch(raw, rew, done)
    assert norm_obs == (not torch.equal(applied, raw))
    want = pol.act(applied)
    got = pol.act(raw, normalizer=norm)
    assert np.array_equal(bits(got), bits(want))
    fewer = pol.act(raw[:3].contiguous(), normalizer=norm)  # the normaliser's own E does not matter
    assert np.array_equal(bits(fewer), bits(want[:3]))
    norm.close()
    pol.close()


def test_a_forward_on_another_stream_waits_for_the_normalisers_update():
    from fleetrl_amd import DeviceNormalizer

    pol = make_policy("388-64-64-50")
    E, D = 16 * pol.tile_rows + 1, pol.obs_dim
    norm = DeviceNormalizer(E, D)
    gen = torch.Generator(device=dev())
    gen.manual_seed(3)
    rew, done = torch.zeros(E, device=dev(), dtype=torch.float64), torch.zeros(E, device=dev(), dtype=torch.uint8)
    raws = [torch.randn((E, D), device=dev(), generator=gen) * (k + 1) + k for k in range(6)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = []
    for raw in raws:  # update k on torch's stream, then a forward on the side stream that must see statistics k
        norm.step_torch(raw, rew, done)
        with torch.cuda.stream(side):
            got.append(pol.act(raws[0], normalizer=norm))
    torch.cuda.synchronize()
    # the same sequence on one stream
    norm2 = DeviceNormalizer(E, D)
    for k, raw in enumerate(raws):
        norm2.step_torch(raw, rew, done)
        want = pol.act(raws[0], normalizer=norm2)
        assert np.array_equal(bits(got[k]), bits(want)), k
    assert not np.array_equal(bits(got[0]), bits(got[5]))
    norm.close(), norm2.close(), pol.close()


def test_a_normaliser_of_another_width_is_refused():
    from fleetrl_amd import DeviceNormalizer, FleetHipError, _capi

    pol = make_policy("fixture")
    norm = DeviceNormalizer(8, 44)
    x = on_device(pm.inputs("fixture", 8))
    with pytest.raises(FleetHipError) as ei:
        pol.act(x, normalizer=norm)
    assert ei.value.status == _capi.ERR_INVALID and "obs_dim 44" in str(ei.value)
    with pytest.raises(TypeError):
        pol.act(x, normalizer=object())
    norm.close(), pol.close()


# ---- (d) integration ---------------------------------------------------------------------------------------------------------------
def _small_env(seed, N):
    from bench import bench_config

    from fleetrl_amd import FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    E = 8
    cfg = dict(bench_config(E, N, "ct"), episode_length=48, log_data=True)  # a 2-day episode
    venv = FleetVecNormalize(FleetVecEnv(cfg, E, tables=synth_tables("ct", N, seed=3), seed=seed))
    rng = np.random.default_rng(seed)
    venv.reset()
    for _ in range(12):  # statistics that are not the initial ones, the same in every env built here
        venv.step(rng.uniform(-1, 1, (E, N)).astype(np.float32))
    venv.training = False
    venv.venv.core.clear_log()
    return venv


@pytest.mark.parametrize("N", [5, 1])
def test_evaluate_policy_equals_a_host_loop_on_a_small_env(N):
    """8 envs x N EVs, 2-day episodes, FleetVecNormalize(training=False).  The shipped agent (45 inputs, 1 action) runs when the
    env has that shape.  With 5 EVs the observation is wider and there are 5 actions: a random tanh network of the env's own
    width runs instead.  With 1 EV the shape is the agent's and the fixture runs (both asserted below)."""
    from fleetrl_amd import DevicePolicy, evaluate_policy

    host_env, dev_env = _small_env(11, N), _small_env(11, N)
    D, A = host_env.observation_space.shape[0], host_env.action_space.shape[0]
    uses_fixture = (D, A) == (45, 1)
    assert uses_fixture == (N == 1) and A == N
    layers = pm.fixture_layers()[0] if uses_fixture else pm.random_layers(np.random.default_rng(8), (D, 64, 64, A))
    if not uses_fixture:
        layers[-1] = (layers[-1][0] * 3, layers[-1][1])  # some actions reach the clip
    pol = DevicePolicy(layers)
    n_eval = 13  # ragged: envs 3..7 owe two episodes, envs 0..2 one
    want_r, want_l = pm.sb3_evaluate_policy(pol, host_env, n_eval_episodes=n_eval, return_episode_rewards=True)
    got_r, got_l = evaluate_policy(pol, dev_env, n_eval_episodes=n_eval, return_episode_rewards=True)
    assert len(got_r) == n_eval and got_l == [int(v) for v in want_l]
    assert np.array_equal(np.array(got_r).view(np.uint64), np.array(want_r, dtype=np.float64).view(np.uint64))
    assert len(set(got_r)) > 1
    host_rows = [len(x) for x in host_env.env_method("get_log")]
    dev_rows = [len(x) for x in dev_env.env_method("get_log")]
    assert dev_rows == host_rows and min(dev_rows) > 0
    mean, std = evaluate_policy(pol, dev_env, n_eval_episodes=8)
    assert np.isfinite(mean) and std >= 0
    with pytest.raises(NotImplementedError):
        evaluate_policy(pol, dev_env, deterministic=False)
    pol.close(), host_env.close(), dev_env.close()


def test_predict_is_sb3s_signature_for_host_callers():
    pol = make_policy("fixture")
    x = pm.inputs("fixture", 17)
    a, state = pol.predict(x, deterministic=True)
    assert state is None and a.shape == (17, 1) and a.dtype == np.float32
    assert np.array_equal(a, pol.act(on_device(x)).cpu().numpy())
    one, _ = pol.predict(x[3])
    assert one.shape == (1,) and one[0] == a[3, 0]
    with pytest.raises(NotImplementedError):
        pol.predict(x, deterministic=False)
    d = pol.describe()
    assert d["obs_dim"] == 45 and d["n_heads"] == 2 and d["heads"][0] == {"widths": [64, 64, 1], "activation": "tanh", "output": "clip", "low": -1.0, "high": 1.0}
    assert d["heads"][1]["widths"] == [64, 64, 1] and d["heads"][1]["output"] == "none"
    pol.close()
    pol.close()


# ---- (e) negative paths ----------------------------------------------------------------------------------------------------------
def test_refusals_come_with_their_status_and_message_and_leave_the_device_alone():
    from fleetrl_amd import DevicePolicy, FleetHipError, _capi

    rng = np.random.default_rng(9)
    x = on_device(pm.inputs("fixture", 8))
    for build, word in ((lambda: DevicePolicy(pm.random_layers(rng, (5, 513, 2))), "width"),
                        (lambda: DevicePolicy(pm.random_layers(rng, (5, 4, 4, 4, 4, 2))), "n_layers"),
                        (lambda: DevicePolicy([(np.full((2, 5), np.nan, np.float32), np.zeros(2, np.float32))]), "not finite")):
        with pytest.raises(FleetHipError) as ei:
            build()
        assert ei.value.status == _capi.ERR_INVALID and word in str(ei.value)
    one_head = DevicePolicy(pm.network("fixture")[0])
    out, values = torch.full((8, 1), 9.0, device=dev()), torch.full((8, 1), 9.0, device=dev())
    with pytest.raises(FleetHipError) as ei:
        one_head.act(x, out=out, values_out=values)
    assert ei.value.status == _capi.ERR_INVALID and "critic" in str(ei.value)
    for E in (0, -3):
        assert one_head.lib.fleet_policy_forward_dev(one_head.h, x.data_ptr(), E, None, out.data_ptr(), None) == _capi.ERR_INVALID
        assert "E must be >= 1" in one_head.lib.fleet_policy_last_error(one_head.h).decode()
    assert one_head.lib.fleet_policy_forward_dev(one_head.h, None, 8, None, out.data_ptr(), None) == _capi.ERR_INVALID
    actor = pm.network("fixture")[0]
    bad = [(w.copy(), b.copy()) for w, b in actor]
    bad[1][1][7] = np.inf
    with pytest.raises(FleetHipError) as ei:
        one_head.load_host(bad)
    assert ei.value.status == _capi.ERR_INVALID and "head 0, layer 1: bias 7 is not finite" in str(ei.value)
    torch.cuda.synchronize()
    assert (out == 9.0).all() and (values == 9.0).all()  # nothing was launched
    assert np.array_equal(bits(one_head.act(x)), bits(DevicePolicy(actor).act(x)))  # ... and the refused load changed nothing
    one_head.close()
