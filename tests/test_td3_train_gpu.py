"""TD3 / DDPG's whole update on the device (fleet_offpolicy.hip): the image-to-image Polyak update against fleet_qtarget_polyak_dev, the
one call against the existing pieces run step by step on a second set of handles -- bit for bit --, what a result may not depend on, the
refusals that need handles, and the example."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import offpolicy_model as om
import policy_bits as pb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
SEED = 0x7A46E7


def dev():
    return torch.device("cuda", 0)


def host(t):
    return t.detach().cpu().numpy().copy()


def same64(a, b) -> bool:
    """float64 arrays equal bit for bit, a NaN equal to a NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def all_same(xs, ys) -> bool:
    return len(xs) == len(ys) and all(pb.same_bits(x, y) for x, y in zip(xs, ys))


def pair(**kw):
    a, b = om.Stack(**kw), om.Stack(**kw)
    assert om.same_state(a.state(), b.state()) == []
    return a, b


# ---- 1. the Polyak update on its own --------------------------------------------------------------------------------------------------
POLYAK = {
    "8-8": dict(),
    "65-wide": dict(hidden=(65, 8)),  # two out64 tiles
    "rows-of-16-bytes": dict(D=8, A=4),
    "one-critic": dict(n_critics=1),
}


@pytest.mark.parametrize("tau", [0.0, 0.005, 1.0])
@pytest.mark.parametrize("case", sorted(POLYAK))
def test_three_image_to_image_updates_equal_three_tensor_walks_bit_for_bit(case, tau):
    a, b = pair(**POLYAK[case])
    rng = np.random.default_rng(len(case))
    probe = {k: torch.from_numpy(v).to(dev()) for k, v in (("next_obs", rng.standard_normal((5, a.D)).astype(F32)),
                                                            ("rewards", rng.standard_normal(5).astype(F32)),
                                                            ("dones", (rng.random(5) < 0.4).astype(F32)))}
    start = [host(t) for t in a.targets.export_torch()]
    for k in range(3):
        for s in (a, b):  # new online weights in torch's parameters AND in the online image, the same in both sets
            g = torch.Generator(device="cpu").manual_seed(100 + k)
            with torch.no_grad():
                for p in s.online_params:
                    p.add_((0.3 * torch.randn(p.shape, generator=g)).to(dev()))
            s.online.load_torch(s.online_params)
        a.train.polyak(tau)
        b.targets.polyak(b.online_params, tau)
        got, want = [host(t) for t in a.targets.export_torch()], [host(t) for t in b.targets.export_torch()]
        assert all_same(got, want), (case, tau, k)
        ya, yb = (s.targets.target(probe["next_obs"], probe["rewards"], probe["dones"], gamma=0.99, sigma=s.sigma, noise_clip=0.5, seed=3, step=k)
                  for s in (a, b))
        assert pb.same_bits(host(ya), host(yb)) and np.isfinite(host(ya)).all()
        if tau == 0.0:
            assert all_same(got, start)
        elif tau == 1.0:
            assert all(np.array_equal(x, host(p)) for x, p in zip(got, a.online_params))  # (== : a -0 of the online comes out +0)
        else:
            assert not all_same(got, start)
    assert all_same([host(t) for t in a.online.export_torch()], [host(p) for p in a.online_params])  # the online image is only read
    a.close()
    b.close()


def test_polyak_refuses_a_tau_outside_the_unit_interval():
    from fleetrl_amd import FleetHipError

    s = om.Stack()
    before = [host(t) for t in s.targets.export_torch()]
    for tau in (1.5, float("nan"), -0.1):
        with pytest.raises(FleetHipError, match=r"fleet_offpolicy_polyak_dev: tau must be in \[0, 1\], got"):
            s.train.polyak(tau)
    assert all_same([host(t) for t in s.targets.export_torch()], before)
    s.close()


# ---- 2. the one call against the pieces ------------------------------------------------------------------------------------------------
BASE = dict(G=5, B=4, delay=2, first_update=0, seed=SEED)
EQUIVALENCE = {
    "delay-2-even": (dict(), BASE),
    "delay-2-odd": (dict(), dict(BASE, first_update=1)),
    "no-actor-step": (dict(), dict(BASE, G=2, delay=3)),
    "delay-1": (dict(), dict(BASE, delay=1)),
    "ddpg": (dict(n_critics=1), dict(BASE, delay=1)),
    "batch-1": (dict(), dict(BASE, B=1)),
    "batch-tile-plus-1": (dict(max_batch=32), dict(BASE, B=17)),
    "ring-partly-filled": (dict(pos=4, full=False), BASE),
    "ring-wrapped": (dict(pos=4, full=True), BASE),
    "tanh": (dict(activation="tanh"), BASE),
    "65-wide": (dict(hidden=(65, 8)), BASE),
    "rows-of-16-bytes": (dict(D=8, A=4), BASE),
    "normalised": (dict(with_norm=True), BASE),
    "one-step": (dict(), dict(BASE, G=1, delay=1)),
    "max-steps": (dict(max_steps=8), dict(BASE, G=8)),
}


@pytest.mark.parametrize("case", sorted(EQUIVALENCE))
def test_the_one_call_equals_the_existing_pieces_step_by_step_bit_for_bit(case):
    make, kw = EQUIVALENCE[case]
    a, b = pair(**make)
    if case == "batch-tile-plus-1":
        assert kw["B"] == a.grad.tile_rows + 1
    if case == "max-steps":
        assert kw["G"] == a.train.describe()["max_steps"]
    start = a.state()
    stats = host(a.one_call(**kw))
    slots = b.step_by_step(**kw)
    got, want = a.state(), b.state()
    model = om.finish(slots, kw["first_update"], kw["delay"])
    hits = om.actor_steps(kw["first_update"], kw["G"], kw["delay"])
    print(case, "actor steps", hits, "statistics", dict(zip(om.STATS, stats[:8])), "model", model[:8].tolist())
    assert om.same_state(got, want) == [], om.same_state(got, want)
    assert got["calls"] == start["calls"] + kw["G"] and got["critic_step"] == kw["G"] and got["actor_step"] == len(hits)
    assert all_same(got["params"], got["online_image"]) and all_same(got["params"], got["online_export"])  # the image moved with them
    n_actor = len(a.actor_params)
    assert not all_same(got["params"][n_actor:], start["params"][n_actor:])  # the critics did move
    # [4..7] against the step-by-step run's own last statistics, [0..3] against the model's ordered sums over its per-step statistics
    last_actor = np.float64(slots[hits[-1], om.ACTOR_AT]) if hits else np.nan
    assert same64(stats[4:8], [np.float64(slots[-1, 0]), last_actor, kw["first_update"] + kw["G"], len(hits)])
    assert same64(stats[:4], model[:4]) and same64(stats, model) and not stats[8:].any()
    assert np.isfinite(stats[:3]).all() and (stats[2] == 0.0) == (a.n_critics == 1)
    if hits:
        assert np.isfinite(stats[3]) and not all_same(got["target_image"], start["target_image"])
        assert not all_same(got["params"][:n_actor], start["params"][:n_actor])
    else:  # no actor step: NaN, the actor and the targets untouched bit for bit
        assert np.isnan(stats[3]) and np.isnan(stats[5])
        assert all_same(got["params"][:n_actor], start["params"][:n_actor]) and all_same(got["target_image"], start["target_image"])
        assert got["actor_m"] == [] or all(not m.any() for m in got["actor_m"])
    if case == "normalised":  # and the normaliser's statistics did enter: the raw minibatches give other weights
        raw = om.Stack()
        raw.one_call(**kw)
        assert not all_same(raw.state()["params"], got["params"])
        raw.close()
    a.buf.check_errors()
    a.close()
    b.close()


# ---- 3. reproducibility and independence ---------------------------------------------------------------------------------------------
def run(kw=None, make=None, prepare=None, stream=None):
    s = om.Stack(**(make or {}))
    if prepare:
        prepare(s)
    kw = dict(BASE, G=4, **(kw or {}))
    if stream is None:
        stats = host(s.one_call(**kw))
    else:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):  # the borrowed handles move with torch's current stream
            stats = s.one_call(**kw)
        torch.cuda.synchronize()
        stats = host(stats)
    out = (s.state(), stats)
    s.close()
    return out


def fill_block_with_nan(s):
    from fleetrl_amd._handle import _DeviceArray

    d = s.train.describe()
    assert d["slots"] == d["staging"] + d["staging_bytes"] and d["staging_bytes"] % 256 == 0
    floats = d["staging_bytes"] // 4 + d["max_steps"] * om.SLOT
    torch.as_tensor(_DeviceArray(d["staging"], (floats,), "<f4", s.train), device=dev()).fill_(float("nan"))
    torch.cuda.synchronize()


def test_a_result_depends_on_the_state_the_seed_and_the_update_count_and_on_nothing_else():
    ref, ref_stats = run()
    assert np.isfinite(ref_stats).all() and all(np.isfinite(p).all() for p in ref["params"])

    again, stats = run()  # two calls from identical states
    assert om.same_state(again, ref) == [] and same64(stats, ref_stats)

    s = om.Stack()  # one call of G = 4 equals two of G = 2, the second with first_update + 2
    s.one_call(**dict(BASE, G=2))
    second = host(s.one_call(**dict(BASE, G=2, first_update=2)))
    assert om.same_state(s.state(), ref) == [] and second[6] == 4.0 and same64(second[4:6], ref_stats[4:6])
    s.close()

    other, stats = run(stream=torch.cuda.Stream(device=dev()))
    assert om.same_state(other, ref) == [] and same64(stats, ref_stats)

    big, stats = run(make=dict(max_batch=4 * 16, max_steps=4 * 8))  # other staging strides, another scratch, more slots
    assert om.same_state(big, ref) == [] and same64(stats, ref_stats)

    nan, stats = run(prepare=fill_block_with_nan)  # NaN in every staging row and slot before the call
    assert om.same_state(nan, ref) == [] and same64(stats, ref_stats)

    for change in (dict(seed=SEED + 1), dict(first_update=2)):  # another noise key / another phase of the delay: other weights
        moved, _ = run(kw=change)
        assert not all_same(moved["params"], ref["params"]) and moved["critic_step"] == ref["critic_step"]


# ---- 4. the refusals that need handles -------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handles_launch_nothing():
    from fleetrl_amd import DeviceNormalizer, DeviceReplayBuffer, DeviceTD3Target, DeviceTD3Train, FleetHipError, _capi

    s = om.Stack(max_batch=4, max_steps=3)
    before = s.state()
    kw = dict(BASE, G=3)
    with pytest.raises(FleetHipError, match="fleet_offpolicy_td3_dev: gradient_steps must be at most max_steps = 3, got 4"):
        s.one_call(**dict(kw, G=4))
    with pytest.raises(FleetHipError, match="fleet_offpolicy_td3_dev: batch_size: B must be at most max_batch = 4, got 5"):
        s.one_call(**dict(kw, B=5))
    s.buf.set_position(0, False, before["calls"])
    with pytest.raises(FleetHipError, match="fleet_offpolicy_td3_dev: the buffer is empty") as e:
        s.one_call(**kw)
    assert e.value.status == _capi.ERR_STATE
    s.buf.set_position(0, True, before["calls"])
    wrong = DeviceNormalizer(s.E, s.D + 1)
    s.env = wrong
    with pytest.raises(FleetHipError, match=f"fleet_offpolicy_td3_dev: the normaliser has obs_dim {s.D + 1} on device 0, the buffer {s.D} on device 0"):
        s.one_call(**kw)
    s.env = None
    other = torch.cuda.Stream(device=dev())
    s.train.use_torch_stream()
    s.buf.set_stream(other.cuda_stream)
    with pytest.raises(FleetHipError, match="fleet_offpolicy_td3_dev: the replay buffer, the target networks and the online networks do not launch"):
        _raw_call(s, 3, 4)
    s.buf.set_stream(torch.cuda.current_stream().cuda_stream)
    s.targets.set_stream(other.cuda_stream)
    with pytest.raises(FleetHipError, match="do not launch on one stream"):
        _raw_call(s, 3, 4)
    with pytest.raises(FleetHipError, match="fleet_offpolicy_polyak_dev: the target networks launch on another stream"):
        s.train._check(s.train.lib.fleet_offpolicy_polyak_dev(s.train.h, 0.5))
    s.targets.set_stream(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(FleetHipError, match=r"fleet_offpolicy_td3_dev: expected 6 tensors \(W, b per layer of the actor\), got 4"):
        _raw_call(s, 3, 4, n_actor=4)
    with pytest.raises(FleetHipError, match=r"fleet_offpolicy_td3_dev: expected 12 tensors \(W, b per layer, critic after critic\), got 6"):
        _raw_call(s, 3, 4, n_critic=6)
    torch.cuda.synchronize()
    assert om.same_state(s.state(), before) == []  # nothing was launched: the counter, the step counts and every bit stayed
    stats = host(_raw_call(s, 3, 4))  # and the same arguments pass
    after = s.state()
    assert after["calls"] == before["calls"] + 3 and after["critic_step"] == 3 and after["actor_step"] == 1 and np.isfinite(stats).all()

    # create
    twin = om.Stack(max_batch=4, max_steps=3)
    new = lambda *a, **k: DeviceTD3Train(*a, **k)  # noqa: E731
    with pytest.raises(FleetHipError, match="fleet_offpolicy_create: the online and the target networks are one handle"):
        new(s.buf, s.online, s.grad, s.opt_a, s.opt_c)
    actor, critics = om.networks(s.D, s.A, (8, 8), 2, 1)
    for why, kwargs in (("activation", dict(activation="tanh")), ("output", dict(output="clip")), ("bounds", dict(output="tanh", high=2.0))):
        odd = DeviceTD3Target(actor, critics, **dict(dict(activation="relu", output="tanh"), **kwargs))
        with pytest.raises(FleetHipError, match="fleet_offpolicy_create: the online and the target networks differ in their records"):
            new(s.buf, odd, s.grad, s.opt_a, s.opt_c)
        odd.close()
    wide_actor, wide_critics = om.networks(s.D, s.A, (9, 8), 2, 1)
    odd = DeviceTD3Target(wide_actor, wide_critics, activation="relu", output="tanh")
    with pytest.raises(FleetHipError, match="differ in their records"):
        new(s.buf, odd, s.grad, s.opt_a, s.opt_c)
    odd.close()
    with pytest.raises(FleetHipError, match="fleet_offpolicy_create: the actor optimiser lies on another image than the gradient handle"):
        new(s.buf, s.targets, s.grad, twin.opt_a, s.opt_c)
    with pytest.raises(FleetHipError, match="fleet_offpolicy_create: the critic optimiser lies on another image than the gradient handle"):
        new(s.buf, s.targets, s.grad, s.opt_a, twin.opt_c)
    with pytest.raises(FleetHipError, match=r"fleet_offpolicy_create: the actor optimiser's span must be \(first_net 0, n_nets 1, no extras\)"):
        new(s.buf, s.targets, s.grad, s.opt_c, s.opt_c)
    with pytest.raises(FleetHipError, match=r"fleet_offpolicy_create: the critic optimiser's span must be \(first_net 1, n_nets 2, no extras\)"):
        new(s.buf, s.targets, s.grad, s.opt_a, s.opt_a)
    wide = DeviceReplayBuffer(21, 3, s.D + 1, s.A)
    with pytest.raises(FleetHipError, match=f"fleet_offpolicy_create: the replay buffer's obs_dim is {s.D + 1}, the networks' {s.D}"):
        new(wide, s.targets, s.grad, s.opt_a, s.opt_c)
    short = DeviceReplayBuffer(21, 3, s.D, s.A - 1)
    with pytest.raises(FleetHipError, match=f"fleet_offpolicy_create: the replay buffer's act_dim is {s.A - 1}, the networks' {s.A}"):
        new(short, s.targets, s.grad, s.opt_a, s.opt_c)
    for bad in (0, 65537):
        with pytest.raises(FleetHipError, match=f"fleet_offpolicy_create: max_steps must be in 1..65536, got {bad}"):
            new(s.buf, s.targets, s.grad, s.opt_a, s.opt_c, max_steps=bad)
    assert om.same_state(s.state(), after) == []
    for h in (wide, short, wrong):
        h.close()
    twin.close()
    s.close()


def _raw_call(s, G, B, n_actor=None, n_critic=None):
    """fleet_offpolicy_td3_dev through train_dev, WITHOUT moving any handle to torch's stream first."""
    from fleetrl_amd import _capi

    for p in s.online_params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    a = _capi.FleetOffpolicyArgs()
    a.gradient_steps, a.batch_size, a.policy_delay = G, B, 2
    a.gamma, a.tau, a.noise_clip, a.act_lo, a.act_hi, a.lr = 0.99, 0.005, 0.5, -1.0, 1.0, 1e-3
    for o in range(2):
        a.beta1[o], a.beta2[o], a.eps[o], a.max_grad_norm[o] = 0.9, 0.999, 1e-8, 0.0
    a.seed, a.first_update, a.sigma = SEED, 0, s.sigma.data_ptr()
    stats = torch.zeros(16, device=dev(), dtype=torch.float64)
    a.stats = stats.data_ptr()
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    ga, gc = [p.grad for p in s.actor_params], [p.grad for p in s.critic_params]
    s.train.train_dev(a, arr(s.actor_params), arr(ga), len(ga) if n_actor is None else n_actor, arr(s.critic_params), arr(gc),
                      len(gc) if n_critic is None else n_critic)
    return stats


# ---- 5. the example ----------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_and_prints_finite_losses():
    """examples/td3_device_train.py as a child process under a time limit of its own: exit 0, finite losses, the update count moves."""
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(om.ROOT, "examples", "td3_device_train.py"), "--steps", "40", "--envs", "8",
           "--evs", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{") and "train/critic_loss" in x]
    assert len(lines) >= 1
    for d in lines:
        for k in ("train/critic_loss", "train/actor_loss", "train/n_updates", "mean_raw_reward"):
            assert np.isfinite(d[k]), (k, d)
    assert lines[-1]["train/n_updates"] > 0
