"""SAC's whole update on the device (fleet_sactrain_*, fleet_sactrain.hip): the alpha, scale and Polyak launches in bits, the one call
against the existing pieces run step by step on a second set of handles -- bit for bit --, what a result may not depend on, the
refusals that need handles, the float64 parity of the whole call against SB3's loop under autograd, and the example."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import policy_bits as pb
import sac_grad_model as gm
import sac_train_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
PARITY_FILE = os.path.join(sm.ROOT, "profiles", "sac_train_parity.json")
_parity = {}


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
    a, b = sm.Stack(**kw), sm.Stack(**kw)
    assert sm.same_state(a.state(), b.state()) == []
    return a, b


# ---- 1. the three launches on their own ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", [-20.0, -1.6094379, 0.0, 0.5, 2.0])
def test_alpha_equals_the_numpy_restatement_in_bits_and_torchs_exp_within_one_ulp(x):
    s = sm.Stack()
    t = torch.full((1,), x, device=dev())
    got = host(s.train.alpha(t))
    ref = host(torch.exp(t))
    assert got.dtype == F32 and got.view(np.int32)[0] == sm.alpha32(x).view(np.int32)
    assert abs(int(got.view(np.int32)[0]) - int(ref.view(np.int32)[0])) <= 1
    cell = torch.full((1,), 9.0, device=dev())  # into a tensor of the caller's
    assert s.train.alpha(t, out=cell) is cell and host(cell).tobytes() == got.tobytes()
    s.close()


@pytest.mark.parametrize("scale", [0.5, 0.3])
def test_scale_equals_foreach_mul_in_bits_and_touches_nothing_behind_a_tensor(scale):
    """131-(130, 70) critics with A = 65: W0 has 196 * 130 = 25 480 elements (24 chunks and 904 more), the last bias one; every gradient
    tensor is a slice of one buffer with a NaN behind it."""
    s = sm.Stack(max_batch=32, **sm.WIDE)
    shapes = s.train._shapes["critic"]
    assert shapes[0] == (130, 196) and int(np.prod(shapes[0])) == 25480 and 25480 % sm.SCALE_CHUNK != 0 and shapes[-1] == (1,)
    rng = np.random.default_rng(int(scale * 10))
    sizes = [int(np.prod(sh)) for sh in shapes]
    flat = torch.full((sum(sizes) + len(sizes),), float("nan"), device=dev())
    want, at = [], 0
    for p, n, sh in zip(s.critic_params, sizes, shapes):
        p.grad = flat[at:at + n].view(sh)
        p.grad.copy_(torch.from_numpy(rng.standard_normal(sh).astype(F32)).to(dev()))
        want.append(p.grad.clone())
        at += n + 1
    torch._foreach_mul_(want, scale)
    s.train.scale(s.critic_params, scale)
    torch.cuda.synchronize()
    assert all_same([host(p.grad) for p in s.critic_params], [host(w) for w in want])
    guards = np.cumsum([n + 1 for n in sizes]) - 1
    assert np.isnan(host(flat)[guards]).all() and int(np.isnan(host(flat)).sum()) == len(sizes)
    d = s.train.describe()
    assert d["scale_chunks"] == sum((n + sm.SCALE_CHUNK - 1) // sm.SCALE_CHUNK for n in sizes)
    s.close()


@pytest.mark.parametrize("tau", [0.0, 0.005, 1.0])
def test_three_image_to_image_updates_equal_three_tensor_walks_bit_for_bit(tau):
    a, b = pair()
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
        assert all_same(got, want), (tau, k)
        if tau == 0.0:
            assert all_same(got, start)
        elif tau == 1.0:
            assert all(np.array_equal(x, host(p)) for x, p in zip(got, a.online_params))  # (== : a -0 of the online comes out +0)
        else:
            assert not all_same(got, start)
    assert all_same([host(t) for t in a.online.export_torch()], [host(p) for p in a.online_params])  # the online image is only read
    a.close()
    b.close()


# ---- 2. the one call against the pieces ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(sm.EQUIVALENCE))
def test_the_one_call_equals_the_existing_pieces_step_by_step_bit_for_bit(case):
    make, kw = sm.EQUIVALENCE[case]
    a, b = pair(**make)
    if case == "batch-tile-plus-1":
        assert kw["B"] == a.grad.tile_rows + 1
    if case == "max-steps":
        assert kw["G"] == a.train.describe()["max_steps"]
    start = a.state()
    stats = host(a.one_call(**kw))
    slots = b.step_by_step(**kw)
    got, want = a.state(), b.state()
    G, interval, scale = kw["G"], kw["interval"], kw.get("loss_scale", 0.5)
    model = sm.finish(slots, kw["first_update"], interval, scale, a.learned)
    print(case, "target steps", sm.target_steps(G, interval), "statistics", dict(zip(sm.SAC_TRAIN_STATS, stats[:10])), "model", model[:10].tolist())
    assert sm.same_state(got, want) == [], sm.same_state(got, want)
    assert got["calls"] == start["calls"] + G and got["critic_step"] == G and got["actor_step"] == G
    assert all_same(got["params"], got["online_image"]) and all_same(got["params"], got["online_export"])  # the image moved with them
    assert not all_same(got["params"], start["params"]) and not all_same(got["target_image"], start["target_image"])
    if a.learned:
        assert got["ent_step"] == G and not all_same(got["log_ent_coef"], start["log_ent_coef"])
    # [4..7] against the step-by-step run's own last statistics, the means against the model's ordered sums over its per-step statistics
    assert same64(stats[4:8], [np.float64(F32(scale)) * np.float64(slots[-1, 0]), np.float64(slots[-1, sm.ACTOR_AT]), kw["first_update"] + G,
                               sm.target_updates(G, interval)])
    assert same64(stats, model) and not stats[10:].any()
    assert np.isnan(stats[3]) == (not a.learned) and np.isfinite(np.delete(stats, 3)).all()
    if case == "normalised":  # and the normaliser's statistics did enter: the raw minibatches give other weights
        raw = sm.Stack()
        raw.one_call(**kw)
        assert not all_same(raw.state()["params"], got["params"])
        raw.close()
    a.buf.check_errors()
    a.close()
    b.close()


# ---- 3. reproducibility and independence ---------------------------------------------------------------------------------------------
def run(kw=None, make=None, prepare=None, stream=None):
    s = sm.Stack(**(make or {}))
    if prepare:
        prepare(s)
    kw = dict(sm.BASE, G=4, **(kw or {}))
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
    assert d["alpha"] == d["staging"] + d["staging_bytes"] and d["slots"] == d["alpha"] + 256 and d["staging_bytes"] % 256 == 0
    floats = d["staging_bytes"] // 4 + 64 + d["max_steps"] * sm.SLOT  # the staging arrays, the alpha cell's 256 bytes, the slots
    torch.as_tensor(_DeviceArray(d["staging"], (floats,), "<f4", s.train), device=dev()).fill_(float("nan"))
    torch.cuda.synchronize()


def test_a_result_depends_on_the_state_the_seeds_and_the_update_count_and_on_nothing_else():
    ref, ref_stats = run()
    assert np.isfinite(ref_stats).all() and all(np.isfinite(p).all() for p in ref["params"])

    again, stats = run()  # two calls from identical states
    assert sm.same_state(again, ref) == [] and same64(stats, ref_stats)

    other, stats = run(stream=torch.cuda.Stream(device=dev()))
    assert sm.same_state(other, ref) == [] and same64(stats, ref_stats)

    big, stats = run(make=dict(max_batch=4 * 16, max_steps=4 * 8))  # other staging strides, another scratch, more slots
    assert sm.same_state(big, ref) == [] and same64(stats, ref_stats)

    nan, stats = run(prepare=fill_block_with_nan)  # NaN in every staging row, the alpha cell and every slot before the call
    assert sm.same_state(nan, ref) == [] and same64(stats, ref_stats)

    for change in (dict(seed=sm.SEED + 1), dict(target_seed=sm.TARGET_SEED + 1), dict(first_update=2)):  # other noise: other weights
        moved, _ = run(kw=change)
        assert not all_same(moved["params"], ref["params"]) and moved["critic_step"] == ref["critic_step"]


@pytest.mark.parametrize("interval", [1, 2, 3])
def test_one_call_of_four_steps_against_two_calls_of_two(interval):
    """The schedule restarts at every call: G = 4 moves the targets at g = 0, interval, ...; two calls of G = 2 at 0 (and 1) of each.  At
    interval 1 and 2 these are the same steps and every bit agrees; at interval 3 they are 0, 3 against 0, 2 and the targets differ."""
    one, one_stats = run(kw=dict(interval=interval))
    s = sm.Stack()
    s.one_call(**dict(sm.BASE, G=2, interval=interval))
    second = host(s.one_call(**dict(sm.BASE, G=2, interval=interval, first_update=2)))
    two = s.state()
    s.close()
    whole = [g for g in range(4) if g % interval == 0]
    halves = [g0 + g for g0 in (0, 2) for g in range(2) if g % interval == 0]
    assert second[6] == 4.0 and one_stats[6] == 4.0 and one_stats[7] == len(whole) and second[7] == len(halves) / 2
    if interval in (1, 2):
        assert whole == halves and sm.same_state(two, one) == [] and same64(second[4:6], one_stats[4:6])
    else:
        assert whole == [0, 3] and halves == [0, 2]
        assert not all_same(two["target_image"], one["target_image"])
        assert two["calls"] == one["calls"] and two["critic_step"] == one["critic_step"] == 4


# ---- 4. the refusals that need handles -------------------------------------------------------------------------------------------------
def _raw_call(s, G, B, n_actor=None, n_critic=None, fixed=False):
    """fleet_sactrain_sac_dev through train_dev, WITHOUT moving any handle to torch's stream first."""
    from fleetrl_amd import _capi

    for p in [*s.online_params, s.log_ent_coef]:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    a = _capi.FleetSacTrainArgs()
    a.gradient_steps, a.batch_size, a.target_update_interval = G, B, 2
    a.gamma, a.tau, a.lr, a.loss_scale, a.target_entropy = 0.99, 0.005, 1e-3, 0.5, -float(s.A)
    for o in range(3):
        a.beta1[o], a.beta2[o], a.eps[o], a.max_grad_norm[o] = 0.9, 0.999, 1e-8, 0.0
    a.seed, a.target_seed, a.first_update = sm.SEED, sm.TARGET_SEED, 0
    if fixed:
        a.ent_coef = s.alpha.data_ptr()
    else:
        a.log_ent_coef, a.log_ent_coef_grad = s.log_ent_coef.data_ptr(), s.log_ent_coef.grad.data_ptr()
    stats = torch.zeros(16, device=dev(), dtype=torch.float64)
    a.stats = stats.data_ptr()
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    ga, gc = [p.grad for p in s.actor_params], [p.grad for p in s.critic_params]
    s.train.train_dev(a, arr(s.actor_params), arr(ga), len(ga) if n_actor is None else n_actor, arr(s.critic_params), arr(gc),
                      len(gc) if n_critic is None else n_critic)
    return stats


def test_refusals_that_need_the_handles_launch_nothing():
    from fleetrl_amd import (DeviceAdam, DeviceNormalizer, DeviceReplayBuffer, DeviceSACNetworks, DeviceSACTrain, DeviceTD3Grad, DeviceTD3Target,
                             FleetHipError, _capi)

    s = sm.Stack(max_batch=4, max_steps=3)
    for p in [*s.online_params, s.log_ent_coef]:
        p.grad = torch.zeros_like(p)
    before = s.state()
    kw = dict(sm.BASE, G=3)
    with pytest.raises(FleetHipError, match="fleet_sactrain_sac_dev: gradient_steps must be at most max_steps = 3, got 4"):
        s.one_call(**dict(kw, G=4))
    with pytest.raises(FleetHipError, match="fleet_sactrain_sac_dev: batch_size: B must be at most max_batch = 4, got 5"):
        s.one_call(**dict(kw, B=5))
    with pytest.raises(ValueError, match="give exactly one of ent_coef"):
        s.train.train(s.actor_params, s.critic_params, gradient_steps=1, batch_size=1, gamma=0.99, tau=0.005, lr=1e-3, seed=1, target_seed=2,
                      first_update=0)
    with pytest.raises(FleetHipError, match="fleet_sactrain_sac_dev: the handle has an entropy coefficient optimiser: give log_ent_coef"):
        _raw_call(s, 3, 4, fixed=True)
    s.buf.set_position(0, False, before["calls"])
    with pytest.raises(FleetHipError, match="fleet_sactrain_sac_dev: the buffer is empty") as e:
        s.one_call(**kw)
    assert e.value.status == _capi.ERR_STATE
    s.buf.set_position(0, True, before["calls"])
    wrong = DeviceNormalizer(s.E, s.D + 1)
    s.env = wrong
    with pytest.raises(FleetHipError, match=f"fleet_sactrain_sac_dev: the normaliser has obs_dim {s.D + 1} on device 0, the buffer {s.D} on device 0"):
        s.one_call(**kw)
    s.env = None
    other = torch.cuda.Stream(device=dev())
    s.train.use_torch_stream()
    s.buf.set_stream(other.cuda_stream)
    with pytest.raises(FleetHipError, match="fleet_sactrain_sac_dev: the replay buffer, the target networks and the online networks do not launch"):
        _raw_call(s, 3, 4)
    s.buf.set_stream(torch.cuda.current_stream().cuda_stream)
    s.targets.set_stream(other.cuda_stream)
    with pytest.raises(FleetHipError, match="do not launch on one stream"):
        _raw_call(s, 3, 4)
    with pytest.raises(FleetHipError, match="fleet_sactrain_polyak_dev: the target networks launch on another stream"):
        s.train._check(s.train.lib.fleet_sactrain_polyak_dev(s.train.h, 0.5))
    s.targets.set_stream(torch.cuda.current_stream().cuda_stream)
    for tau in (1.5, float("nan"), -0.1):
        with pytest.raises(FleetHipError, match=r"fleet_sactrain_polyak_dev: tau must be in \[0, 1\], got"):
            s.train.polyak(tau)
    with pytest.raises(FleetHipError, match=r"fleet_sactrain_sac_dev: expected 6 tensors \(W, b per layer of the actor\), got 4"):
        _raw_call(s, 3, 4, n_actor=4)
    with pytest.raises(FleetHipError, match=r"fleet_sactrain_sac_dev: expected 12 tensors \(W, b per layer, critic after critic\), got 6"):
        _raw_call(s, 3, 4, n_critic=6)
    arr = (C.c_void_p * 6)(*[p.grad.data_ptr() for p in s.critic_params[:6]])
    assert s.train.lib.fleet_sactrain_scale_dev(s.train.h, arr, 6, 0.5) == _capi.ERR_INVALID
    assert "fleet_sactrain_scale_dev: expected 12 tensors" in s.train.lib.fleet_sactrain_last_error(s.train.h).decode()
    torch.cuda.synchronize()
    assert sm.same_state(s.state(), before) == []  # nothing was launched: the counter, the three step counts and every bit stayed
    stats = host(_raw_call(s, 3, 4))  # and the same arguments pass
    after = s.state()
    assert after["calls"] == before["calls"] + 3 and after["critic_step"] == 3 and after["actor_step"] == 3 and after["ent_step"] == 3
    assert np.isfinite(stats).all() and stats[7] == 2.0

    # a handle without an entropy coefficient's optimiser refuses a learned one
    f = sm.Stack(max_batch=4, max_steps=3, learned=False)
    f.log_ent_coef = torch.zeros(1, device=dev(), requires_grad=True)
    f_before = f.state()
    with pytest.raises(FleetHipError, match="fleet_sactrain_sac_dev: the handle has no entropy coefficient optimiser: give ent_coef"):
        _raw_call(f, 3, 4)
    f.log_ent_coef = None
    assert sm.same_state(f.state(), f_before) == []
    f.close()

    # create
    twin = sm.Stack(max_batch=4, max_steps=3)
    new = lambda *a, **k: DeviceSACTrain(*a, **k)  # noqa: E731
    with pytest.raises(FleetHipError, match="fleet_sactrain_create: the online and the target networks are one handle"):
        new(s.buf, s.online, s.grad, s.opt_a, s.opt_c, s.opt_e)
    actor, critics = sm.networks(s.D, s.A, (8, 8), 2, 1)
    odd = DeviceSACNetworks(actor, critics, activation="tanh")
    with pytest.raises(FleetHipError, match="fleet_sactrain_create: the online and the target networks differ in their records"):
        new(s.buf, odd, s.grad, s.opt_a, s.opt_c, s.opt_e)
    odd.close()
    wide_actor, wide_critics = sm.networks(s.D, s.A, (9, 8), 2, 1)
    odd = DeviceSACNetworks(wide_actor, wide_critics, activation="relu")
    with pytest.raises(FleetHipError, match="differ in their records"):
        new(s.buf, odd, s.grad, s.opt_a, s.opt_c, s.opt_e)
    odd.close()
    td3_actor = [(w[:s.A], b[:s.A]) if i == len(actor) - 1 else (w, b) for i, (w, b) in enumerate(actor)]
    plain, plain_t = (DeviceTD3Target(td3_actor, critics, activation="relu", output="tanh") for _ in range(2))
    pg = DeviceTD3Grad(plain, 4)
    pp = [torch.from_numpy(a.copy()).to(dev()).requires_grad_(True) for pair_ in td3_actor for a in pair_]
    pq = [torch.from_numpy(a.copy()).to(dev()).requires_grad_(True) for c in critics for pair_ in c for a in pair_]
    pa, pc = DeviceAdam(plain, pp, nets="actor"), DeviceAdam(plain, pq, nets="critic")
    with pytest.raises(FleetHipError, match="fleet_sactrain_create: the networks' actor is not a squashed Gaussian .*fleet_offpolicy_create"):
        new(s.buf, plain_t, pg, pa, pc)
    for h in (pa, pc, pg, plain, plain_t):
        h.close()
    with pytest.raises(FleetHipError, match="fleet_sactrain_create: the actor optimiser lies on another image than the gradient handle"):
        new(s.buf, s.targets, s.grad, twin.opt_a, s.opt_c, s.opt_e)
    with pytest.raises(FleetHipError, match="fleet_sactrain_create: the critic optimiser lies on another image than the gradient handle"):
        new(s.buf, s.targets, s.grad, s.opt_a, twin.opt_c, s.opt_e)
    with pytest.raises(FleetHipError, match="fleet_sactrain_create: the entropy coefficient optimiser lies on another image"):
        new(s.buf, s.targets, s.grad, s.opt_a, s.opt_c, twin.opt_e)
    with pytest.raises(FleetHipError, match=r"fleet_sactrain_create: the actor optimiser's span must be \(first_net 0, n_nets 1, no extras\)"):
        new(s.buf, s.targets, s.grad, s.opt_c, s.opt_c, s.opt_e)
    with pytest.raises(FleetHipError, match=r"fleet_sactrain_create: the critic optimiser's span must be \(first_net 1, n_nets 2, no extras\)"):
        new(s.buf, s.targets, s.grad, s.opt_a, s.opt_a, s.opt_e)
    with pytest.raises(FleetHipError, match=r"fleet_sactrain_create: the entropy coefficient optimiser's span must be \(first_net 0, n_nets 0, one extra"):
        new(s.buf, s.targets, s.grad, s.opt_a, s.opt_c, s.opt_a)
    two = torch.zeros(2, device=dev(), requires_grad=True)
    long = DeviceAdam(s.online, [two], nets="none")
    with pytest.raises(FleetHipError, match="one extra of length 1"):
        new(s.buf, s.targets, s.grad, s.opt_a, s.opt_c, long)
    long.close()
    wide = DeviceReplayBuffer(21, 3, s.D + 1, s.A)
    with pytest.raises(FleetHipError, match=f"fleet_sactrain_create: the replay buffer's obs_dim is {s.D + 1}, the networks' {s.D}"):
        new(wide, s.targets, s.grad, s.opt_a, s.opt_c, s.opt_e)
    short = DeviceReplayBuffer(21, 3, s.D, s.A - 1)
    with pytest.raises(FleetHipError, match=f"fleet_sactrain_create: the replay buffer's act_dim is {s.A - 1}, the networks' {s.A}"):
        new(short, s.targets, s.grad, s.opt_a, s.opt_c, s.opt_e)
    for bad in (0, 65537):
        with pytest.raises(FleetHipError, match=f"fleet_sactrain_create: max_steps must be in 1..65536, got {bad}"):
            new(s.buf, s.targets, s.grad, s.opt_a, s.opt_c, s.opt_e, max_steps=bad)
    assert sm.same_state(s.state(), after) == []
    for h in (wide, short, wrong):
        h.close()
    twin.close()
    s.close()


# ---- 5. the float64 parity of the whole call -----------------------------------------------------------------------------------------
def write_parity():
    """The figures are printed; they go to profiles/sac_train_parity.json only when FLEET_WRITE_PARITY=1 asks for it (a test run leaves the
    tree as it found it), merged into the cases the file already holds."""
    if os.environ.get("FLEET_WRITE_PARITY") != "1":
        return
    cases = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as fh:
            cases = json.load(fh).get("cases", {})
    cases.update(_parity)
    with open(PARITY_FILE, "w") as fh:
        json.dump({"bound": "worst |device - float64 reference| / (8 * max(max|ref32 - ref64|, 2^-24 * max|ref64|)) per tensor class; <= 1 passes",
                   "call": sm.PARITY, "cases": dict(sorted(cases.items()))}, fh, indent=1)
        fh.write("\n")


def _one_call_on_the_device(shape, salt):
    """The one call of sm.PARITY under `salt`, and the two references on the device's own minibatches and draws."""
    c = sm.parity_inputs(shape, salt)
    P, B, A = sm.PARITY, c["B"], c["A"]
    make = dict(E=c["E"], R=c["R"], D=c["D"], A=A, n_critics=2, activation=c["activation"], max_batch=B, max_steps=P["G"], lr=P["lr"],
                nets=(c["actor"], c["critics"], c["target_critics"]), ring=c["ring"], seed=7)
    s, twin = sm.Stack(**make), sm.Stack(**make)
    batches, noise, target_noise = [], [], []
    for u in range(P["G"]):  # the minibatches the call will draw (the twin's buffer counts with it) and the draws of its two keys
        b = twin.buf.sample(B)
        e_pi, e_t = torch.empty((B, A), device=dev()), torch.empty((B, A), device=dev())
        twin.online.act(b.observations, seed=sm.SEED, step=u, noise=e_pi)
        twin.online.act(b.next_observations, seed=sm.TARGET_SEED, step=u, noise=e_t)
        batches.append(tuple(host(t) for t in (b.observations, b.actions, b.next_observations, b.dones.reshape(-1), b.rewards.reshape(-1))))
        noise.append(host(e_pi)), target_noise.append(host(e_t))
    stats = host(s.one_call(G=P["G"], B=B, interval=P["interval"], first_update=0, seed=sm.SEED, target_seed=sm.TARGET_SEED, gamma=P["gamma"],
                            tau=P["tau"]))
    kw = dict(activation=c["activation"], gamma=P["gamma"], tau=P["tau"], lr=P["lr"], interval=P["interval"], log_ent_coef=c["log_ent_coef"])
    ref = {dt: sm.sac_train_reference(c["actor"], c["critics"], c["actor"], c["target_critics"], batches, noise, target_noise, dtype=dt, **kw)
           for dt in ("float64", "float32")}
    twin.close()
    return s, stats, ref, gm.ur.kink_margins(ref["float64"]["kinks"], ref["float32"]["kinks"])


@pytest.mark.parametrize("shape", sorted(sm.PARITY_SHAPES))
def test_the_whole_call_follows_sb3s_loop_under_autograd_and_torchs_adam(shape):
    """G = 4 at interval 2 with a learned alpha: every parameter, target and Adam moment within the bound of the autograd reference stepping
    torch.optim.Adam with the schedule, on the minibatches and the noise the device drew; step counts exact.  Condition (a) is asked of
    the run that is judged: a salt that misses it is not judged and the next one is taken."""
    for salt in range(gm.MAX_SALT):
        s, stats, ref, margins = _one_call_on_the_device(shape, salt)
        if all(dist >= gm.KINK_FACTOR * devi for dist, devi in margins.values()):
            break
        print(f"{shape}: salt {salt} misses condition (a): {margins}: the next salt")
        s.close()
    else:
        raise AssertionError(f"{shape}: no salt below {gm.MAX_SALT} meets condition (a)")
    r64, r32 = ref["float64"], ref["float32"]
    n = len(s.actor_params)
    tgt = s.targets.export_torch()
    got = {"actor": [host(p) for p in s.actor_params], "critics": [host(p) for p in s.critic_params], "target_actor": [host(t) for t in tgt[:n]],
           "target_critics": [host(t) for t in tgt[n:]], "log_ent_coef": [host(s.log_ent_coef)]}
    for k, opt in (("actor_opt", s.opt_a), ("critic_opt", s.opt_c), ("ent_opt", s.opt_e)):
        sd = opt.state_dict()["state"]
        assert {int(float(x["step"])) for x in sd.values()} == {sm.PARITY["G"]} == {r64[k]["step"]}
        got[k] = {mom: [host(sd[i][mom]) for i in range(len(sd))] for mom in ("exp_avg", "exp_avg_sq")}
    worst = sm.class_ratios(got, r64, r32)
    print(f"{shape}: salt {salt}, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    _parity[shape] = {"salt": salt, **{k: round(float(v), 4) for k, v in worst.items()}}
    write_parity()
    assert r64["stats"]["updated"] == [True, False, True, False] and stats[7] == 2.0 and stats[6] == 4.0
    assert all(v <= 1.0 for v in worst.values()), worst
    s.close()


# ---- 6. the example ------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_with_check():
    env = dict(os.environ, PYTHONPATH=sm.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(sm.ROOT, "examples", "sac_device_train.py"), "--updates", "3", "--gradient-steps", "4",
                        "--batch", "33", "--check"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert lines and lines[-1]["check"]["bit_equal"] is True and lines[-1]["train/n_updates"] == 12
    for d in lines:
        for k in ("train/critic_loss", "train/actor_loss", "train/ent_coef", "train/ent_coef_loss"):
            assert np.isfinite(d[k]), (k, d)
