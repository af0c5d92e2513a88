"""The handles that borrow a weight image -- `DevicePPOGrad`, `DeviceTD3Grad`, `DeviceAdam` (fleet_mlp.h `FleetMlpUser`, _handle.py
`_ImageBorrower`): a handle of the other family is refused by every create, a borrower's end leaves the image and its other borrowers
as they were, a borrower's stream is its owner's, and the cached pointer array follows a replaced `.grad`.  The smallest shapes: the
kernels' arithmetic is test_ppo_grad_gpu.py's, test_td3_grad_gpu.py's and test_adam_gpu.py's business."""
import ctypes as C
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

D, A, HID, MAX_BATCH, B = 5, 3, 8, 16, 5


def dev():
    return torch.device("cuda", 0)


def layers(sizes, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-0.5, 0.5, (o, i)).astype(np.float32), rng.uniform(-0.5, 0.5, (o,)).astype(np.float32))
            for i, o in zip(sizes[:-1], sizes[1:])]


def parameters(*nets):
    return [torch.nn.Parameter(torch.from_numpy(t.copy()).to(dev())) for net in nets for pair in net for t in pair]


def make_policy():
    from fleetrl_amd import DevicePolicy

    actor, critic = layers((D, HID, A), 1), layers((D, HID, 1), 2)
    return DevicePolicy(actor, critic_layers=critic, activation="tanh", output="clip"), parameters(actor, critic) + \
        [torch.nn.Parameter(torch.full((A,), -0.25, device=dev()))]


def make_networks(n_critics=2):
    from fleetrl_amd import DeviceTD3Target

    actor, critics = layers((D, HID, A), 3), [layers((D + A, HID, 1), 4 + c) for c in range(n_critics)]
    return DeviceTD3Target(actor, critics, activation="relu", output="tanh"), parameters(actor), parameters(*critics)


def ppo_batch():
    rng = np.random.default_rng(11)
    f = lambda *shape: torch.from_numpy(rng.uniform(-1.0, 1.0, shape).astype(np.float32)).to(dev())  # noqa: E731
    return types.SimpleNamespace(observations=f(B, D), actions=f(B, A), old_log_prob=f(B) - 3.0, advantages=f(B), returns=f(B))


def ppo_grads(g, batch, params):
    """One gradient call into NaN-filled `.grad`s; the gradients and the statistics as host arrays."""
    for p in params:
        if p.grad is not None:
            p.grad.fill_(float("nan"))
    stats = g.grad(batch, params[-1], 0.2, 0.5, 0.01, into=params)
    torch.cuda.synchronize()
    return [p.grad.cpu().numpy().copy() for p in params] + [stats.cpu().numpy().copy()]


def td3_grads(g, batch, actor_params, critic_params):
    for p in actor_params + critic_params:
        if p.grad is not None:
            p.grad.fill_(float("nan"))
    cs = g.critic_grad((batch.observations, batch.actions), batch.returns, into=critic_params)
    st = g.actor_grad(batch.observations, into=actor_params)
    torch.cuda.synchronize()
    return [p.grad.cpu().numpy().copy() for p in critic_params + actor_params] + [cs.cpu().numpy().copy(), st.cpu().numpy().copy()]


def same_bits(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(xs, ys))


def finite(xs):
    return all(np.isfinite(x).all() for x in xs)


# ---- 1, 2. a handle of the other family ---------------------------------------------------------------------------------------------
def _create(entry, last_error, owner, params):
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    params.struct_bytes = C.sizeof(params)
    h = C.c_void_p()
    rc = getattr(lib, entry)(owner.h, C.byref(params), C.byref(h))
    return rc, getattr(lib, last_error)(None).decode(), h.value


def test_ppo_create_refuses_a_networks_handle_with_one_critic():
    """n_nets == 2, net 1 ends in width 1 with no output transform: everything fleet_ppo_create looked at before it asked for the
    family.  Differentiated as a policy, the critic's first layer would read obs_dim + act_dim columns from rows of obs_dim floats."""
    from fleetrl_amd import _capi

    nets = make_networks(n_critics=1)[0]
    assert nets.describe()["n_critics"] == 1
    p = _capi.FleetPpoParams()
    p.max_batch = MAX_BATCH
    rc, why, h = _create("fleet_ppo_create", "fleet_ppo_last_error", nets, p)
    assert rc == _capi.ERR_INVALID and h is None
    assert why == "fleet_ppo_create: the handle is not a policy handle"


def test_td3_and_adam_creates_refuse_a_handle_of_the_other_family():
    from fleetrl_amd import _capi

    policy, nets = make_policy()[0], make_networks()[0]
    p = _capi.FleetTd3Params()
    p.max_batch = MAX_BATCH
    rc, why, h = _create("fleet_td3_create", "fleet_td3_last_error", policy, p)
    assert rc == _capi.ERR_INVALID and h is None and why == "fleet_td3_create: the handle is not a networks handle"
    q = _capi.FleetAdamParams()
    q.first_net, q.n_nets = 0, 1
    rc, why, h = _create("fleet_adam_create_policy", "fleet_adam_last_error", nets, q)
    assert rc == _capi.ERR_INVALID and h is None and why == "fleet_adam_create_policy: the handle is not a policy handle"


# ---- 3. lifetime and sharing -----------------------------------------------------------------------------------------------------------
def test_a_policys_borrowers_end_without_a_trace_in_the_image_or_in_each_other():
    from fleetrl_amd import DeviceAdam, DevicePPOGrad

    policy, params = make_policy()
    batch = ppo_batch()
    g = DevicePPOGrad(policy, MAX_BATCH)
    opt = DeviceAdam(policy, params, max_grad_norm=0.5)
    values = torch.empty((B, 1), device=dev())
    act0 = policy.act(batch.observations, values_out=values).cpu().numpy().copy()
    val0 = values.cpu().numpy().copy()
    grads0 = ppo_grads(g, batch, params)
    assert finite(grads0) and finite([act0, val0])
    opt.close()
    g.close()
    values.fill_(float("nan"))
    act1 = policy.act(batch.observations, values_out=values).cpu().numpy().copy()
    assert same_bits([act1, values.cpu().numpy()], [act0, val0])
    again = DevicePPOGrad(policy, MAX_BATCH)
    assert same_bits(ppo_grads(again, batch, params), grads0)


def test_a_networks_handles_borrowers_end_without_a_trace_in_the_image_or_in_each_other():
    from fleetrl_amd import DeviceAdam, DeviceTD3Grad

    nets, actor_params, critic_params = make_networks()
    batch = ppo_batch()
    zeros = torch.zeros(B, device=dev())
    target = lambda: nets.target(batch.observations, batch.returns, zeros, gamma=0.99, sigma=0.0, noise_clip=0.5, seed=1,  # noqa: E731
                                 step=0).cpu().numpy().copy()
    g = DeviceTD3Grad(nets, MAX_BATCH)
    opt_actor = DeviceAdam(nets, actor_params, nets="actor")
    opt_critic = DeviceAdam(nets, critic_params, nets="critic")
    assert (opt_actor.describe()["n_nets"], opt_critic.describe()["first_net"], opt_critic.describe()["n_nets"]) == (1, 1, 2)
    y0 = target()
    grads0 = td3_grads(g, batch, actor_params, critic_params)
    assert finite(grads0) and finite([y0])
    opt_critic.close()
    opt_actor.close()
    g.close()
    assert same_bits([target()], [y0])
    again = DeviceTD3Grad(nets, MAX_BATCH)
    assert same_bits(td3_grads(again, batch, actor_params, critic_params), grads0)


# ---- 4. the stream is the owner's ------------------------------------------------------------------------------------------------------
def test_a_borrowers_stream_is_its_owners_and_the_gradients_do_not_depend_on_it():
    from fleetrl_amd import DeviceAdam, DevicePPOGrad, DeviceTD3Grad

    policy, params = make_policy()
    nets, actor_params, critic_params = make_networks()
    batch = ppo_batch()
    ppo, td3 = DevicePPOGrad(policy, MAX_BATCH), DeviceTD3Grad(nets, MAX_BATCH)
    adam = DeviceAdam(policy, params)
    want_ppo, want_td3 = ppo_grads(ppo, batch, params), td3_grads(td3, batch, actor_params, critic_params)
    default = torch.cuda.current_stream(dev())
    assert policy._stream == default.cuda_stream == nets._stream
    side = [torch.cuda.Stream(dev()) for _ in range(3)]
    for borrower, owner, s in ((ppo, policy, side[0]), (adam, policy, side[1]), (td3, nets, side[2])):
        borrower.set_stream(s.cuda_stream)
        assert owner._stream == s.cuda_stream != default.cuda_stream
    with torch.cuda.stream(side[0]):
        side[0].wait_stream(default)
        got_ppo = ppo_grads(ppo, batch, params)
        assert policy._stream == side[0].cuda_stream
        got_td3 = td3_grads(td3, batch, actor_params, critic_params)
        assert nets._stream == side[0].cuda_stream
    assert same_bits(got_ppo, want_ppo) and same_bits(got_td3, want_td3)


# ---- 5. the cached pointer array -------------------------------------------------------------------------------------------------------
def test_the_pointer_array_is_kept_until_a_grad_is_replaced_and_then_names_the_new_one():
    from fleetrl_amd import DevicePPOGrad

    policy, params = make_policy()
    batch = ppo_batch()
    g = DevicePPOGrad(policy, MAX_BATCH)
    want = ppo_grads(g, batch, params)
    order = "the actor's then the critic's, then log_std"
    first = g._grad_pointers("grad", params, g._shapes, order)
    assert g._grad_pointers("grad", params, g._shapes, order) is first
    assert [first[i] for i in range(len(params))] == [p.grad.data_ptr() for p in params]
    old = params[2].grad
    params[2].grad = torch.full_like(old, float("nan"))
    old.fill_(7.0)
    second = g._grad_pointers("grad", params, g._shapes, order)
    assert second is not first and second[2] == params[2].grad.data_ptr() != old.data_ptr()
    assert [second[i] for i in range(len(params)) if i != 2] == [first[i] for i in range(len(params)) if i != 2]
    g.grad(batch, params[-1], 0.2, 0.5, 0.01, into=params)
    torch.cuda.synchronize()
    assert g._grad_pointers("grad", params, g._shapes, order) is second  # the launch went through the same array
    assert same_bits([params[2].grad.cpu().numpy()], [want[2]]) and bool((old == 7.0).all())
    with pytest.raises(ValueError, match=r"into: expected 9 parameters \(W, b per layer, the actor's then the critic's, then log_std\), got 8"):
        g._grad_pointers("grad", params[:-1], g._shapes, order)
