"""The optimiser step on the device (fleet_adam.hip) against the bit model of tests/adam_model.py, against torch's float64
clip_grad_norm_ + Adam under the project's rule, the weight image against the stepped parameters, and what a result may not depend on."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import adam_model as am
import policy_bits as pb

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARITY_FILE = os.path.join(am.ROOT, "profiles", "adam_parity.json")
F32 = np.float32
INF = float("inf")
_parity = {}


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy().copy()


def layers_of(name, tensors) -> list:
    """`tensors` (W, b per layer of every net) as one [(W, b), ...] list per net."""
    out, i = [], 0
    for sizes in am.CASES[name]["nets"]:
        n = len(sizes) - 1
        out.append([(tensors[i + 2 * l], tensors[i + 2 * l + 1]) for l in range(n)])
        i += 2 * n
    return out


def make_image(name, tensors=None):
    from fleetrl_amd import DevicePolicy, DeviceTD3Target

    c = am.CASES[name]
    nets = layers_of(name, list(am.initial(name)) if tensors is None else tensors)
    if c["kind"] == "policy":
        return DevicePolicy(nets[0], critic_layers=nets[1] if len(nets) > 1 else None, activation=c["activation"], output=c["output"])
    return DeviceTD3Target(nets[0], nets[1:], activation=c["activation"], output=c["output"])


def open_case(name, clip, params=None):
    """The image, torch's parameters of every net (then the extras), and one optimiser per span with its slice of the parameters."""
    from fleetrl_amd import DeviceAdam

    assert all(am.facts_of(name).values()), am.facts_of(name)  # the table's conditions, enforced in every case
    image = make_image(name)
    params = [torch.nn.Parameter(on_device(a)) for a in am.initial(name)] if params is None else params
    opts = []
    for nets, first, n in am.spans(name):
        sl = am.span_slice(name, first, n)
        opt = DeviceAdam(image, params[sl], nets=nets, lr=am.LR, betas=am.BETAS, eps=am.CASES[name]["eps"],
                         max_grad_norm=am.MAX_GRAD_NORM if clip else None)
        d = opt.describe()
        assert (d["norm_chunk"], d["step_tile"]) == (am.CHUNK, am.TILE)  # the launch shapes the table was drawn for
        opts.append((opt, params[sl], first, n))
    return image, params, opts


def set_grads(ps, grads):
    for p, g in zip(ps, grads):
        if p.grad is None:
            p.grad = on_device(g)
        else:
            p.grad.copy_(on_device(g))


def exported_state(opt):
    sd = opt.state_dict()["state"]
    return [host(sd[i]["exp_avg"]) for i in range(len(sd))], [host(sd[i]["exp_avg_sq"]) for i in range(len(sd))]


def image_tensors(opt):
    """The whole image an optimiser stands on; a TD3 image's own export must say the same."""
    out = [host(t) for t in opt.export_image()]
    if hasattr(opt.image, "export_torch"):
        assert all(pb.same_bits(a, host(b)) for a, b in zip(out, opt.image.export_torch()))
    return out


@functools.lru_cache(maxsize=None)
def device_run(name, clip):
    """Six steps of every span's optimiser: per span and step (params, exp_avg, exp_avg_sq, norm) as host arrays; per step the
    exported image and all parameters; and the end's image and parameters, kept for the forward tests."""
    image, params, opts = open_case(name, clip)
    norm = torch.full((1,), np.nan, device=dev())
    per_span = {(first, n): [] for _, _, first, n in opts}
    images = []
    for s in range(am.STEPS):
        for opt, ps, first, n in opts:
            set_grads(ps, am.gradients(name, first, n, s))
            before = [host(p.grad) for p in ps]
            opt.step(norm_out=norm)
            assert all(pb.same_bits(a, host(p.grad)) for a, p in zip(before, ps))  # the gradients are read only
            m, v = exported_state(opt)
            assert opt.describe()["step"] == s + 1
            per_span[(first, n)].append(([host(p) for p in ps], m, v, host(norm)[0]))
        images.append((image_tensors(opts[0][0]), [host(p) for p in params]))
    return per_span, images, image, params, opts


ALL = [(name, clip) for name in sorted(am.CASES) for clip in (True, False)]


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clip", ALL)
def test_parameters_state_and_norm_equal_the_model_bit_for_bit(name, clip):
    per_span = device_run(name, clip)[0]
    for (first, n), steps in per_span.items():
        want = am.run(name, first, n, clip)
        for s in range(am.STEPS):
            for k, what in enumerate(("p", "exp_avg", "exp_avg_sq")):
                for i, (a, b) in enumerate(zip(steps[s][k], want[s][k])):
                    assert pb.same_bits(a, b), (first, n, s, what, i, float(np.abs(a - b).max()))
            assert pb.same_bits(steps[s][3], want[s][3]), (first, n, s, "norm", steps[s][3], want[s][3])


# ---- 2. the project's bound ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clip", ALL)
def test_every_tensor_stays_within_the_bound_of_torchs_float64_run(name, clip):
    per_span = device_run(name, clip)[0]
    worst = 0.0
    for (first, n), steps in per_span.items():
        r64, r32 = am.torch_reference(name, first, n, clip, True), am.torch_reference(name, first, n, clip, False)
        for s in range(am.STEPS):
            for k, r in am.bound_ratios(steps[s], r64[s], r32[s]).items():
                _parity[f"{name}/{'clip' if clip else 'noclip'}/span{first}+{n}/step{s}/{k}"] = r
                worst = max(worst, r)
    print(f"{name} clip={clip}: worst error / bound {worst:.3f}")
    ranked = sorted(_parity.items(), key=lambda kv: -kv[1])
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as f:
        json.dump({"rule": "|device - torch float64| <= 8 * max(|torch float32 - torch float64|, 2^-24 max|torch float64|), per tensor and step",
                   "worst": ranked[0], "ratios": dict(ranked)}, f, indent=1)
    assert worst <= 1.0


# ---- 3. the image equals the parameters ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clip", ALL)
def test_the_image_equals_the_parameters_after_every_step(name, clip):
    images = device_run(name, clip)[1]
    n_img = len(am.shapes(name, extras=False))
    for s, (img, ps) in enumerate(images):
        assert len(img) == n_img
        for i, (a, b) in enumerate(zip(img, ps)):
            assert pb.same_bits(a, b), (s, i)


@pytest.mark.parametrize("name", sorted(am.CASES))
def test_the_stepped_images_forward_equals_a_fresh_image_of_the_stepped_parameters(name):
    _, _, image, params, _ = device_run(name, True)
    fresh = make_image(name, [host(p) for p in params[:len(am.shapes(name, extras=False))]])
    D = am.CASES[name]["nets"][0][0]
    rng = np.random.default_rng(am.seed(name, "obs"))
    obs = on_device(rng.standard_normal((19, D)).astype(F32))
    if am.CASES[name]["kind"] == "policy":
        two = len(am.CASES[name]["nets"]) > 1
        va, vb = (torch.full((19, 1), np.nan, device=dev()) for _ in range(2))
        a, b = image.act(obs, values_out=va if two else None), fresh.act(obs, values_out=vb if two else None)
        assert pb.same_bits(host(a), host(b)) and np.isfinite(host(a)).all()
        assert not two or pb.same_bits(host(va), host(vb))
    else:
        rew, done = on_device(rng.standard_normal(19).astype(F32)), torch.zeros(19, device=dev())
        outs = []
        for t in (image, fresh):
            na, q = torch.full((19, t.act_dim), np.nan, device=dev()), torch.full((19, t.n_critics), np.nan, device=dev())
            y = t.target(obs, rew, done, gamma=0.99, sigma=0.0, noise_clip=0.5, low=-INF, high=INF, seed=1, step=0, next_actions_out=na, q_out=q)
            outs.append((host(y), host(na), host(q)))
        assert all(pb.same_bits(x, y) and np.isfinite(x).all() for x, y in zip(*outs))
    fresh.close()


# ---- 4. spans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(am.CASES) if am.CASES[n]["kind"] == "td3"])
def test_an_optimiser_leaves_the_other_spans_parameters_and_image_alone(name):
    image, params, opts = open_case(name, True)
    for opt, ps, first, n in opts:
        set_grads(ps, am.gradients(name, first, n, 0))
    for k, (opt, ps, first, n) in enumerate(opts):
        sl = am.span_slice(name, first, n)
        before_p, before_img = [host(p) for p in params], image_tensors(opt)
        opt.step()
        after_p, after_img = [host(p) for p in params], image_tensors(opt)
        for i in range(len(params)):
            mine = sl.start <= i < sl.stop
            assert pb.same_bits(before_p[i], after_p[i]) != mine and pb.same_bits(before_img[i], after_img[i]) != mine, (k, i)


def test_an_optimiser_without_a_net_is_a_flat_adam_and_equals_the_model():
    from fleetrl_amd import DeviceAdam

    image = make_image("one-layer-5x3")
    rng = np.random.default_rng(am.seed("flat", "init"))
    p0 = rng.standard_normal(am.FLAT_LEN).astype(F32)
    p = torch.nn.Parameter(on_device(p0))
    opt = DeviceAdam(image, [p], nets="none", lr=am.LR, eps=1e-8, max_grad_norm=am.MAX_GRAD_NORM)
    before = image_tensors(opt)
    d = opt.describe()
    assert (d["n_nets"], d["n_extra"], d["extra_len"], d["n_tensors"], d["n_elements"], d["state_bytes"], d["step"]) == \
        (0, 1, [am.FLAT_LEN], 1, am.FLAT_LEN, 8 * am.FLAT_LEN, 0)
    norm = torch.full((1,), np.nan, device=dev())
    P, M, V = [p0], [np.zeros_like(p0)], [np.zeros_like(p0)]
    for s in range(am.STEPS):
        g = am.scaled_gradients([(am.FLAT_LEN,)], "flat", s)
        set_grads([p], g)
        opt.step(norm_out=norm)
        P, M, V, want = am.step(P, g, M, V, s + 1, lr=am.LR, eps=1e-8, max_grad_norm=am.MAX_GRAD_NORM)
        m, v = exported_state(opt)
        assert pb.same_bits(host(p), P[0]) and pb.same_bits(m[0], M[0]) and pb.same_bits(v[0], V[0]) and pb.same_bits(host(norm)[0], want), s
    assert all(pb.same_bits(a, b) for a, b in zip(before, image_tensors(opt)))


# ---- 5. what a result may not depend on ----------------------------------------------------------------------------------------------
NAME5 = "ragged-33"


def _steps_on(opt, ps, name, first, n, steps):
    for s in steps:
        set_grads(ps, am.gradients(name, first, n, s))
        opt.step()


def _equals_model(ps, opt, name, first, n, s, clip=True):
    want = am.run(name, first, n, clip)[s]
    m, v = exported_state(opt)
    return all(pb.same_bits(host(p), w) for p, w in zip(ps, want[0])) and all(pb.same_bits(a, w) for a, w in zip(m, want[1])) and \
        all(pb.same_bits(a, w) for a, w in zip(v, want[2]))


def test_two_handles_and_another_stream_agree():
    ia, pa, oa = open_case(NAME5, True)
    ib, pbb, ob = open_case(NAME5, True)
    (opt_a, ps_a, first, n), (opt_b, ps_b, _, _) = oa[0], ob[0]
    _steps_on(opt_a, ps_a, NAME5, first, n, range(3))
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _steps_on(opt_b, ps_b, NAME5, first, n, range(3))
    side.synchronize()
    assert all(pb.same_bits(host(a), host(b)) for a, b in zip(ps_a, ps_b))
    assert all(pb.same_bits(a, b) for a, b in zip(image_tensors(opt_a), image_tensors(opt_b)))
    assert _equals_model(ps_a, opt_a, NAME5, first, n, 2) and _equals_model(ps_b, opt_b, NAME5, first, n, 2)


def test_parameters_and_gradients_off_the_16_byte_alignment_agree():
    """Every parameter and every gradient is a view one float into a buffer of its own: the addresses are 4 modulo 16."""
    def view(a):
        buf = torch.zeros(a.size + 1, device=dev())
        t = buf[1:].view(a.shape)
        t.copy_(on_device(a))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t

    params = [view(a) for a in am.initial(NAME5)]
    for p in params:
        p.grad = view(np.zeros(tuple(p.shape), F32))
    image, _, opts = open_case(NAME5, True, params=params)
    opt, ps, first, n = opts[0]
    _steps_on(opt, ps, NAME5, first, n, range(2))
    assert all(p.grad.data_ptr() % 16 == 4 for p in ps)
    assert _equals_model(ps, opt, NAME5, first, n, 1)
    assert all(pb.same_bits(a, host(p)) for a, p in zip(image_tensors(opt), params))


def test_a_state_exported_and_loaded_into_a_second_handle_continues_alike():
    _, _, oa = open_case(NAME5, True)
    opt_a, ps_a, first, n = oa[0]
    _steps_on(opt_a, ps_a, NAME5, first, n, range(3))
    sd = opt_a.state_dict()
    assert int(sd["state"][0]["step"]) == 3 and sd["param_groups"][0]["lr"] == am.LR and sd["param_groups"][0]["eps"] == 1e-5
    ib, _, ob = open_case(NAME5, True, params=[torch.nn.Parameter(p.detach().clone()) for p in ps_a])
    ib.load_torch([p for p in ob[0][1][:len(am.shapes(NAME5, extras=False))]])
    opt_b, ps_b = ob[0][0], ob[0][1]
    assert opt_b.state_dict()["state"] == {} and opt_b.describe()["step"] == 0
    opt_b.load_state_dict(sd)
    assert opt_b.describe()["step"] == 3
    _steps_on(opt_b, ps_b, NAME5, first, n, range(3, 6))
    assert _equals_model(ps_b, opt_b, NAME5, first, n, 5)
    assert all(pb.same_bits(a, host(p)) for a, p in zip(image_tensors(opt_b), ps_b))


# ---- 6. the state and torch.optim.Adam -------------------------------------------------------------------------------------------------
def test_the_exported_state_continues_in_torchs_adam_within_the_bound():
    name = NAME5
    _, _, opts = open_case(name, True)
    opt, ps, first, n = opts[0]
    _steps_on(opt, ps, name, first, n, range(3))
    sd, start = opt.state_dict(), [host(p) for p in ps]
    grads = [am.gradients(name, first, n, s) for s in range(3, 6)]
    kw = dict(eps=am.CASES[name]["eps"], max_grad_norm=am.MAX_GRAD_NORM, state=sd)
    r64, r32 = am.torch_run(start, grads, torch.float64, **kw), am.torch_run(start, grads, torch.float32, **kw)
    norm = torch.full((1,), np.nan, device=dev())
    for s in range(3):
        set_grads(ps, grads[s])
        opt.step(norm_out=norm)
        m, v = exported_state(opt)
        ratios = am.bound_ratios(([host(p) for p in ps], m, v, host(norm)[0]), r64[s], r32[s])
        print(s, ratios)
        assert all(r <= 1.0 for r in ratios.values()), (s, ratios)


def test_a_loaded_step_count_of_1000_follows_the_model_bit_for_bit():
    name = "one-layer-5x3"
    _, _, opts = open_case(name, False)
    opt, ps, first, n = opts[0]
    rng = np.random.default_rng(am.seed(name, "state"))
    M = [(0.01 * rng.standard_normal(tuple(p.shape))).astype(F32) for p in ps]
    V = [(1e-4 * rng.random(tuple(p.shape)) + 1e-8).astype(F32) for p in ps]
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(1000.0), "exp_avg": torch.from_numpy(M[i]), "exp_avg_sq": torch.from_numpy(V[i])} for i in range(len(ps))}
    opt.load_state_dict(sd)
    assert opt.describe()["step"] == 1000
    P = [host(p) for p in ps]
    for s in range(2):
        g = am.gradients(name, first, n, s)
        set_grads(ps, g)
        opt.step()
        P, M, V, _ = am.step(P, g, M, V, 1001 + s, lr=am.LR, betas=am.BETAS, eps=am.CASES[name]["eps"])
        m, v = exported_state(opt)
        assert all(pb.same_bits(host(p), w) for p, w in zip(ps, P)) and all(pb.same_bits(a, w) for a, w in zip(m, M))
        assert all(pb.same_bits(a, w) for a, w in zip(v, V))
    assert opt.describe()["step"] == 1002 and int(opt.state_dict()["state"][0]["step"]) == 1002


# ---- 7. the rate per call ----------------------------------------------------------------------------------------------------------------
def test_the_learning_rate_is_taken_per_call_and_zero_moves_the_state_alone():
    name = "td3-5x3-two-critics"
    image, params, opts = open_case(name, False)
    opt, ps, first, n = opts[1]
    P = [host(p) for p in ps]
    M, V = [np.zeros_like(a) for a in P], [np.zeros_like(a) for a in P]
    for s, lr in enumerate((3e-4, 1e-4, 0.0)):
        g = am.gradients(name, first, n, s)
        set_grads(ps, g)
        before_p, before_img, (before_m, before_v) = [host(p) for p in ps], image_tensors(opt), exported_state(opt)
        opt.step(lr=lr)
        P, M, V, _ = am.step(P, g, M, V, s + 1, lr=lr, betas=am.BETAS, eps=am.CASES[name]["eps"])
        m, v = exported_state(opt)
        assert all(pb.same_bits(host(p), w) for p, w in zip(ps, P)) and all(pb.same_bits(a, w) for a, w in zip(m, M))
        assert all(pb.same_bits(a, w) for a, w in zip(v, V))
        still = all(pb.same_bits(a, host(p)) for a, p in zip(before_p, ps)) and all(pb.same_bits(a, b) for a, b in zip(before_img, image_tensors(opt)))
        assert still == (lr == 0.0)
        assert not any(pb.same_bits(a, b) for a, b in zip(before_m, m)) and not any(pb.same_bits(a, b) for a, b in zip(before_v, v))


# ---- 8. NaN --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
def test_a_nan_gradient_spreads_as_in_torch(clip):
    name = "ragged-33"
    image, params, opts = open_case(name, clip)
    opt, ps, first, n = opts[0]
    g = [np.array(a) for a in am.gradients(name, first, n, 0)]
    g[2][7, 11] = np.nan  # the second layer's W [25, 31]
    set_grads(ps, g)
    norm = torch.full((1,), 0.0, device=dev())
    opt.step(norm_out=norm)
    zero = [np.zeros_like(a) for a in g]
    P, M, V, want_norm = am.step(list(am.initial(name)), g, zero, zero, 1, lr=am.LR, betas=am.BETAS, eps=am.CASES[name]["eps"],
                                 max_grad_norm=am.MAX_GRAD_NORM if clip else None)
    got = [host(p) for p in ps]
    assert np.isnan(host(norm)[0]) and np.isnan(want_norm)
    assert all(pb.same_bits_or_both_nan(a, b) for a, b in zip(got, P))
    img = image_tensors(opt)
    assert all(pb.same_bits_or_both_nan(a, b) for a, b in zip(img, got))
    if clip:
        assert all(np.isnan(a).all() for a in got)
    else:
        assert sum(int(np.isnan(a).sum()) for a in got) == 1 and np.isnan(got[2][7, 11]) and np.isnan(img[2][7, 11])
    # torch agrees on where the NaNs are
    ref = am.torch_run(list(am.initial(name)), [g], torch.float32, eps=am.CASES[name]["eps"], max_grad_norm=am.MAX_GRAD_NORM if clip else None)[0][0]
    assert all(np.array_equal(np.isnan(a), np.isnan(b)) for a, b in zip(got, ref))


# ---- 9. the refusals that need a handle ----------------------------------------------------------------------------------------------
def test_a_wrong_count_and_a_wrong_shape_are_refused():
    from fleetrl_amd import DeviceAdam, _capi
    from fleetrl_amd._capi import FleetHipError

    name = "one-layer-5x3"
    image, params, opts = open_case(name, True)
    opt, ps, first, n = opts[0]
    set_grads(ps, am.gradients(name, first, n, 0))
    before = [host(p) for p in ps]
    a = _capi.FleetAdamStepArgs()
    a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = 3e-4, 0.9, 0.999, 1e-8, 0.5
    k = len(ps) - 1
    pa, ga = (C.c_void_p * k)(*[p.data_ptr() for p in ps[:k]]), (C.c_void_p * k)(*[p.grad.data_ptr() for p in ps[:k]])
    with pytest.raises(FleetHipError, match=r"fleet_adam_step_dev: expected 5 tensors .* got 4"):
        opt.step_dev(a, pa, ga, k)
    st = C.c_int64(0)
    assert opt.lib.fleet_adam_state_dev(opt.h, _capi.ADAM_STATE_EXPORT, pa, ga, k, C.byref(st)) == _capi.ERR_INVALID
    assert "fleet_adam_state_dev: expected 5 tensors" in opt.lib.fleet_adam_last_error(opt.h).decode()
    torch.cuda.synchronize()
    assert opt.describe()["step"] == 0 and all(pb.same_bits(b, host(p)) for b, p in zip(before, ps))
    wrong = list(ps)
    wrong[0] = torch.nn.Parameter(torch.zeros((3, 6), device=dev()))  # a span tensor of the wrong length
    with pytest.raises(ValueError, match=r"expected a parameter of shape \(3, 5\), got \(3, 6\)"):
        DeviceAdam(image, wrong, max_grad_norm=0.5)
    with pytest.raises(ValueError, match="at most 2 extras"):
        DeviceAdam(image, list(ps) + [ps[-1], ps[-1]])
    with pytest.raises(FleetHipError, match="fleet_adam_create_policy: the span of nets 1 .. 2 lies outside the image's 2 nets"):
        p = _capi.FleetAdamParams()
        p.struct_bytes, p.first_net, p.n_nets = C.sizeof(p), 1, 2
        h = C.c_void_p()
        rc = opt.lib.fleet_adam_create_policy(image.h, C.byref(p), C.byref(h))
        raise FleetHipError(rc, opt.lib.fleet_adam_last_error(None).decode())
    with pytest.raises(FleetHipError, match="fleet_adam_create_qtarget: the handle is not a networks handle"):
        p = _capi.FleetAdamParams()
        p.struct_bytes, p.first_net, p.n_nets = C.sizeof(p), 0, 1
        h = C.c_void_p()
        rc = opt.lib.fleet_adam_create_qtarget(image.h, C.byref(p), C.byref(h))
        raise FleetHipError(rc, opt.lib.fleet_adam_last_error(None).decode())
