"""The policy forward on the device (fleet_policy.hip) held to the chain include/fleet_hip.h documents, bit for bit, against the
NumPy model of tests/policy_bits.py -- wherever `tanhf` does not stand in the way: every ReLU network and every one-layer head --
at the shapes the kernel itself branches on: the input width against the 128-column staging chunk and the pad to 4, every count
of 64-column groups in each layer position, wide last layers, the LDS row stride set by a late layer, two heads that differ in
width, depth and output width, load_torch and the fused normalisation at those shapes, rows that are not finite, and the tanh
networks at the new shapes under the bound of tests/test_policy_gpu.py.  The bit-exact cases carry no tolerance.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import policy_bits as pb
import policy_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def dev():
    return torch.device("cuda", 0)


def on_device(a):
    return torch.from_numpy(np.array(a)).to(dev())


def host(t):
    return t.detach().cpu().numpy()


def make_policy(name, salt=0):
    from fleetrl_amd import DevicePolicy

    c = pb.CASES[name]
    actor, critic = pb.network(name, salt)
    return DevicePolicy(actor, critic_layers=critic, activation=c["activation"], output=c["output"], low=c["low"], high=c["high"])


def differences(got, want) -> str:
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return f"shape {got.shape} against {want.shape}"
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    if not len(bad):
        return "no difference"
    r, j = bad[0]
    return (f"{len(bad)} of {got.size} words differ, in rows {sorted(set(bad[:, 0].tolist()))[:8]}; first at [{r}, {j}]: device "
            f"{got[r, j]!r} ({got[r, j].view(np.uint32):#010x}), model {want[r, j]!r} ({want[r, j].view(np.uint32):#010x})")


# ---- 1-3: one head against the chain: input widths, every width in every layer position, stride and depth, one-layer heads --------
@pytest.mark.parametrize("name", pb.BIT_CASES)
def test_one_head_equals_the_documented_chain_bit_for_bit(name):
    c = pb.CASES[name]
    pol = make_policy(name)
    assert pol.obs_dim == c["sizes"][0] and pol.act_dim == c["sizes"][-1]
    for E in pb.BATCHES:
        y = host(pol.act(on_device(pb.inputs(name, E))))
        assert pb.same_bits(y, pb.model(name, E)[0]), f"E = {E}: " + differences(y, pb.model(name, E)[0])
    if c["output"] == "clip" and c["last_scale"] != 1.0:  # (y is the E = 17 run) some outputs saturate and some do not
        lo, hi = np.float32(c["low"]), np.float32(c["high"])
        assert ((y == lo) | (y == hi)).any() and ((y > lo) & (y < hi)).any() and y.min() >= lo and y.max() <= hi
    pol.close()


# ---- 4: two heads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pb.PAIRS)
def test_two_heads_of_different_shapes_equal_the_chain_and_their_one_head_policies(name):
    """`PolicyDesc.stride` is shared and comes from the wider head; depth, widths and the output transform are per head."""
    from fleetrl_amd import DevicePolicy

    c = pb.CASES[name]
    actor, critic = pb.network(name)
    both = make_policy(name)
    actor_only = DevicePolicy(actor, activation=c["activation"], output=c["output"], low=c["low"], high=c["high"])
    critic_alone = DevicePolicy(critic, activation=c["activation"], output="none")  # the same chain as an actor-only policy
    assert both.value_dim == c["critic"][-1] == critic_alone.act_dim
    for E in pb.BATCHES:
        x = on_device(pb.inputs(name, E))
        want_a, want_v = pb.model(name, E)
        values = torch.full((E, both.value_dim), float("nan"), device=dev())
        with_values, without_values = host(both.act(x, values_out=values)), host(both.act(x))
        values = host(values)
        assert pb.same_bits(with_values, want_a), f"actor, E = {E}: " + differences(with_values, want_a)
        assert pb.same_bits(without_values, want_a), f"actor without values_out, E = {E}: " + differences(without_values, want_a)
        assert pb.same_bits(values, want_v), f"critic, E = {E}: " + differences(values, want_v)
        assert pb.same_bits(host(actor_only.act(x)), with_values) and pb.same_bits(host(critic_alone.act(x)), values)
    both.close(), actor_only.close(), critic_alone.close()


# ---- 5: load_torch at ragged shapes -----------------------------------------------------------------------------------------------
def _parameters(name, salt):
    actor, critic = pb.network(name, salt)
    return [on_device(a) for pair in actor + critic for a in pair]


def _both_heads(pol, x):
    values = torch.full((x.shape[0], pol.value_dim), float("nan"), device=dev())
    return host(pol.act(x, values_out=values)), host(values)


@pytest.mark.parametrize("name", pb.PAIRS)
def test_load_torch_relays_ragged_layers_into_the_padded_image(name):
    """in4 and out64 padding at their least mild: 389 inputs, widths 50, 400, 300, 1, 3.  Every pair, because the launch finds a
    tensor's net by walking the nets' depths: 3 + 3, 3 + 1, a one-layer head in front of a four-layer one, 2 + 2.  Weights B are the
    case's own (salt 0), the policy is created with others (salt 1) and, for the double load, goes through a third set (salt 2) first."""
    loaded, twice, fresh = make_policy(name, salt=1), make_policy(name, salt=1), make_policy(name)
    loaded.load_torch(_parameters(name, 0))
    twice.load_torch(_parameters(name, 2))
    for E in pb.BATCHES:
        x = on_device(pb.inputs(name, E))
        want = pb.model(name, E)
        after_a = _both_heads(twice, x)
        assert not pb.same_bits(after_a[0], want[0]) and not pb.same_bits(after_a[1], want[1])  # (the first load did land)
        for head, (got, new) in enumerate(zip(_both_heads(loaded, x), _both_heads(fresh, x))):
            assert pb.same_bits(got, new), f"head {head}, E = {E}, against a new policy: " + differences(got, new)
            assert pb.same_bits(got, want[head]), f"head {head}, E = {E}: " + differences(got, want[head])
    twice.load_torch(_parameters(name, 0))
    for E in pb.BATCHES:
        for head, got in enumerate(_both_heads(twice, on_device(pb.inputs(name, E)))):
            assert pb.same_bits(got, pb.model(name, E)[head]), f"loaded twice, head {head}, E = {E}: " + differences(got, pb.model(name, E)[head])
    loaded.close(), twice.close(), fresh.close()


# ---- 6: fused normalisation at the chunk edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [127, 128, 129, 1438, 8192])
def test_fused_normalisation_at_the_chunk_edges_equals_the_chain_on_the_normalisers_output(D):
    """The pattern of test_fused_normalisation_equals_the_normalisers_own_output, and one step further: the forward of the
    normaliser's own float32 output equals the bit model of it, which ties the fused path to the model and not only to the kernel."""
    from fleetrl_amd import DeviceNormalizer

    name = f"in-{D}"
    pol = make_policy(name)
    E = 17
    norm = DeviceNormalizer(E, D, clip_obs=4.0)
    gen = torch.Generator(device=dev())
    gen.manual_seed(D)
    rew, done = torch.zeros(E, device=dev(), dtype=torch.float64), torch.zeros(E, device=dev(), dtype=torch.uint8)
    for _ in range(4):  # statistics of a few steps; column 0 constant (var 0), column 1 far from zero, the last column wide
        raw = torch.randn((E, D), device=dev(), generator=gen) * 3 + 1
        raw[:, 0] = 7.0
        raw[:, 1] += 1e4
        raw[:, D - 1] *= 50
        norm.step_torch(raw, rew, done)
    norm.configure(training=False, norm_obs=True)
    raw = torch.randn((E, D), device=dev(), generator=gen) * 5 + 1
    raw[:, 1] += 1e4
    applied, _, _ = norm.step_torch(raw, rew, done)
    assert not torch.equal(applied, raw)
    want = host(pol.act(applied))
    got = host(pol.act(raw, normalizer=norm))
    assert pb.same_bits(got, want), differences(got, want)
    one = host(pol.act(raw[:1].contiguous(), normalizer=norm))  # E = 1; the normaliser's own E does not matter
    assert pb.same_bits(one, want[:1]), differences(one, want[:1])
    c = pb.CASES[name]
    model = pb.forward_bits(pb.network(name)[0], host(applied), c["activation"], c["output"])
    assert pb.same_bits(want, model), differences(want, model)
    norm.close(), pol.close()


# ---- 7: a hostile row stays in its row -------------------------------------------------------------------------------------------
HOSTILE_ROWS = (7, 20, 32)


@pytest.mark.parametrize("name", ["hostile-relu", "hostile-tanh"])
def test_a_row_that_is_not_finite_stays_in_its_row(name):
    c = pb.CASES[name]
    E = 33  # two full tiles and a ragged last row, which is hostile
    clean = np.array(pb.inputs(name, E))
    x = clean.copy()
    x[7] = np.nan
    x[20, 3], x[20, 11] = np.inf, -np.inf
    x[32, 44] = np.nan  # the last column, in the padded group of four
    pol = make_policy(name)
    y, y_clean = host(pol.act(on_device(x))), host(pol.act(on_device(clean)))
    others = [r for r in range(E) if r not in HOSTILE_ROWS]
    assert np.isfinite(y_clean).all()
    assert pb.same_bits(y[others], y_clean[others]), differences(y[others], y_clean[others])
    actor = pb.network(name)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        y64 = pm.forward64(actor, x, c["activation"], c["output"], c["low"], c["high"])
    assert np.isnan(y64[list(HOSTILE_ROWS)]).any(axis=1).all() and np.isfinite(y64[others]).all()
    assert np.array_equal(np.isnan(y), np.isnan(y64))
    if c["activation"] == "relu":
        model = pb.forward_bits(actor, x, c["activation"], c["output"], c["low"], c["high"])
        assert np.array_equal(np.isnan(y), np.isnan(model)) and pb.same_bits_or_both_nan(y, model), differences(y, model)
        assert pb.same_bits(y_clean, pb.forward_bits(actor, clean, c["activation"], c["output"], c["low"], c["high"]))
    pol.close()


@pytest.mark.parametrize("name", ["first-1", "middle-65"])
def test_an_infinite_input_reaches_no_other_row_and_its_own_row_as_the_chain_or_as_nan(name):
    """What include/fleet_hip.h promises of an input that is not finite.  The chain is not promised for it: the layout's zero
    padding multiplies the infinity (inf * 0 = NaN in a padded column of a hidden layer, which the next layer reads when its
    `in` is no multiple of 4), so 20-1-3 gives NaN where the chain gives the bias or an infinity.  Either is accepted, per element."""
    c = pb.CASES[name]
    E = 17
    clean = np.array(pb.inputs(name, E))
    x = clean.copy()
    x[3, 0], x[16, 19] = np.inf, -np.inf
    pol = make_policy(name)
    y, y_clean = host(pol.act(on_device(x))), host(pol.act(on_device(clean)))
    others = [r for r in range(E) if r not in (3, 16)]
    assert pb.same_bits(y[others], y_clean[others]) and pb.same_bits(y_clean, pb.model(name, E)[0])
    model = pb.forward_bits(pb.network(name)[0], x, c["activation"], c["output"])
    print(f"{name}: rows 3 and 16 on the device {y[[3, 16]].tolist()}, in the chain {model[[3, 16]].tolist()}")
    assert (np.isnan(y[[3, 16]]) | (y[[3, 16]].view(np.int32) == model[[3, 16]].view(np.int32))).all()
    assert not np.isfinite(model[3]).all() and not np.isfinite(y[[3, 16]]).any()
    pol.close()


# ---- 8: the tanh networks at the new shapes -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tanh_reference(name, E):
    """(float64 model, eps_ref = max |torch-CPU float32 - float64 model|), as policy_model.reference."""
    c = pb.CASES[name]
    actor, x = pb.network(name)[0], pb.inputs(name, E)
    y64 = pm.forward64(actor, x, c["activation"], c["output"], c["low"], c["high"])
    y32 = pm.forward_torch32(actor, x, c["activation"], c["output"], c["low"], c["high"])
    return y64, float(np.max(np.abs(y32.astype(np.float64) - y64)))


@pytest.mark.parametrize("name", pb.TANH_CASES)
def test_tanh_networks_at_the_new_shapes_stay_within_the_projects_bound(name):
    """The rule of test_forward_stays_within_eight_times_the_float32_reference_error, unchanged: 8 * max(eps_ref, 2^-24 max|out|)
    against the float64 model.  Column groups 4 and 6 (193..256, 321..384), an exact 256 and 384, a last layer of three groups."""
    pol = make_policy(name)
    for E in pb.BATCHES:
        y = host(pol.act(on_device(pb.inputs(name, E)))).astype(np.float64)
        y64, eps_ref = tanh_reference(name, E)
        err = float(np.max(np.abs(y - y64)))
        bound = 8 * max(eps_ref, 2.0 ** -24 * float(np.max(np.abs(y64))))
        print(f"{name} E={E}: eps_ref {eps_ref:.3g} device {err:.3g} bound {bound:.3g}")
        assert y.shape == y64.shape and err <= bound, (E, err, bound)
    pol.close()


@pytest.mark.parametrize("name", pb.TANH_CASES[::2])
def test_a_row_of_a_tanh_network_does_not_depend_on_the_batch_or_its_position(name):
    """test_a_row_does_not_depend_on_the_batch_or_its_position at the new shapes (the output transform plays no part: one of two)."""
    def bits(t):
        return host(t).view(np.int32)

    pol = make_policy(name)
    T = pol.tile_rows
    E = 16 * T + 1
    x = on_device(pb.inputs(name, E))
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
