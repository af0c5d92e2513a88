"""The bit model of the policy forward (tests/policy_bits.py) on its own: the float32 fused multiply-add against exact rational
arithmetic, at random and where going through float64 would round twice; the chain against the float64 model; known answers that
tell the summation order, the fusion and the place of the bias apart.  No GPU and no library."""
import random
from fractions import Fraction

import numpy as np
import pytest

import policy_bits as pb
import policy_model as pm

f32 = np.float32


def round32(q: Fraction) -> np.float32:
    """A rational, rounded once to the nearest float32, ties to even (normal range only)."""
    if q == 0:
        return f32(0.0)
    e = q.numerator.bit_length() - q.denominator.bit_length() - 24  # within one of the exponent
    while abs(q) / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while abs(q) / Fraction(2) ** e < 2 ** 23:
        e -= 1
    n = round(q / Fraction(2) ** e)  # (Python rounds a Fraction's tie to even)
    assert -126 <= e + 23 and e + 23 <= 127, "outside the normal range"
    r = f32(float(Fraction(n) * Fraction(2) ** e))
    assert Fraction(float(r)) == Fraction(n) * Fraction(2) ** e
    return r


def exact(x, w, acc) -> np.float32:
    return round32(Fraction(float(x)) * Fraction(float(w)) + Fraction(float(acc)))


def through_float64(x, w, acc) -> np.float32:
    """What a model without the round-to-odd step would compute: two roundings."""
    return f32(np.float64(x) * np.float64(w) + np.float64(acc))


def test_fma32_equals_exact_rational_arithmetic_on_random_triples():
    rng = np.random.default_rng(0)
    n = 20000
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))).astype(f32)
    w = (rng.standard_normal(n) * np.exp2(rng.integers(-8, 9, n))).astype(f32)
    acc = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 13, n))).astype(f32)
    # a third of them with an accumulator near -x*w (cancellation), a third with one that dwarfs the product
    acc[: n // 3] = (-(x[: n // 3].astype(np.float64) * w[: n // 3]) * (1 + rng.integers(-4, 5, n // 3) * 2.0 ** -23)).astype(f32)
    acc[n // 3: 2 * n // 3] *= f32(2.0 ** 20)
    got = pb.fma32(x, w, acc)
    want = np.array([exact(*t) for t in zip(x, w, acc)], f32)
    assert got.dtype == f32 and pb.same_bits(got, want)


# acc + x*w = a float32 midpoint -+ 2^-40, far below float64's last place at 2^30 (2^-22): float64 rounds the sum ONTO the midpoint
# and the tie then goes to the even neighbour, which is the wrong one whenever the odd one was nearer.
_UP = (f32(2.0 ** 6 * (1 + 2.0 ** -23)), f32(1 - 2.0 ** -23))  # x*w = 2^6 - 2^-40 exactly
_ODD, _EVEN = f32(2.0 ** 30 + 2.0 ** 7), f32(2.0 ** 30)  # neighbours: the last place at 2^30 is 2^7
DOUBLE_ROUNDING = [
    # (x, w, acc, the correctly rounded result)
    (_UP[0], _UP[1], _ODD, _ODD),                # odd + 2^6 - 2^-40: just below the midpoint above -> stays; float64 first: up to even
    (-_UP[0], _UP[1], _ODD, _ODD),               # odd - 2^6 + 2^-40: just above the midpoint below -> stays; float64 first: down to even
    (_UP[0], -_UP[1], -_ODD, -_ODD),             # both mirrored
    (-_UP[0], -_UP[1], -_ODD, -_ODD),
    (-_UP[0], _UP[1], f32(2.0 ** 30 + 2.0 ** 8), f32(2.0 ** 30 + 2.0 ** 8)),  # even - 2^6 + 2^-40: stays either way (the control)
    (_UP[0], _UP[1], _EVEN, _EVEN),              # even + 2^6 - 2^-40: stays either way (the control)
]


@pytest.mark.parametrize("x,w,acc,want", DOUBLE_ROUNDING)
def test_fma32_rounds_once_where_float64_would_round_twice(x, w, acc, want):
    assert Fraction(float(x)) * Fraction(float(w)) in (Fraction(2) ** 6 - Fraction(2) ** -40, -(Fraction(2) ** 6 - Fraction(2) ** -40))
    assert exact(x, w, acc) == want
    got = pb.fma32(x, w, acc)
    assert pb.same_bits(got, want), (got, want)


def test_the_double_rounding_cases_do_catch_a_model_that_goes_through_float64():
    wrong = [through_float64(x, w, acc) != want for x, w, acc, want in DOUBLE_ROUNDING]
    assert wrong == [True, True, True, True, False, False]


def test_fma32_cancellation_zero_signs_and_non_finite_operands():
    assert pb.same_bits(pb.fma32(f32(3), f32(5), f32(-15)), f32(0.0))  # exact cancellation: +0
    assert pb.same_bits(pb.fma32(f32(0), f32(-2), f32(0.0)), f32(0.0))  # -0 + +0 = +0: a zero input row leaves the accumulator +0
    assert pb.same_bits(pb.fma32(f32(0), f32(-2), f32(-0.0)), f32(-0.0))
    x, w = f32(1 + 2.0 ** -23), f32(1 - 2.0 ** -23)
    assert pb.same_bits(pb.fma32(x, w, f32(-1)), f32(-2.0 ** -46))  # the product's low half survives: fused
    assert f32(x * w) + f32(-1) == 0  # ... which a separate multiply and add loses
    assert np.isposinf(pb.fma32(f32(np.inf), f32(2), f32(1))) and np.isneginf(pb.fma32(f32(np.inf), f32(-2), f32(1)))
    assert np.isnan(pb.fma32(f32(np.inf), f32(2), f32(-np.inf))) and np.isnan(pb.fma32(f32(np.nan), f32(2), f32(1)))
    assert np.isnan(pb.fma32(f32(np.inf), f32(0), f32(1)))
    got = pb.fma32(np.array([[1], [2]], f32), np.array([3, 4, 5], f32), f32(1))  # broadcasting: a column of x against a row of W
    assert got.shape == (2, 3) and np.array_equal(got, np.array([[4, 5, 6], [7, 9, 11]], f32))
    with pytest.raises(AssertionError):
        pb.fma32(f32(2.0 ** 100), f32(2.0 ** 100), f32(0))  # overflow of a finite chain is refused, not modelled
    with pytest.raises(AssertionError):
        pb.fma32(f32(2.0 ** -100), f32(2.0 ** -40), f32(0))  # so is a subnormal result


def test_fma32_on_random_bit_patterns_against_python_fractions():
    """Operands drawn as raw significands and exponents, so every bit of the significand is in play."""
    rnd = random.Random(1)

    def draw(emin, emax):
        return f32((-1) ** rnd.getrandbits(1) * (2 ** 23 + rnd.getrandbits(23)) * 2.0 ** (rnd.randint(emin, emax) - 23))

    triples = [(draw(-10, 10), draw(-10, 10), draw(-30, 30)) for _ in range(5000)]
    got = pb.fma32(*(np.array(c, f32) for c in zip(*triples)))
    assert pb.same_bits(got, np.array([exact(*t) for t in triples], f32))


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,activation,output", [((20, 33, 70, 4), "relu", "clip"), ((45, 9), "tanh", "none")])
def test_forward_stays_within_the_float32_reference_error_of_the_float64_model(sizes, activation, output):
    """The rule of tests/test_policy_gpu.py: within 8 * max(eps_ref, 2^-24 max|out|) of the float64 model, eps_ref being torch-CPU
    float32's own distance from it."""
    rng = np.random.default_rng(5)
    layers = pm.random_layers(rng, sizes)
    layers[-1] = (layers[-1][0] * f32(4), layers[-1][1])  # some outputs reach the clip
    x = np.clip(rng.standard_normal((17, sizes[0])) * 3, -10, 10).astype(f32)
    lo, hi = pb.CLIP
    y = pb.forward_bits(layers, x, activation, output, lo, hi)
    y64 = pm.forward64(layers, x, activation, output, f32(lo), f32(hi))
    eps_ref = float(np.max(np.abs(pm.forward_torch32(layers, x, activation, output, float(f32(lo)), float(f32(hi))).astype(np.float64) - y64)))
    err = float(np.max(np.abs(y.astype(np.float64) - y64)))
    bound = 8 * max(eps_ref, 2.0 ** -24 * float(np.max(np.abs(y64))))
    print(f"{sizes}: eps_ref {eps_ref:.3g} model {err:.3g} bound {bound:.3g}")
    assert y.shape == y64.shape and y.dtype == f32 and err <= bound
    if output == "clip":
        assert (y == f32(lo)).any() and (y == f32(hi)).any() and ((y > f32(lo)) & (y < f32(hi))).any()


def test_forward_known_answers_tell_the_order_the_fusion_and_the_bias_apart():
    big = f32(2.0 ** 24)
    one = np.ones((1, 3), f32)
    up, down = np.array([[big, 1, -big]], f32), np.array([[-big, 1, big]], f32)
    zero = np.zeros(1, f32)
    # ascending k: 2^24, then 2^24 + 1 -> 2^24 (a tie, to even), then 0.  Descending: -2^24, -(2^24 - 1) (exact), then 1.
    assert pb.forward_bits([(up, zero)], one, "relu", "none")[0, 0] == 0.0
    assert pb.forward_bits([(down, zero)], one, "relu", "none")[0, 0] == 1.0  # = the first network summed from the far end
    assert pb.forward_bits([(up[:, ::-1], zero)], one, "relu", "none")[0, 0] == 1.0
    # the bias goes in last: as the accumulator's initial value the 1 would be absorbed by 2^24 at once (0 instead of 1) ...
    w = np.array([[big, -big]], f32)
    assert pb.forward_bits([(w, np.ones(1, f32))], np.ones((1, 2), f32), "relu", "none")[0, 0] == 1.0
    # ... and it is a float32 add of its own, not fused into the last multiply-add: 2^24 + 1 rounds to 2^24 first
    assert pb.forward_bits([(np.array([[big, 1]], f32), np.full(1, -big, f32))], np.ones((1, 2), f32), "relu", "none")[0, 0] == 0.0
    # fused: (1 + 2^-23)(1 - 2^-23) - 1 = -2^-46, which a rounded product loses
    x = np.array([[1, 1 + 2.0 ** -23]], f32)
    w = np.array([[-1, 1 - 2.0 ** -23]], f32)
    assert pb.forward_bits([(w, zero)], x, "relu", "none")[0, 0] == f32(-2.0 ** -46)
    # two layers by hand: ReLU zeroes the negative unit, the clip saturates at its bounds exactly
    layers = [(np.array([[0.5, 0.25], [1.0, 1.0]], f32), np.array([0.0, 0.5], f32)), (np.array([[2.0, -4.0]], f32), np.array([0.25], f32))]
    xs = np.array([[1.0, -2.0], [4.0, 2.0]], f32)  # hidden (0, -0.5) -> (0, 0); (2.5, 6.5) -> 5 - 26 + 0.25
    assert np.array_equal(pb.forward_bits(layers, xs, "relu", "none"), np.array([[0.25], [-20.75]], f32))
    assert np.array_equal(pb.forward_bits(layers, xs, "relu", "clip", -0.3, 0.2), np.array([[0.2], [-0.3]], f32))
    assert pb.forward_bits(layers, xs, "relu", "clip", -0.3, 0.2)[1, 0] == f32(-0.3) and float(f32(-0.3)) != -0.3  # the bounds are float32


def test_relu_and_clip_pass_nan_and_negative_zero_as_the_kernel_does():
    eye = np.eye(2, dtype=f32)
    x = np.array([[np.nan, 1.0], [-1.0, 2.0]], f32)
    y = pb.forward_bits([(eye, np.zeros(2, f32)), (eye, np.zeros(2, f32))], x, "relu", "clip", -0.5, 0.5)
    assert np.isnan(y[0]).all()  # fma(1, 0, NaN) is NaN: a NaN spreads through its own row ...
    assert np.array_equal(y[1], np.array([0.0, 0.5], f32))  # ... and stays out of the next
    # y < 0 ? 0 : y keeps -0.0 (np.maximum(-0.0, 0.0) may not)
    y = pb.forward_bits([(np.ones((1, 1), f32), np.array([-0.0], f32)), (np.ones((1, 1), f32), np.array([-0.0], f32))],
                        np.array([[-0.0]], f32), "relu", "none")
    assert pb.same_bits(y, np.array([[0.0]], f32))  # fma(-0, 1, +0) = +0; +0 + -0 = +0


def test_the_model_refuses_what_it_cannot_state_exactly():
    rng = np.random.default_rng(6)
    x = np.ones((2, 5), f32)
    with pytest.raises(ValueError, match="tanhf"):
        pb.forward_bits(pm.random_layers(rng, (5, 4, 2)), x, "tanh", "none")
    with pytest.raises(ValueError, match="tanhf"):
        pb.forward_bits(pm.random_layers(rng, (5, 4, 2)), x, "relu", "tanh")
    with pytest.raises(ValueError, match="tanhf"):
        pb.forward_bits(pm.random_layers(rng, (5, 2)), x, "tanh", "tanh")
    with pytest.raises(ValueError):
        pb.forward_bits(pm.random_layers(rng, (5, 2)), x, "gelu", "none")
    assert pb.forward_bits(pm.random_layers(rng, (5, 2)), x, "tanh", "clip").shape == (2, 2)  # one layer: no hidden activation


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------
def test_case_table_has_the_shapes_the_kernel_branches_on_and_leaves_the_old_table_alone():
    assert len(pm.NETWORKS) == 9 and not set(pb.CASES) & set(pm.NETWORKS)
    assert {pb.CASES[f"in-{D}"]["sizes"] for D in pb.INPUT_WIDTHS} == {(D, 65, 3) for D in pb.INPUT_WIDTHS}
    groups = {-(-w // 64) for w in pb.WIDTHS}
    assert groups == set(range(1, 9)) and all(w in pb.WIDTHS for w in (128, 192, 256, 320, 384, 448, 512))
    for name, c in pb.CASES.items():
        if name in pb.BIT_CASES or name in pb.PAIRS or name == "hostile-relu":
            assert c["output"] != "tanh" and (c["activation"] == "relu" or len(c["sizes"]) == 2), name
        assert pb.seed(name) != pb.seed(name, 1)
    assert len({pb.seed(n) for n in pb.CASES}) == len(pb.CASES)
    for name in ("in-5", "pair-130-5+130-5"):
        x = pb.inputs(name, 17)
        assert x.dtype == f32 and not x.flags.writeable and (x[5] == 0).all() and (np.abs(x[6]) == 10).all() and np.abs(x).max() <= 10
        assert pb.inputs(name, 1).shape == (1, x.shape[1])


@pytest.mark.parametrize("name", [n for n in pb.CASES if n.startswith("last-") and n.endswith("-clip")])
def test_the_clipped_last_layers_saturate_in_part(name):
    """What the GPU test relies on: at E = 17 some outputs of every clipped case sit on a bound and some do not."""
    c = pb.CASES[name]
    y = pb.model(name, 17)[0]
    lo, hi = f32(c["low"]), f32(c["high"])
    assert (lo, hi) != (-1, 1) and y.min() >= lo and y.max() <= hi
    assert ((y == lo) | (y == hi)).any() and ((y > lo) & (y < hi)).any()
