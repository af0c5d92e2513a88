"""The policy forward of include/fleet_hip.h in the header's own words, bit for bit, in NumPy: every output element is one chain
`acc = 0; acc = fmaf(x[k], W[j][k], acc)` for k = 0 .. in-1; `y = acc + b[j]`, float32 throughout.  `fma32` is a correctly rounded
float32 fused multiply-add on arrays; `forward_bits` is the chain.  It models what is exact and nothing else: ReLU networks and
one-layer heads with output `none` or `clip`; a network that would need `tanhf` is refused.  Then the networks and inputs of
tests/test_policy_bits_gpu.py, a table of its own beside `policy_model.NETWORKS` (whose seeds come from the position of a name in
the sorted table, so that one never grows).  Shared with tests/test_policy_bits_cpu.py; nothing here needs a GPU or the library."""
import functools
import zlib

import numpy as np

import policy_model as pm

F32_TINY = np.float32(np.finfo(np.float32).tiny)  # the smallest normal float32


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def fma32(x, w, acc) -> np.ndarray:
    """round32(x * w + acc), rounded once, for float32 arrays (broadcast against each other).

    The product of two 24-bit significands is exact in float64.  The float64 sum s = p + acc and its TwoSum error e are exact
    together (p + acc = s + e).  Rounding s to float32 directly would round twice; instead s is first made the round-to-odd
    float64 of the exact sum -- where e != 0 and s's last significand bit is even, s moves to its neighbour on e's side -- and a
    round-to-odd value with 53 >= 24 + 2 bits rounds to the same float32 as the exact sum does.
    Infinities and NaNs go through as IEEE has them.  Subnormal results and overflow from finite operands are not modelled:
    AssertionError."""
    x, w, acc = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(w, np.float32), np.asarray(acc, np.float32))
    a = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = x.astype(np.float64) * w.astype(np.float64)
        s = np.asarray(p + a)
        bb = s - p
        e = (p - (s - bb)) + (a - bb)
        move = np.isfinite(s) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(move, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        r = s.astype(np.float32)
    mag = np.abs(r)
    finite_in = np.isfinite(p) & np.isfinite(a)
    assert (np.isfinite(r) | ~finite_in).all(), "fma32: a finite chain overflowed float32"
    assert ((mag >= F32_TINY) | (r == 0) | ~finite_in).all(), "fma32: a subnormal float32 result"
    return r


def forward_bits(layers, x, activation, output, low=-1.0, high=1.0) -> np.ndarray:
    """The header's chain.  layers: [(W float32 [out, in], b float32 [out]), ...]; x float32 [E, in].  Per layer acc = 0, one fma32
    per k in ascending order over the declared `in` (the device's padding contributes fma(0, 0, acc) = acc), one float32 add of the
    bias; the hidden ReLU and the clip as the kernel writes them, so a NaN and -0.0 pass through a ReLU and a NaN through a clip."""
    if activation not in ("relu", "tanh") or output not in ("none", "clip", "tanh"):
        raise ValueError(f"unknown activation {activation!r} or output {output!r}")
    if output == "tanh":
        raise ValueError("forward_bits does not model tanhf: output 'tanh' has no bit-exact model")
    if activation == "tanh" and len(layers) > 1:
        raise ValueError("forward_bits does not model tanhf: a tanh network with a hidden layer has no bit-exact model")
    y = np.asarray(x, dtype=np.float32)
    assert y.ndim == 2
    for i, (w, b) in enumerate(layers):
        w, b = np.asarray(w, dtype=np.float32), np.asarray(b, dtype=np.float32)
        assert w.shape == (b.shape[0], y.shape[1])
        wt = np.ascontiguousarray(w.T)  # [in, out]
        acc = np.zeros((y.shape[0], w.shape[0]), np.float32)
        for k in range(w.shape[1]):
            acc = fma32(y[:, k:k + 1], wt[k], acc)
        with np.errstate(invalid="ignore"):
            y = acc + b
            assert (np.isfinite(y) | ~np.isfinite(acc)).all()
            if i < len(layers) - 1:
                y = np.where(y < 0, np.float32(0), y)
    if output == "clip":
        lo, hi = np.float32(low), np.float32(high)
        with np.errstate(invalid="ignore"):
            y = np.where(y < lo, lo, np.where(y > hi, hi, y))
    assert y.dtype == np.float32
    return y


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def same_bits_or_both_nan(a, b) -> bool:
    """Bit equality, except that a NaN equals a NaN of any payload."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | both).all())


# ---- the cases of tests/test_policy_bits_gpu.py -------------------------------------------------------------------------------------
BATCHES = (1, 17)  # one row; one full tile of 16 and one ragged row
WIDTHS = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 512)  # both sides of every column-group edge
INPUT_WIDTHS = (1, 3, 4, 5, 127, 128, 129, 131, 132, 255, 256, 257, 1438, 8191, 8192)  # the pad to 4, the 128-column chunk, the maximum
CLIP = (-0.3, 0.7)  # bounds that are not +-1


def _case(sizes, activation="relu", output="none", low=-1.0, high=1.0, critic=None, last_scale=1.0):
    """last_scale: the actor's last weights times this, so that some outputs reach a clip."""
    return {"sizes": tuple(sizes), "activation": activation, "output": output, "low": low, "high": high,
            "critic": None if critic is None else tuple(critic), "last_scale": last_scale}


def _cases() -> dict:
    c = {}
    for D in INPUT_WIDTHS:  # 1. the input width
        c[f"in-{D}"] = _case((D, 65, 3))
    for w in WIDTHS:  # 2. every width as the first layer, as a middle layer fed from the LDS, as the last layer
        c[f"first-{w}"] = _case((20, w, 3))
        c[f"middle-{w}"] = _case((20, 33, w, 3))
        c[f"last-{w}"] = _case((20, 70, w))
        c[f"last-{w}-clip"] = _case((20, 70, w), output="clip", low=CLIP[0], high=CLIP[1], last_scale=4.0)
    # 3. the LDS row stride set by a late layer after narrower ones, and heads of one layer (no hidden activation: tanh qualifies)
    c["stride-20-33-512-70-4"] = _case((20, 33, 512, 70, 4))
    c["stride-20-1-512-1-2"] = _case((20, 1, 512, 1, 2))
    c["one-17-5"] = _case((17, 5), activation="tanh", output="clip", low=CLIP[0], high=CLIP[1])
    c["one-129-130"] = _case((129, 130), activation="tanh")
    c["one-8192-512"] = _case((8192, 512), activation="tanh", output="clip", low=CLIP[0], high=CLIP[1])
    # 4. two heads that differ in width, depth and output width (the actor's output transform varies, the critic's is none)
    c["pair-64-64-50+400-300-1"] = _case((389, 64, 64, 50), output="clip", critic=(389, 400, 300, 1))
    c["pair-512-512-3+1"] = _case((389, 512, 512, 3), critic=(389, 1))
    c["pair-5+33-130-70-3"] = _case((389, 5), output="clip", low=CLIP[0], high=CLIP[1], critic=(389, 33, 130, 70, 3))
    c["pair-130-5+130-5"] = _case((389, 130, 5), critic=(389, 130, 5))
    # 7. the network of the hostile rows
    c["hostile-relu"] = _case((45, 65, 65, 3))
    c["hostile-tanh"] = _case((45, 65, 65, 3), activation="tanh", output="clip")
    # 8. tanh networks at the new shapes: no bit model, the float64 model and the project's bound
    for sizes in ((129, 193, 321, 3), (257, 256, 384, 130)):
        for output in ("tanh", "clip"):
            c["tanh-" + "-".join(map(str, sizes)) + "-" + output] = _case(sizes, activation="tanh", output=output)
    return c


CASES = _cases()
PAIRS = tuple(n for n in CASES if n.startswith("pair-"))
TANH_CASES = tuple(n for n in CASES if n.startswith("tanh-"))
BIT_CASES = tuple(n for n in CASES if not n.startswith(("pair-", "tanh-", "hostile-")))  # one head, bit model


def seed(name, salt=0) -> int:
    """From the name alone: adding a case changes no other case."""
    return zlib.crc32(f"{name}/{salt}".encode())


@functools.lru_cache(maxsize=None)
def network(name, salt=0):
    """(actor layers, critic layers or None); `salt` gives other weights of the same shapes."""
    c = CASES[name]
    rng = np.random.default_rng(seed(name, salt))
    actor = pm.random_layers(rng, c["sizes"])
    actor[-1] = ((actor[-1][0] * np.float32(c["last_scale"])).astype(np.float32), actor[-1][1])
    return actor, (pm.random_layers(rng, c["critic"]) if c["critic"] else None)


@functools.lru_cache(maxsize=None)
def inputs(name, E) -> np.ndarray:
    """As policy_model.inputs: standard normal x 3 clipped to +-10; from 7 rows on, row 5 is all zero and row 6 all +-10."""
    D = CASES[name]["sizes"][0]
    rng = np.random.default_rng(seed(name, 1000 + E))
    x = np.clip(rng.standard_normal((E, D)) * 3, -10, 10).astype(np.float32)
    if E >= 7:
        x[5] = 0.0
        x[6] = np.where(rng.random(D) < 0.5, -10.0, 10.0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def model(name, E, salt=0) -> tuple:
    """The bit model's outputs per head (the critic's output transform is `none`), computed once per case."""
    c = CASES[name]
    actor, critic = network(name, salt)
    x = inputs(name, E)
    out = [forward_bits(actor, x, c["activation"], c["output"], c["low"], c["high"])]
    if critic:
        out.append(forward_bits(critic, x, c["activation"], "none"))
    for y in out:
        y.setflags(write=False)
    return tuple(out)
