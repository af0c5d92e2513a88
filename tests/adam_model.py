"""The optimiser step of include/fleet_hip.h "Adam and clip_grad_norm_ on the device" in the header's own words, bit for bit, in
NumPy float32 (`fma32` is tests/policy_bits.py's correctly rounded fused multiply-add): the norm in its stated order, the clip, the
update.  Then the case table of tests/test_adam_gpu.py -- shapes, initial parameters, six steps of gradients -- with the conditions it
must meet, the model's run over it and torch's own clip_grad_norm_ + Adam on the CPU in float64 and float32.  Shared with
tests/test_adam_cpu.py; nothing here needs a GPU or the library.

The arithmetic.  The host forms in double, with t the step being taken (1 for the first), and rounds to float32:
    omb1 = 1 - beta1;  omb2 = 1 - beta2;  b2 = beta2;  nstep = -(lr / (1 - beta1^t));  bs = sqrt(1 - beta2^t);  eps
The norm: a chunk is 1024 consecutive elements of one gradient tensor (never of two).  Thread t of 256 takes elements 4t .. 4t + 3:
acc = 0; acc = fmaf(g, g, acc) ascending; an xor butterfly over each wavefront of 64 threads, offsets 32, 16, 8, 4, 2, 1; the four
wavefront sums added in wave order; the chunks' float32 partials added in float64 in ascending order; norm = (float)sqrt(sum).
The clip: q = maxn32 / (norm + 1e-6f); c = q > 1 ? 1 : q (a NaN stays); g' = g * c -- also when c == 1, not at all without clipping.
The update: m' = fmaf(g' - m, omb1, m); v' = fmaf(g' * omb2, g', v * b2); den = sqrtf(v') / bs + eps; p' = fmaf(m' / den, nstep, p).
"""
import functools
import math
import os
import zlib

import numpy as np

from policy_bits import fma32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CHUNK, THREADS, TILE = 1024, 256, 32  # what fleet_adam_describe must report for the table below to hold its edges
_LANE = np.arange(64)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def chunk_partials(g) -> np.ndarray:
    """float32 [ceil(n / 1024)]: the partial sums of squares of one tensor's chunks.  Elements past the end count as +0:
    fmaf(0, 0, acc) = acc for the acc >= +0 of a sum of squares, and NaN stays NaN, so this is the kernel's skip."""
    g = np.asarray(g, F32).ravel()
    n = -(-g.size // CHUNK)
    buf = np.zeros(n * CHUNK, F32)
    buf[:g.size] = g
    q = buf.reshape(n, THREADS, 4)
    acc = np.zeros((n, THREADS), F32)
    for e in range(4):
        acc = fma32(q[:, :, e], q[:, :, e], acc)
    w = acc.reshape(n, THREADS // 64, 64)
    with np.errstate(invalid="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            w = w + w[:, :, _LANE ^ off]
        ws = w[:, :, 0]
        out = ((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]
    assert out.dtype == F32
    return out


def grad_norm(grads) -> np.float32:
    s = 0.0
    for g in grads:
        for part in chunk_partials(g):
            s += float(part)  # float64, one by one in ascending chunk order
    return F32(math.sqrt(s)) if s == s else F32(np.nan)


def scalars(t: int, lr: float, betas, eps: float) -> dict:
    b1, b2 = float(betas[0]), float(betas[1])
    return {"omb1": F32(1.0 - b1), "omb2": F32(1.0 - b2), "b2": F32(b2), "nstep": F32(-(lr / (1.0 - b1 ** t))),
            "bs": F32(math.sqrt(1.0 - b2 ** t)), "eps": F32(eps)}


def clip_coef(norm, max_grad_norm) -> np.float32:
    with np.errstate(invalid="ignore"):
        q = F32(max_grad_norm) / (F32(norm) + F32(1e-6))
    return F32(1.0) if q > F32(1.0) else F32(q)


def step(params, grads, exp_avg, exp_avg_sq, t: int, *, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
    """Step t (>= 1) over lists of float32 arrays -> (params', exp_avg', exp_avg_sq', norm); the inputs are not changed.  The norm is
    always formed (what norm_out receives); it enters the update only with max_grad_norm > 0."""
    k = scalars(t, lr, betas, eps)
    norm = grad_norm(grads)
    clip = max_grad_norm is not None and max_grad_norm > 0
    c = clip_coef(norm, max_grad_norm) if clip else None
    P, M, V = [], [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
            p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
            if clip:
                g = g * c
            m1 = fma32(g - m, k["omb1"], m)
            v1 = fma32(g * k["omb2"], g, v * k["b2"])
            den = np.sqrt(v1) / k["bs"] + k["eps"]
            p1 = fma32(m1 / den, k["nstep"], p)
            assert m1.dtype == v1.dtype == den.dtype == p1.dtype == F32
            P.append(p1), M.append(m1), V.append(v1)
    return P, M, V, norm


# ---- the cases of tests/test_adam_gpu.py --------------------------------------------------------------------------------------------
SCALES = (3.0, 1e-3, 0.2, 40.0, 1e-2, 1.0)  # the gradients' scale per step
STEPS = len(SCALES)
MAX_GRAD_NORM = 0.5
NEAR = 1.04  # a step of scale s has the global norm s * NEAR * MAX_GRAD_NORM: scale 1 lies 4 % above the threshold
LR = 3e-4
BETAS = (0.9, 0.999)

# sizes: (in, width, ..., out) per net, as tests/policy_bits.py writes them.  kind "policy": actor, critic (or None), then log_std
# [A] as the extra; kind "td3": actor over D, critics over D + A.
CASES = {
    "one-layer-5x3": {"kind": "policy", "nets": ((5, 3), (5, 1)), "extras": (3,), "activation": "tanh", "output": "clip", "eps": 1e-5},
    "ragged-33": {"kind": "policy", "nets": ((33, 31, 25, 41, 3), (33, 32, 32, 1)), "extras": (3,), "activation": "tanh", "output": "clip",
                  "eps": 1e-5},
    "in-129": {"kind": "policy", "nets": ((129, 65, 3),), "extras": (3,), "activation": "relu", "output": "none", "eps": 1e-5},  # policy_bits' "in-129"
    "td3-5x3-two-critics": {"kind": "td3", "nets": ((5, 7, 3), (8, 9, 1), (8, 9, 1)), "extras": (), "activation": "relu", "output": "tanh",
                            "eps": 1e-8},
    "td3-6x2-deep-actor": {"kind": "td3", "nets": ((6, 33, 17, 5, 2), (8, 12, 1)), "extras": (), "activation": "relu", "output": "tanh",
                           "eps": 1e-8},
}
FLAT_LEN = 1025  # the optimiser without a net: one extra, one element past a chunk


def spans(name) -> tuple:
    """The optimisers a case is stepped with: (nets argument of DeviceAdam, first net, number of nets)."""
    c = CASES[name]
    if c["kind"] == "policy":
        return ((None, 0, len(c["nets"])),)
    return (("actor", 0, 1), ("critic", 1, len(c["nets"]) - 1))


def shapes(name, first=0, n=None, extras=True) -> list:
    """torch's shapes of the span's tensors (W [out, in], b [out] per layer, net after net), then the extras'."""
    c = CASES[name]
    nets = c["nets"][first:first + (len(c["nets"]) if n is None else n)]
    out = [s for sizes in nets for i, o in zip(sizes[:-1], sizes[1:]) for s in ((o, i), (o,))]
    return out + ([(e,) for e in c["extras"]] if extras else [])


def seed(name, salt) -> int:
    return zlib.crc32(f"adam/{name}/{salt}".encode())


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def initial(name) -> tuple:
    """The parameters of ALL nets of the case and its extras before the first step: uniform in +-1/sqrt(in) as torch's Linear, the
    extras zero as SB3's log_std."""
    rng = np.random.default_rng(seed(name, "init"))
    out = []
    for s in shapes(name, extras=False):
        bound = 1.0 / math.sqrt(s[1]) if len(s) == 2 else 0.5
        out.append(rng.uniform(-bound, bound, s).astype(F32))
    return _frozen(out + [np.zeros((e,), F32) for e in CASES[name]["extras"]])


def span_slice(name, first, n) -> slice:
    """Where the span's tensors (and, for a policy, the extras behind them) lie in `initial(name)`."""
    lo = len(shapes(name, 0, first, extras=False))
    hi = lo + len(shapes(name, first, n, extras=False))
    if CASES[name]["kind"] == "policy":
        hi += len(CASES[name]["extras"])
    return slice(lo, hi)


def scaled_gradients(shp, key, s) -> tuple:
    """Standard normal, scaled so that the global norm over the tensors is SCALES[s] * NEAR * MAX_GRAD_NORM (to float64 rounding)."""
    rng = np.random.default_rng(seed(key, f"grad{s}"))
    z = [rng.standard_normal(x) for x in shp]
    total = math.sqrt(sum(float((a * a).sum()) for a in z))
    return _frozen([(a * (SCALES[s] * NEAR * MAX_GRAD_NORM / total)).astype(F32) for a in z])


@functools.lru_cache(maxsize=None)
def gradients(name, first, n, s) -> tuple:
    return scaled_gradients(shapes(name, first, n, extras=CASES[name]["kind"] == "policy"), f"{name}/{first}/{n}", s)


@functools.lru_cache(maxsize=None)
def run(name, first, n, clip: bool) -> tuple:
    """The model's six steps from a zero state: per step (params, exp_avg, exp_avg_sq, norm)."""
    p = list(initial(name)[span_slice(name, first, n)])
    m, v = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    out = []
    for s in range(STEPS):
        p, m, v, norm = step(p, gradients(name, first, n, s), m, v, s + 1, lr=LR, betas=BETAS, eps=CASES[name]["eps"],
                             max_grad_norm=MAX_GRAD_NORM if clip else None)
        out.append((_frozen(p), _frozen(m), _frozen(v), norm))
    return tuple(out)


def facts_of(name) -> dict:
    """What the table promises, from the shapes and the model alone."""
    lens = [int(np.prod(s)) for c in CASES for s in shapes(c)]
    mats = [s for c in CASES for s in shapes(c) if len(s) == 2]
    facts = {
        "a tensor one below, at and one above the chunk": {CHUNK - 1, CHUNK, CHUNK + 1} <= set(lens) and
        {(31, 33), (32, 32), (41, 25)} <= set(mats),
        "a bias of one element": (1,) in [s for c in CASES for s in shapes(c)],
        "in and out off the multiples of 4, 32 and 64": {(3, 5), (65, 129)} <= set(mats),
        "a critic's first layer over D + A columns": any(c["kind"] == "td3" and c["nets"][1][0] == c["nets"][0][0] + c["nets"][0][-1]
                                                        for c in CASES.values()),
        "more than one tile in both directions": any(o > TILE and i > TILE for o, i in mats),
    }
    for _, first, n in spans(name):
        norms = [float(r[3]) for r in run(name, first, n, True)]
        facts[f"span {first}+{n}: a norm above the threshold"] = any(x > 1.1 * MAX_GRAD_NORM for x in norms)
        facts[f"span {first}+{n}: a norm below the threshold"] = any(x < 0.9 * MAX_GRAD_NORM for x in norms)
        facts[f"span {first}+{n}: a norm within 10 % of the threshold"] = any(abs(x - MAX_GRAD_NORM) <= 0.1 * MAX_GRAD_NORM for x in norms)
    return facts


# ---- torch's own clip + Adam on the CPU -----------------------------------------------------------------------------------------------
def torch_run(params, grads_per_step, dtype, *, lr=LR, betas=BETAS, eps=1e-8, max_grad_norm=None, state=None, lrs=None) -> list:
    """clip_grad_norm_(foreach=False) + Adam(foreach=False) on CPU copies in `dtype`, fed the float32 gradients: per step (params,
    exp_avg, exp_avg_sq, norm) as float64 arrays.  state: a torch.optim.Adam state dict to start from; lrs: the rate per step."""
    import torch

    ps = [torch.nn.Parameter(torch.tensor(np.asarray(p), dtype=dtype)) for p in params]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, foreach=False)
    if state is not None:
        opt.load_state_dict(state)
    out = []
    for s, grads in enumerate(grads_per_step):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[s]
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(np.asarray(g), dtype=dtype)
        if max_grad_norm is not None and max_grad_norm > 0:
            norm = torch.nn.utils.clip_grad_norm_(ps, max_grad_norm, foreach=False)
        else:
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ps]))
        opt.step()
        f64 = lambda t: t.detach().to(torch.float64).numpy().copy()  # noqa: E731
        out.append(([f64(p) for p in ps], [f64(opt.state[p]["exp_avg"]) for p in ps], [f64(opt.state[p]["exp_avg_sq"]) for p in ps],
                    float(norm)))
    return out


@functools.lru_cache(maxsize=None)
def torch_reference(name, first, n, clip: bool, double: bool) -> tuple:
    import torch

    grads = [gradients(name, first, n, s) for s in range(STEPS)]
    return tuple(torch_run(initial(name)[span_slice(name, first, n)], grads, torch.float64 if double else torch.float32,
                           eps=CASES[name]["eps"], max_grad_norm=MAX_GRAD_NORM if clip else None))


def bound_ratios(got, ref64, ref32) -> dict:
    """Per quantity the worst |got - ref64| / (8 max(eps_ref, 2^-24 max|ref64|)) over the tensors of one step; eps_ref is the
    distance of torch's float32 run from its float64 run on that tensor."""
    worst = {}
    for key, i in (("p", 0), ("exp_avg", 1), ("exp_avg_sq", 2)):
        r = 0.0
        for g, a, b in zip(got[i], ref64[i], ref32[i]):
            err = float(np.abs(np.asarray(g, np.float64) - a).max())
            lim = 8.0 * max(float(np.abs(b - a).max()), 2.0 ** -24 * float(np.abs(a).max()))
            r = max(r, err / lim if lim > 0 else (0.0 if err == 0 else np.inf))
        worst[key] = r
    lim = 8.0 * max(abs(ref32[3] - ref64[3]), 2.0 ** -24 * abs(ref64[3]))
    worst["norm"] = abs(float(got[3]) - ref64[3]) / lim
    return worst
