"""The TD3 / DDPG learning target and the Polyak update of include/fleet_hip.h ("TD3 / DDPG learning targets on the device") in the
header's own words, bit for bit, in NumPy, on `policy_bits.forward_bits` and `policy_bits.fma32`; then the cases of
tests/test_qtarget_gpu.py.  `target_bits` takes a `variant` that gets ONE step wrong on purpose, for the known answers of
tests/test_qtarget_cpu.py.  Nothing here needs a GPU or the library."""
import functools
import zlib
from fractions import Fraction

import numpy as np

import policy_bits as pb
import policy_model as pm

f32 = np.float32
VARIANTS = ("max", "fma", "clip_after_sum", "action_first")


def clip32(x, lo, hi):
    """x < lo ? lo : (x > hi ? hi : x): a NaN passes through."""
    lo, hi = f32(lo), f32(hi)
    with np.errstate(invalid="ignore"):
        return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(np.float32)


def target_bits(actor, critics, next_obs, rewards, dones, eps, sigma, *, gamma, noise_clip, low=-1.0, high=1.0, activation="relu",
                output="clip", actor_low=-1.0, actor_high=1.0, variant=None) -> dict:
    """{"y" [B], "q" [B, n_critics], "next_actions" [B, A]}, float32, every step rounded as the header states it.
    variant (the mistakes the known answers tell apart): "max" takes the larger critic; "fma" fuses rewards + t * qmin;
    "clip_after_sum" clips d + n to +-noise_clip instead of n; "action_first" feeds the critics concat(a', next_obs)."""
    assert variant is None or variant in VARIANTS
    x = np.asarray(next_obs, dtype=np.float32)
    r, dn = np.asarray(rewards, dtype=np.float32).reshape(-1), np.asarray(dones, dtype=np.float32).reshape(-1)
    A = actor[-1][0].shape[0]
    d = pb.forward_bits(actor, x, activation, output, actor_low, actor_high)
    n = (np.broadcast_to(np.asarray(sigma, dtype=np.float32), (A,)) * np.asarray(eps, dtype=np.float32)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        if variant == "clip_after_sum":
            a = clip32(clip32(d + n, -noise_clip, noise_clip), low, high)
        else:
            a = clip32(d + clip32(n, -noise_clip, noise_clip), low, high)
        xa = np.concatenate([a, x] if variant == "action_first" else [x, a], axis=1)
        q = np.stack([pb.forward_bits(c, xa, activation, "none")[:, 0] for c in critics], axis=1)
        if len(critics) == 2:
            pick = q[:, 1] > q[:, 0] if variant == "max" else q[:, 1] < q[:, 0]
            qmin = np.where(pick, q[:, 1], q[:, 0])
        else:
            qmin = q[:, 0]
        t = ((f32(1.0) - dn) * f32(gamma)).astype(np.float32)
        y = pb.fma32(t, qmin, r) if variant == "fma" else (r + (t * qmin).astype(np.float32)).astype(np.float32)
    return {"y": y, "q": q.astype(np.float32), "next_actions": a}


# ---- the Polyak update ---------------------------------------------------------------------------------------------------------
def polyak_constants(tau: float):
    """(tau32, omt32) = ((float)tau, (float)(1.0 - tau))."""
    return f32(tau), f32(1.0 - float(tau))


def polyak_bits(target, param, tau: float) -> np.ndarray:
    """t' = fmaf(tau32, p, t * omt32): the product rounded to float32, then one fused multiply-add."""
    tau32, omt32 = polyak_constants(tau)
    t, p = np.asarray(target, dtype=np.float32), np.asarray(param, dtype=np.float32)
    return pb.fma32(tau32, p, (t * omt32).astype(np.float32))


def round_fraction32(v: Fraction) -> np.float32:
    """The float32 nearest to an exact rational, ties to even: the candidates around float(v) compared in exact arithmetic."""
    c = f32(float(v))
    cands = {float(c), float(np.nextafter(c, f32(-np.inf))), float(np.nextafter(c, f32(np.inf)))}
    best = min(cands, key=lambda u: (abs(Fraction(u) - v), int(np.array(u, np.float32).view(np.int32)) & 1))
    return f32(best)


def polyak_exact(t: float, p: float, tau: float) -> np.float32:
    """The same update on one element through exact rational arithmetic, rounded where the header rounds."""
    tau32, omt32 = polyak_constants(tau)
    m = round_fraction32(Fraction(float(t)) * Fraction(float(omt32)))
    return round_fraction32(Fraction(float(tau32)) * Fraction(float(p)) + Fraction(float(m)))


# ---- the cases of tests/test_qtarget_gpu.py -----------------------------------------------------------------------------------------
ROWS = 17  # every case has 17 rows; B = 1 and B = 16 take the first rows of them
BATCHES = (1, 16, 17)
ACTOR_CLIP = (-0.3, 0.7)  # the actor's output transform in the bit cases
ACTION_BOUNDS = (-0.5, 0.8)  # act_lo, act_hi
NOISE_CLIP, SIGMA, GAMMA = 0.5, 0.4, 0.99
PAIRS = ((5, 3), (126, 1), (127, 2), (128, 5), (129, 65), (250, 6), (388, 50), (7680, 512))  # (D, A): the seam against the chunk and the pad
# name -> (the actor's hidden widths, the critic's widths)
TRUNKS = {"c1": ((70,), (1,)), "c64-1": ((70,), (64, 1)), "c65-63-1": ((70,), (65, 63, 1)), "c400-300-1": ((70,), (400, 300, 1)),
          "deep-critic": ((), (33, 130, 70, 1)),  # a one-layer actor: the critic sets the stride S
          "deep-actor": ((33, 130, 70), (1,))}    # ... and the reverse


def _cases() -> dict:
    c = {}
    for D, A in PAIRS:
        for trunk in TRUNKS:
            if D == 7680 and trunk not in ("c1", "c400-300-1"):
                continue  # (the widest input: the seam at 7680 of 8192 columns is the point, not the trunk)
            c[f"{D}x{A}-{trunk}-2"] = (D, A, trunk, 2)
    for D, A in PAIRS[:-1]:
        c[f"{D}x{A}-c64-1-1"] = (D, A, "c64-1", 1)
    for trunk in TRUNKS:
        c[f"127x2-{trunk}-1"] = (127, 2, trunk, 1)
    return c


CASES = _cases()
# the cases the other GPU tests take their networks from (tests/test_qtarget_cpu.py holds every name to the table)
COMPOSE = (("relu", "clip", "250x6-c400-300-1-2"), ("tanh", "tanh", "388x50-c400-300-1-2"), ("tanh", "tanh", "129x65-c65-63-1-2"),
           ("tanh", "clip", "127x2-deep-critic-2"), ("relu", "tanh", "5x3-c64-1-1"), ("tanh", "tanh", "127x2-deep-actor-1"))
POLYAK_CASES = ("5x3-c65-63-1-2", "127x2-deep-critic-2", "129x65-c400-300-1-2", "126x1-c64-1-1", "127x2-deep-actor-1")
INVARIANCE_CASE, REFUSAL_CASE, HOSTILE_CASE, DESCRIBE_CASE = "129x65-c65-63-1-2", "127x2-c1-1", "127x2-c65-63-1-2", "5x3-c65-63-1-2"


def seed(name, salt=0) -> int:
    return zlib.crc32(f"qtarget/{name}/{salt}".encode())


@functools.lru_cache(maxsize=None)
def network(name, salt=0):
    """(actor layers, [critic layers, ...]) of a case; `salt` gives other weights of the same shapes (the online networks)."""
    D, A, trunk, nc = CASES[name]
    rng = np.random.default_rng(seed(name, salt))
    hidden, critic = TRUNKS[trunk]
    actor = pm.random_layers(rng, (D,) + hidden + (A,))
    actor[-1] = ((actor[-1][0] * f32(4.0)).astype(np.float32), actor[-1][1])  # so that some outputs reach the actor's clip
    critics = []
    for _ in range(nc):
        layers = pm.random_layers(rng, (D + A,) + critic)
        # the action columns weigh as much as the observation's, so that a wrong action shows in q
        w0 = layers[0][0].copy()
        w0[:, D:] *= f32(np.sqrt(max(D / A, 1.0)))
        layers[0] = (w0, layers[0][1])
        critics.append(layers)
    if nc == 2:
        # a narrow last layer leaves q near its bias and one critic below the other on every row: critic 1's last bias is moved
        # by the median of q_1 - q_0 over the case's rows (float64, a' = 0), so that each critic is the smaller one on some rows
        xa = np.concatenate([inputs(name)["next_obs"], np.zeros((ROWS, A), np.float32)], axis=1)
        diff = pm.forward64(critics[1], xa, "relu", "none")[:, 0] - pm.forward64(critics[0], xa, "relu", "none")[:, 0]
        w, b = critics[1][-1]
        critics[1][-1] = (w, (b - f32(np.median(diff))).astype(np.float32))
    return actor, critics


@functools.lru_cache(maxsize=None)
def inputs(name) -> dict:
    """next_obs, rewards, dones, eps of the case's 17 rows: dones alternate, row 5 of next_obs is zero."""
    D, A, _, _ = CASES[name]
    rng = np.random.default_rng(seed(name, 1000))
    x = np.clip(rng.standard_normal((ROWS, D)) * 3, -10, 10).astype(np.float32)
    x[5] = 0.0
    out = {"next_obs": x, "rewards": rng.standard_normal(ROWS).astype(np.float32), "dones": (np.arange(ROWS) % 2).astype(np.float32),
           "eps": rng.standard_normal((ROWS, A)).astype(np.float32)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(name) -> dict:
    """The bit model's outputs of the case's 17 rows, computed once (rows are independent: B rows are the first B of these)."""
    actor, critics = network(name)
    i = inputs(name)
    out = target_bits(actor, critics, i["next_obs"], i["rewards"], i["dones"], i["eps"], SIGMA, gamma=GAMMA, noise_clip=NOISE_CLIP,
                      low=ACTION_BOUNDS[0], high=ACTION_BOUNDS[1], activation="relu", output="clip", actor_low=ACTOR_CLIP[0],
                      actor_high=ACTOR_CLIP[1])
    for v in out.values():
        v.setflags(write=False)
    return out


def facts(name) -> dict:
    """What a case must exercise, across its rows: each critic wins the min somewhere, the noise saturates somewhere and not
    everywhere, the action saturates somewhere and not everywhere, dones holds both values."""
    D, A, _, nc = CASES[name]
    i, m = inputs(name), model(name)
    n = (f32(SIGMA) * i["eps"]).astype(np.float32)
    sat_n = np.abs(n) > f32(NOISE_CLIP)
    a = m["next_actions"]
    sat_a = (a == f32(ACTION_BOUNDS[0])) | (a == f32(ACTION_BOUNDS[1]))
    q = m["q"]
    return {"each_critic_wins": nc == 1 or bool((q[:, 1] < q[:, 0]).any() and (q[:, 0] < q[:, 1]).any()),
            "noise_saturates_and_not": bool(sat_n.any() and not sat_n.all()),
            "action_saturates_and_not": bool(sat_a.any() and not sat_a.all()),
            "dones_both": bool((i["dones"] == 0).any() and (i["dones"] == 1).any())}


def flat_params(actor, critics) -> list:
    """W, b per layer: the actor's, then each critic's -- the order of load_torch / polyak / export_torch."""
    return [a for net in [actor] + list(critics) for w, b in net for a in (w, b)]
