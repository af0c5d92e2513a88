"""NumPy restatement of include/fleet_hip.h "PPO's whole update on the device" (fleet_train_*, fleetrl_amd/csrc/fleet_train.hip): the
keyed shuffle `perm`, the advantage normalisation's sums and roundings, the statistics block's float64 means, `explained_variance` and
the mean standard deviation.  Every function follows the header's lines; the GPU tests compare the device with them bit for bit."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
F32, F64 = np.float32, np.float64
ROUNDS, MIN_HALF_BITS, LANES = 8, 4, 256  # the header's constants (fleet_train.h: kTrainRounds, kTrainMinHalfBits, kTrainThreads)
STATS = ("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss", "n_updates", "explained_variance", "std")
STATS_LEN = 16
GRAD_STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")  # fleet_ppo_grad_dev's stats[0..5]


def philox_word0(c0, c1, c2, c3, k0, k1):
    """Word 0 of philox4x32_10 over broadcastable arrays of counter and key words."""
    u = np.uint64
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=u) & u(M32) for x in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    m, s = u(M32), u(32)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2  # 32 x 32 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & m, (p0 >> s) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + u(0x9E3779B9)) & m, (k1 + u(0xBB67AE85)) & m
    return c0


def half_bits(n: int, min_half_bits: int = MIN_HALF_BITS) -> int:
    """h: the smallest h >= min_half_bits with 2^(2h) >= n."""
    h = min_half_bits
    while (1 << (2 * h)) < n:
        h += 1
    return h


def perm(n: int, seed, epoch, p, rounds: int = ROUNDS, min_half_bits: int = MIN_HALF_BITS, walks=None):
    """perm(n, seed, epoch, p) for broadcastable arrays of seeds, epochs and positions p in [0, n): the header's balanced Feistel
    network over 2h bits with cycle walking.  walks: a one-element list that receives the longest walk."""
    u = np.uint64
    n = int(n)
    h = u(half_bits(n, min_half_bits))
    mask = (u(1) << h) - u(1)
    seed, epoch, p = np.broadcast_arrays(np.asarray(seed, dtype=u), np.asarray(epoch, dtype=u), np.asarray(p, dtype=u))
    assert (p < u(n)).all()
    k0, k1, e0, e1 = seed & u(M32), seed >> u(32), epoch & u(M32), epoch >> u(32)
    x = p.copy()
    todo = np.ones(x.shape, dtype=bool)
    steps = 0
    while todo.any():
        xs = x[todo]
        L, R = xs >> h, xs & mask
        for r in range(rounds):
            L, R = R, L ^ (philox_word0(R, u(r), e0[todo], e1[todo], k0[todo], k1[todo]) & mask)
        x[todo] = (L << h) | R
        todo = x >= u(n)
        steps += 1
    if walks is not None:
        walks[:] = [steps]
    return x.astype(np.int64)


def indices(n, seed, epoch, start=0, count=None):
    """What fleet_train_indices_dev writes: perm(n, seed, epoch, start .. start + count - 1) as int32."""
    count = n - start if count is None else count
    return perm(n, seed, epoch, np.arange(start, start + count)).astype(np.int32)


def tree_sum(x) -> F64:
    """The header's ordered float64 sum of the values x[0 .. B-1]: lane t of 256 adds x[t], x[t + 256], ... in ascending order to 0.0;
    then for s = 128, 64, ..., 1: lane t < s adds lane t + s's sum to its own; the result is lane 0's."""
    x = np.asarray(x, dtype=F64).reshape(-1)
    lanes = np.zeros(LANES, F64)
    for b0 in range(0, x.size, LANES):
        piece = x[b0:b0 + LANES]
        lanes[:piece.size] = lanes[:piece.size] + piece
    s = LANES // 2
    while s >= 1:
        lanes[:s] = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return lanes[0]


def normalise_stats(adv):
    """(mean32, std32) of a minibatch's advantages f32[B], B >= 2: float64 sums in tree_sum's order, each rounded once."""
    a = np.asarray(adv, dtype=F32).astype(F64)
    B = a.size
    mean = tree_sum(a) / F64(B)
    d = a - mean
    std = np.sqrt(tree_sum(d * d) / F64(B - 1))
    return F32(mean), F32(std)


def normalise(adv, on: bool = True):
    """The advantages the gradient launches read: (adv - mean32) / (std32 + 1e-8f) in float32; the raw ones for B == 1 or `on` off."""
    a = np.asarray(adv, dtype=F32)
    if not on or a.size < 2:
        return a.copy()
    mean, std = normalise_stats(a)
    return ((a - mean) / F32(std + F32(1e-8))).astype(F32)


def minibatches(n: int, batch_size: int):
    """(start, B) of one epoch's minibatches, the short last one included; one minibatch of n rows when batch_size >= n."""
    bs = min(int(batch_size), n)
    return [(s, min(bs, n - s)) for s in range(0, n, bs)]


def explained_variance(returns, values) -> F64:
    """1 - var(returns - values) / var(returns) over the whole buffer in time-major order (x[t * E + e]), float64, tree_sum's order:
    my = sum(y) / n, vy = sum((y - my)^2) / n, d = y - v, md = sum(d) / n, vd = sum((d - md)^2) / n; NaN when vy == 0."""
    y = np.asarray(returns, dtype=F32).reshape(-1).astype(F64)
    v = np.asarray(values, dtype=F32).reshape(-1).astype(F64)
    n = F64(y.size)
    d = y - v
    my, md = tree_sum(y) / n, tree_sum(d) / n
    vy, vd = tree_sum((y - my) * (y - my)) / n, tree_sum((d - md) * (d - md)) / n
    with np.errstate(divide="ignore", invalid="ignore"):
        return F64(np.nan) if vy == 0 else F64(1.0) - vd / vy


def mean_std(log_std) -> F64:
    """mean(exp(log_std)): tree_sum of (double)expf(log_std[j]) / A.  expf is the device's: callers that want bits pass its values."""
    e = np.exp(np.asarray(log_std, dtype=F32)).astype(F32)
    return tree_sum(e.astype(F64)) / F64(e.size)


def stats_block(grad_stats, ev, std) -> np.ndarray:
    """The statistics block f64[16] from the minibatches' fleet_ppo_grad_dev stats f32[8] in the order they ran: [0..4] the float64
    means (acc = 0.0; acc += (double)stat per minibatch in order; acc / count) of policy_loss, value_loss, entropy_loss, approx_kl,
    clip_fraction; [5] the last minibatch's loss; [6] the count; [7] explained_variance; [8] the mean std; [9..15] 0."""
    out = np.zeros(STATS_LEN, F64)
    acc = np.zeros(5, F64)
    src = [GRAD_STATS.index(k) for k in STATS[:5]]
    for s in grad_stats:
        s = np.asarray(s, dtype=F32)
        for k, i in enumerate(src):
            acc[k] = acc[k] + F64(s[i])
    m = F64(len(grad_stats))
    out[:5] = acc / m
    out[5] = F64(np.asarray(grad_stats[-1], dtype=F32)[GRAD_STATS.index("loss")])
    out[6], out[7], out[8] = m, ev, std
    return out


def chi_square_table(n: int, seeds, epoch: int, rounds: int = ROUNDS, min_half_bits: int = MIN_HALF_BITS):
    """(statistic, degrees of freedom) of the position-by-value count table of perm(n, seed, epoch, .) over `seeds`."""
    seeds = np.asarray(seeds, dtype=np.uint64)
    v = perm(n, seeds[:, None], epoch, np.arange(n)[None, :], rounds, min_half_bits)
    table = np.zeros((n, n), np.int64)
    for p in range(n):
        table[p] = np.bincount(v[:, p], minlength=n)
    want = seeds.size / n
    return float(((table - want) ** 2 / want).sum()), (n - 1) ** 2
