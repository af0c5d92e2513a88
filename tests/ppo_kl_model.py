"""The statistics of PPO's update with early stopping on approx_kl (include/fleet_hip.h, fleet_train_ppo_kl_dev), restated the way the
device counts them: one pass over the minibatches in the order they run, a running float64 sum per statistic that is cleared once per
call, the last epoch's approx_kl sum cleared whenever an epoch is entered, and counters that move when a minibatch is folded."""
import numpy as np

import train_model as tm

F32, F64 = np.float32, np.float64
ROOT = tm.ROOT
LOSS, KL = tm.GRAD_STATS.index("loss"), tm.GRAD_STATS.index("approx_kl")
KL_STATS = ("n_steps", "n_epochs", "early_stop", "last_approx_kl", "epoch_approx_kl")


def threshold(target_kl) -> F64:
    """1.5 * target_kl, formed once in double."""
    return F64(1.5) * F64(target_kl)


def stops(approx_kl, thr) -> bool:
    """The comparison of SB3 and of the device: the float32 statistic as float64 against the threshold; a NaN does not stop."""
    return bool(F64(F32(approx_kl)) > F64(thr))


def stats_block(rows, per_epoch: int, thr, ev=0.0, std=0.0):
    """rows: the gradient launches' stats f32[8] of the SCHEDULED minibatches in order (rows behind a stop are never looked at);
    per_epoch: minibatches per epoch; thr: the threshold.  Returns (stop, block): the index of the stopping minibatch or None, and the
    block f64[16] -- [0..4] means over the minibatches that ran, [5] the last one's loss, [6] how many ran, [7] ev, [8] std, [9] steps
    taken, [10] epochs entered, [11] stopped early, [12] the last approx_kl, [13] its mean over the last epoch entered, [14..15] 0."""
    src = [tm.GRAD_STATS.index(k) for k in tm.STATS[:5]]
    acc = np.zeros(5, F64)
    ran = steps = epochs = epoch_n = 0
    epoch_kl = F64(0.0)
    stop = None
    last = None
    for i, row in enumerate(rows):
        row = np.asarray(row, dtype=F32)
        for k, j in enumerate(src):
            acc[k] = acc[k] + F64(row[j])
        ran += 1
        if i % per_epoch == 0:
            epochs, epoch_n, epoch_kl = epochs + 1, 0, F64(0.0)
        epoch_n += 1
        epoch_kl = epoch_kl + F64(row[KL])
        last = row
        if stops(row[KL], thr):
            stop = i
            break
        steps += 1
    out = np.zeros(tm.STATS_LEN, F64)
    out[:5] = acc / F64(ran)
    out[5], out[6], out[7], out[8] = F64(last[LOSS]), F64(ran), ev, std
    out[9], out[10], out[11] = F64(steps), F64(epochs), F64(0.0 if stop is None else 1.0)
    out[12], out[13] = F64(last[KL]), epoch_kl / F64(epoch_n)
    return stop, out


def records(seq):
    """Indices at which the sequence sets a new running maximum (the first element is one); NaNs never do."""
    out, best = [], -np.inf
    for i, x in enumerate(seq):
        if x > best:
            out.append(i)
            best = x
    return out


def target_for(seq, index: int) -> float:
    """A target_kl under which a run with the approx_kl sequence `seq` stops exactly at the running-maximum record `index`:
    1.5 * target_kl lies halfway between seq[index] and the largest value before it (0 when there is none)."""
    seq = [float(x) for x in seq]
    assert index in records(seq)
    below = max(seq[:index], default=0.0)
    return (0.5 * (seq[index] + below)) / 1.5
