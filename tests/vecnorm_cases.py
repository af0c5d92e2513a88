"""Fixed inputs of the normaliser's shape and hostile-input tests, from seeded NumPy generators: the CPU tests (the summation
scheme's restatement against the two-pass model) and the GPU tests (the device against the model) import the same bits."""
from __future__ import annotations

import numpy as np

# the ragged shape matrix: one-row and one-wave batches, a last slab of 1 / 63 / 64 rows, 2 / 5 / 66 (two rounds of the returns
# finalize, not a multiple of the four waves) / 257 slabs; one column, a masked tile, 64 +- 1 columns, the flagship's 388
RAGGED_E = (1, 2, 3, 4, 5, 63, 64, 65, 127, 300, 4161, 16447)
RAGGED_D = (1, 3, 63, 64, 65, 388)

HOSTILE_E = (5, 65, 4161, 65536)
HOSTILE_COLUMNS = ("constant", "far from zero, typical row 0", "far from zero, row 0 = 0", "N(1, 3), row 0 = 1e3",
                   "0.5 +- 1e-3, row 0 = 1e4", "all rows equal but the last", "1e-30 scale", "+-3e38 in two rows")
HOSTILE_D = len(HOSTILE_COLUMNS)
HOSTILE_CONSTANT = 1234.5678  # (as float32; any float32 constant sums exactly in float64)

_MEANS = (1.0, 1e4, -300.0, 0.0, 7.0)
_SDS = (3.0, 0.1, 50.0, 1.0, 0.0)


def ragged_batch(rng, E, D):
    """[E, D] float32: column c is N(mean, sd) of entry c % 5 above (typical, far from zero with a small spread, wide, standard,
    constant), so every tile -- the partial last one too -- holds each kind; rare spikes far past the clip in column 0."""
    c = np.arange(D) % 5
    x = rng.standard_normal((E, D)) * np.take(_SDS, c) + np.take(_MEANS, c)
    x[:, 0] = np.where(rng.random(E) < 0.02, 1e3, x[:, 0])
    return x.astype(np.float32)


def ragged_step(rng, E, D, p_done=0.2):
    """(obs, reward f64, done bool, terminal) of one step."""
    return ragged_batch(rng, E, D), rng.standard_normal(E) * 20 - 5, rng.random(E) < p_done, ragged_batch(rng, E, D)


def hostile_batch(E, k):
    """Batch `k` of the hostile sequence for E envs, [E, 8] float32, one column per entry of HOSTILE_COLUMNS."""
    rng = np.random.default_rng([2024, E, k])
    x = np.empty((E, HOSTILE_D), dtype=np.float64)
    x[:, 0] = HOSTILE_CONSTANT
    x[:, 1] = 1e4 + 0.1 * rng.standard_normal(E)
    x[:, 2] = 1e4 + 0.1 * rng.standard_normal(E)
    x[0, 2] = 0.0
    x[:, 3] = 1.0 + 3.0 * rng.standard_normal(E)
    x[0, 3] = 1e3
    x[:, 4] = 0.5 + 1e-3 * rng.uniform(-1, 1, E)
    x[0, 4] = 1e4
    x[:, 5] = 2.5
    x[-1, 5] = 3.5 + k
    x[:, 6] = 1e-30 * rng.standard_normal(E)
    x[:, 7] = 1.0 + 3.0 * rng.standard_normal(E)
    x[E // 2, 7] = 3e38
    x[E - 1, 7] = -3e38
    return x.astype(np.float32)


def hostile_rewards(E, k, scale=20.0, offset=-5.0):
    return np.random.default_rng([2025, E, k]).standard_normal(E) * scale + offset


def hostile_dones(E, k, p=0.2):
    return np.random.default_rng([2026, E, k]).random(E) < p


def hostile_start(model):
    """The constant column starts at its own mean with variance 0: any batch variance other than exactly 0.0 shows in the running
    variance at once."""
    model.obs_rms.mean[0] = float(np.float32(HOSTILE_CONSTANT))
    model.obs_rms.var[0] = 0.0
