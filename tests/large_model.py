"""The pattern the tests of arrays past 2^32 elements are filled with, the shapes they use and the indices they check -- pure NumPy,
shared by tests/test_large_arrays_cpu.py (which proves the pattern honest) and tests/test_large_arrays_gpu.py.

`value(i) = float32((i mod M) * 2^-24)` for a 64-bit flat element index i, M = 2^24 - 3 (prime).  The values are exact in float32,
lie in [0, 1) and are never NaN.  An address computed in too few bits reads (or writes) element `i - m * 2^k`; the values at i and
there are equal only if M divides m * 2^k, and M is an odd prime larger than any m an array below 2^36 elements allows.  So a read
through a truncated address ALWAYS shows: `deltas(n)` lists every distance a truncation to 30 bits (a 32-bit byte offset of a
float), 31 or 32 bits can produce inside an array of n elements, and the CPU test asserts that none is a multiple of M."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = (1 << 24) - 3
SCALE = 2.0 ** -24
TRUNCATIONS = (30, 31, 32)  # bits an element index may be cut to: a 32-bit byte offset, an int, an unsigned
BOUNDARIES = tuple(1 << k for k in TRUNCATIONS)
N_RANDOM = 12

# what sets one array's pattern off from another's (value(i + offset)): small odd numbers, so a swap of two arrays shows
OFFSETS = {"obs": 0, "next_obs": 7919, "actions": 104729, "rewards": 1299709, "values": 15485863, "log_probs": 2750159,
           "advantages": 4256233, "returns": 6700417, "source": 9999991, "terminal": 12345701}

# ---- the shapes ---------------------------------------------------------------------------------------------------------------------
# Each is the smallest of its kind whose `obs` holds more than 2^32 floats with rows to spare behind the boundary, inside the create
# checks (rollout: E * K < 2^31 and a time row E * D far below 2^32; replay: R * E < 2^31; policy: D <= 8192).
#   rollout  64 * 8200 = 524800 rows of 8196 (16-byte path) or 8197 (scalar path) floats: 4.301e9 elements, 16.0 GiB.  2^32 falls
#            into time row 8188 of 8200; `add` needs that row, the one behind it and row K - 1 as three different rows, and eight more
#            keep the rows behind the boundary (767 of them) from being the array's last few.  A smaller D needs more rows, a larger
#            one a larger batch; K - 9 would be the least.
#   replay   520 * 8 = 4160 transitions of 1048580 / 1048581 floats: 4.362e9 elements, 16.25 GiB per observation array.  2^32 falls
#            into transition 4095 (ring row 511); ring rows 512 .. 519 lie wholly behind it, which a partial ring with pos = 516 and
#            an add at pos = 517 with untouched neighbours on both sides need.  The huge D takes sample_row's lane loop through 4096
#            (16-byte path) and 16385 (scalar path) iterations.
#   policy   524304 rows of D = 8192, the widest input the policy takes: 2^32 + 131072 elements, 16 rows behind the boundary -- one
#            tile of the forward kernel.
ROLLOUT = {"vec": dict(E=64, K=8200, D=8196, A=3), "scalar": dict(E=64, K=8200, D=8197, A=3)}
REPLAY = {"vec": dict(R=520, E=8, D=1048580, A=3), "scalar": dict(R=520, E=8, D=1048581, A=3)}
REPLAY_PARTIAL_POS = 516  # a partial ring whose write position lies behind 2^32
REPLAY_ADD_POS = 517
REPLAY_SEED = 2024
REPLAY_BATCH = 64
POLICY = dict(E=524304, D=8192, A=3)
POLICY_ROWS = (0, 262143, 262144, 262145, 524287, 524288, 524289, POLICY["E"] - 1)


# ---- the pattern --------------------------------------------------------------------------------------------------------------------
def value(i) -> np.ndarray:
    """float32((i mod M) * 2^-24), elementwise, for non-negative 64-bit indices."""
    i = np.asarray(i, dtype=np.uint64)
    return (i % np.uint64(M)).astype(np.float32) * np.float32(SCALE)


def span(start: int, n: int) -> np.ndarray:
    """value(start + arange(n)) for n <= M without 64-bit arithmetic per element: the residues of consecutive indices are
    consecutive, and wrap once at most."""
    assert 0 <= n <= M and start >= 0
    r = np.arange(n, dtype=np.int32) + np.int32(start % M)  # < 2 M < 2^31
    r[r >= M] -= M
    return r.astype(np.float32) * np.float32(SCALE)


def aliases(i: int, n: int) -> list:
    """The indices inside [0, n) that i becomes when it is cut to 30, 31 or 32 bits (those that differ from i)."""
    out = []
    for k in TRUNCATIONS:
        j = i & ((1 << k) - 1)
        if j != i and j < n and j not in out:
            out.append(j)
    return out


def deltas(n: int) -> list:
    """Every distance i - alias a truncation can produce for an index i < n: m * 2^k with m * 2^k <= n - 1."""
    return sorted({m << k for k in TRUNCATIONS for m in range(1, ((n - 1) >> k) + 1)})


# ---- the rows a test checks ---------------------------------------------------------------------------------------------------------
def rows_around(n_rows: int, width: int) -> list:
    """Rows (of `width` elements each) on both sides of the element offsets 2^30, 2^31 and 2^32: the row the offset falls into and the
    two rows before and behind it."""
    out = []
    for b in BOUNDARIES:
        r = b // width
        out += [x for x in range(r - 2, r + 3) if 0 <= x < n_rows]
    return out


def alias_rows(row: int, n_rows: int, width: int) -> list:
    """The rows that hold the aliases of row `row`'s first and last element: where a truncated address would read or write."""
    out = []
    for i in (row * width, row * width + width - 1):
        out += [j // width for j in aliases(i, n_rows * width)]
    return sorted(set(out))


def checked_rows(n_rows: int, width: int, seed: int) -> list:
    """Row 0, the last row, the rows around the three offsets, the alias rows of all of those (low rows that hold other values), and a
    dozen seeded random rows: about 40, in an order that is not sorted (a gather must not depend on one)."""
    rows = [0, n_rows - 1] + rows_around(n_rows, width)
    rows += [a for r in list(rows) for a in alias_rows(r, n_rows, width)]
    rows += [int(x) for x in np.random.default_rng(seed).integers(0, n_rows, N_RANDOM)]
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    order = np.random.default_rng(seed + 1).permutation(len(out))
    return [out[i] for i in order]


def rollout_rows(case: str) -> list:
    """Buffer rows r = t * E + e of the rollout gather."""
    s = ROLLOUT[case]
    return checked_rows(s["K"] * s["E"], s["D"], 11)


def rollout_add_rows(case: str) -> list:
    """The time rows `add` writes: those that straddle 2^31 and 2^32 elements of obs, and the last."""
    s = ROLLOUT[case]
    w = s["E"] * s["D"]
    return [(1 << 31) // w, (1 << 32) // w, s["K"] - 1]


def replay_rows(case: str, upper: int) -> list:
    """Transitions tr = row * E + env of the replay gather, over the first `upper` ring rows."""
    s = REPLAY[case]
    return checked_rows(upper * s["E"], s["D"], 13)


def replay_calls(case: str) -> dict:
    """The call counters at which `sample` is asked on the full and on the partial ring: the first whose 64 draws, by the model of the
    index draw, hold at least two transitions behind element 2^32 of the observation arrays."""
    import replay_model as rp

    s, out = REPLAY[case], {}
    for name, upper in (("full", s["R"]), ("partial", REPLAY_PARTIAL_POS)):
        for call in range(1000):
            rows, envs = rp.draw(REPLAY_SEED, call, REPLAY_BATCH, upper, s["E"])
            tr = rows.astype(np.int64) * s["E"] + envs
            if int((tr * s["D"] >= 1 << 32).sum()) >= 2:
                out[name] = call
                break
    return out


def policy_rows() -> list:
    """The rows of the issue and the rows their aliases fall into."""
    E, D = POLICY["E"], POLICY["D"]
    rows = list(POLICY_ROWS)
    for r in POLICY_ROWS:
        rows += [a for a in alias_rows(r, E, D) if a not in rows]
    return rows


def policy_weights():
    """A one-layer actor 8192 -> 3 beside a one-layer critic 8192 -> 1: (W, b) each, float32, seeded."""
    rng = np.random.default_rng(17)
    D, A = POLICY["D"], POLICY["A"]
    scale = 1.0 / np.sqrt(D)
    actor = ((rng.normal(0, scale, (A, D))).astype(np.float32), rng.normal(0, 0.1, A).astype(np.float32))
    critic = ((rng.normal(0, scale, (1, D))).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32))
    return actor, critic


# ---- the limits -------------------------------------------------------------------------------------------------------------------
def _constant(header, name):
    text = open(os.path.join(ROOT, "fleetrl_amd", "csrc", header)).read()
    m = re.search(rf"(?:constexpr int {name} =|#define {name}) (\d+)", text)
    assert m, (header, name)
    return int(m.group(1))


def limits() -> dict:
    """The largest sizes the buffers accept, as the kernels' launch shapes give them: a counter of 32 bits (unsigned in
    fleet_rollout.hip, int in fleet_replay.hip) that advances by `stride` finishes n items only if n <= 2^32 (2^31) - stride."""
    rollout_stride = _constant("fleet_rollout.h", "kRolloutMaxBlocks") * _constant("fleet_rollout.h", "kRolloutThreads")
    replay_stride = _constant("fleet_replay.h", "FLEET_REPLAY_MAX_BLOCKS") * (_constant("fleet_replay.h", "kReplayThreads") // 64)
    return {"rollout_items": (1 << 32) - rollout_stride, "replay_envs": (1 << 31) - replay_stride, "replay_dim": (1 << 31) - 64}
