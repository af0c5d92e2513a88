"""Correlated action noise on the device off the sequence lengths tests/test_noise_gpu.py runs: the paths of `pink_step`,
`fill_samples`, `ou_step` and `ou_reset` (fleet_noise.hip) that need more than one block of samples (n > 256), more than one chunk of
staged frequencies (n >= 512), a second trip of the copy loop (A > 256), every count of column pairs per trip, the wrap of q, and a
second trip of the OU grid-stride loops.  The pink tolerance is noise_model.pink_tol, from the model alone (tests/test_noise_cpu.py
recomputes it and shows that it sees one dropped frequency); OU keeps test_noise_gpu's OU_TOL.  Needs an MI355X."""
import numpy as np
import pytest

import noise_model as nm
from test_noise_gpu import OU_TOL, bits, on_device, pink, run, state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED_HIGH = (1 << 63) | 12345  # bit 63 set: the key's high word is not a small number
OFFSETS = (0, 5, 2 ** 31 - 70)


def rows64(t):
    return t.cpu().numpy().astype(np.float64)


def copy_state(s):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in s.items()}


# ---- 1. the sequences against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nm.NS_WIDE)
def test_pink_sequences_equal_the_model_at_wide_lengths(n):
    """n + 2 calls (both fill paths, the copy path, the wrap) against the model's float64 sum over the float32 tables, within
    pink_tol(n, beta).  What each length is the smallest case of -- G = ceil(n / 64) groups of samples in blocks of 4 per lane, K =
    n / 2 + 1 frequencies in chunks of 256:
      256   G = 4: the last length with one block            257   G = 4 + 1: a second block with one live lane
      320   G = 4 + 1: a full last group                     386   G = 4 + 3, even n: the Nyquist term
      510   K = 256: exactly one chunk                       511   odd n, exactly one chunk
      512   K = 257: the second chunk is the Nyquist term    513   G = 4 + 4 + 1, K = 257: the second chunk is one complex term
      1030  G = 4 x 4 + 1, chunks of 256 + 256 + 4           4096  the maximum: G = 64, K = 2049, 32 KB of twiddles in the LDS
    Every third case runs under a seed whose high word is set.  Largest |y_dev - y_model| measured on an MI355X per n, with the
    smallest pink_tol of its three betas:
      256   3.22e-6 (4.1e-5)     257   3.69e-6 (4.7e-5)     320   3.72e-6 (4.2e-5)     386   6.16e-6 (4.4e-5)     510   5.40e-6 (4.4e-5)
      511   5.37e-6 (4.4e-5)     512   5.45e-6 (4.8e-5)     513   5.37e-6 (5.0e-5)     1030  9.45e-6 (4.8e-5)     4096  1.69e-5 (5.7e-5)
    (at n = 4096 per beta 0, 1, 2: 1.05e-5, 1.58e-5, 1.69e-5 against 5.7e-5, 5.8e-5, 5.9e-5).  The device sits at the model's
    undisplaced chain error (1.74e-5 at n = 4096, beta = 2): its Box-Muller is well inside NOISE_BOUND, and what grows with n is
    the chain's rounding."""
    shapes = [(3, 5)] if n == 4096 else [(E, A) for E in (1, 3) for A in (1, 2, 5)]
    worst, case = {}, 0
    for beta in nm.BETAS:
        tol = nm.pink_tol(n, beta)
        for E, A in shapes:
            offset = OFFSETS[case % 3]
            seed = SEED_HIGH if (case + case // 3) % 3 == 2 else nm.SEED
            case += 1
            proc = pink(E, A, n, beta, seed=seed, offset=offset)
            got = rows64(run(proc, n + 2))
            model = nm.PinkModel(E, A, n, beta, seed=seed, env_id_offset=offset)
            want = np.stack([model.next() for _ in range(n + 2)])
            err = float(np.abs(got - want).max())
            worst[beta] = max(worst.get(beta, 0.0), err)
            t, q = state(proc)
            assert np.array_equal(t, model.t) and np.array_equal(q, model.q) and q.tolist() == [1] * E and t.tolist() == [2] * E
            assert err <= tol, (n, beta, E, A, hex(seed), offset, err, tol)
            assert proc.describe()["cache_bytes"] == E * n * A * 4
            proc.close()
    print(f"n={n}: max |y_dev - y_model| {max(worst.values()):.3g}; per beta " +
          ", ".join(f"{b:g}: {worst[b]:.3g} (pink_tol {nm.pink_tol(n, b):.2g})" for b in nm.BETAS))


@pytest.mark.parametrize("A,n", [(7, 257), (8, 257), (9, 257), (257, 257), (512, 512)])
def test_wide_action_rows(A, n):
    """Column pairs per trip of the four wavefronts, P = (A + 1) / 2: A = 7 and 8 give P = 4 (one trip, every wavefront holds a
    pair; A = 7's last pair has one column), A = 9 gives P = 5 (a second trip with one live wavefront), A = 257 is odd and above the
    256 threads of the copy loop (its second trip), A = 512 at n = 512 the maximum (64 pair trips, two chunks).  E = 2, beta = 1,
    n + 2 calls; in three of them one env is flagged and fills while the other copies, and in the last call env 1 wraps by itself
    while env 0 copies."""
    E, calls = 2, n + 2
    done = np.zeros((calls, E), np.uint8)
    done[1, 1] = done[3, 0] = done[n // 2, 0] = 1
    tol = nm.pink_tol(n, 1.0)
    proc, model = pink(E, A, n, seed=SEED_HIGH, offset=5), nm.PinkModel(E, A, n, seed=SEED_HIGH, env_id_offset=5)
    got = rows64(run(proc, calls, done))
    want = np.stack([model.next(done[c]) for c in range(calls)])
    err = float(np.abs(got - want).max())
    print(f"A={A} n={n}: max |y_dev - y_model| {err:.3g} (pink_tol {tol:.2g})")
    t, q = state(proc)
    assert np.array_equal(t, model.t) and np.array_equal(q, model.q) and q.tolist() == [2, 2] and t.tolist() == [n + 2 - n // 2, 1]
    assert err <= tol, (A, n, err, tol)
    proc.close()


# ---- 2. what needs no tolerance ----------------------------------------------------------------------------------------------------
def test_a_column_depends_on_its_pair_alone_bit_for_bit():
    """n = 513 (three blocks, two chunks), n + 2 calls, E = 3: columns [0, 50) of an A = 512 handle (64 pair trips, a copy loop of
    two trips) are an A = 50 handle's; column 4 of A = 5 (the odd column of a half-empty pair) is column 4 of A = 6."""
    n, E = 513, 3
    wide, narrow = bits(run(pink(E, 512, n), n + 2)), bits(run(pink(E, 50, n), n + 2))
    assert wide.shape == (n + 2, E, 512) and np.array_equal(wide[:, :, :50], narrow)
    five, six = bits(run(pink(E, 5, n), n + 2)), bits(run(pink(E, 6, n), n + 2))
    assert np.array_equal(five[:, :, 4], six[:, :, 4]) and np.array_equal(five, six[:, :, :5]) and np.array_equal(five, narrow[:, :, :5])
    assert not np.array_equal(six[:, :, 4], six[:, :, 5])


def test_the_row_emitted_from_registers_is_row_0_of_the_cache_bit_for_bit():
    """n = 513, A = 9 (a second pair trip): `next(done = 1)` emits sample 0 from the registers of the fill; a handle loaded with the
    state from before that call, t = 0 and q + 1, copies row 0 of its cache; `reset(mask)` then `next()` copies it too."""
    n, E, A = 513, 3, 9
    x, y, z = pink(E, A, n), pink(E, A, n), pink(E, A, n)
    run(x, 2), run(z, 2)
    before = copy_state(x.state_dict())
    ones = on_device(np.ones(E, np.uint8))
    from_registers = bits(x.next(ones))
    y.load_state_dict({**before, "t": torch.zeros_like(before["t"]), "q": before["q"] + 1})
    from_cache = bits(y.next())
    assert np.array_equal(from_registers, from_cache)
    z.reset(ones)
    assert np.array_equal(bits(z.next()), from_registers)
    for proc in (y, z):
        assert all(np.array_equal(a, b) for a, b in zip(state(proc), state(x)))
    assert state(x)[0].tolist() == [1] * E and state(x)[1].tolist() == [1] * E
    # ... and the rows that follow are the same sequence's
    assert np.array_equal(bits(run(y, 70)), bits(run(x, 70)))
    x.close(), y.close(), z.close()


def test_an_env_alone_equals_the_env_in_a_batch_at_three_chunks_bit_for_bit():
    """n = 1030 (five blocks, chunks of 256 + 256 + 4), A = 9, E = 5 against E = 1 with env_id_offset = g, the other envs
    regenerating at other times."""
    n, E, A = 1030, 5, 9
    calls = n + 2
    rng = np.random.default_rng(n)
    done = (rng.random((calls, E)) < 0.003).astype(np.uint8)
    done[2] = 1  # one call in which every env regenerates
    done[5, 1] = done[700, 3] = 1
    assert not any(np.array_equal(done[:, g], done[:, h]) for g in range(E) for h in range(g))  # no two envs share a history
    full = bits(run(pink(E, A, n), calls, done))
    for g in range(E):
        assert np.array_equal(bits(run(pink(1, A, n, offset=g), calls, done[:, g:g + 1])), full[:, g:g + 1]), g


def test_q_wraps_from_all_ones_to_zero():
    """n = 257, A = 5: a handle loaded with q = 0xFFFFFFFF (as int32 bits) and t = n takes sequence number 0 with its next call: the
    rows of that sequence are a fresh handle's."""
    n, E, A = 257, 3, 5
    proc, fresh = pink(E, A, n), pink(E, A, n)
    s = copy_state(proc.state_dict())
    proc.load_state_dict({**s, "t": torch.full_like(s["t"], n), "q": torch.full_like(s["q"], -1)})
    t, q = state(proc)
    assert t.tolist() == [n] * E and q.tolist() == [0xFFFFFFFF] * E
    first = bits(proc.next())
    t, q = state(proc)
    assert t.tolist() == [1] * E and q.tolist() == [0] * E
    want = bits(run(fresh, n))
    assert np.array_equal(first, want[0]) and np.array_equal(bits(run(proc, n - 1)), want[1:])
    # the sequence before the wrap is another one
    other = pink(E, A, n)
    other.load_state_dict({**s, "q": torch.full_like(s["q"], -1)})
    assert not np.array_equal(bits(other.next()), want[0])
    proc.close(), fresh.close(), other.close()


def test_a_loaded_state_continues_the_stream_across_blocks_and_chunks_bit_for_bit():
    """test_noise_gpu's pink checkpoint case at n = 513, A = 257: the refill after `load_state_dict` crosses three blocks and two
    chunks, the copy loop makes a second trip."""
    E, A, n, k = 3, 257, 513, 8
    rng = np.random.default_rng(2)
    done = (rng.random((k + n + 1, E)) < 0.004).astype(np.uint8)
    done[3, 1] = done[k + 100, 2] = 1
    first = pink(E, A, n)
    run(first, k, done[:k])
    saved = copy_state(first.state_dict())
    want = bits(run(first, n + 1, done[k:]))
    fresh = pink(E, A, n)
    run(fresh, 2)  # (a fresh handle that has moved: the loaded state replaces all of it)
    fresh.load_state_dict(saved)
    assert np.array_equal(bits(run(fresh, n + 1, done[k:])), want)
    assert all(np.array_equal(a, b) for a, b in zip(state(fresh), state(first)))
    first.close(), fresh.close()


# ---- 3. Ornstein-Uhlenbeck past one grid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,seed,offset", [(512, nm.SEED, 0), (511, SEED_HIGH, 2 ** 31 - 70)], ids=["A512", "A511-high-seed"])
def test_ou_grid_stride_loops_make_a_second_trip(A, seed, offset):
    """E = 8200: 8200 x 128 = 1 049 600 items of `ou_step` and 8200 x A of `ou_reset`, more than the 4096 blocks x 256 threads either
    launches, so both grid-stride loops make a second trip; at A = 511 the last block of every row has three columns.  Three calls
    with done flags against the model within OU_TOL (set for 50 calls), then `reset(mask)` zeroes exactly the masked rows."""
    from fleetrl_amd import DeviceOUNoise

    E, calls = 8200, 3
    assert E * ((A + 3) // 4) > 4096 * 256
    rng = np.random.default_rng(A)
    mu, sigma = rng.uniform(-0.2, 0.2, A), rng.uniform(0.2, 0.8, A)
    done = (rng.random((calls, E)) < 0.3).astype(np.uint8)
    proc = DeviceOUNoise(E, A, mu=mu, sigma=sigma, theta=1.5, dt=0.25, seed=seed, env_id_offset=offset)
    out = run(proc, calls, done)
    got = rows64(out)
    model = nm.OUModel(E, A, mu, sigma, 1.5, 0.25, seed=seed, env_id_offset=offset)
    want = np.stack([model.next(done[c]) for c in range(calls)])
    err = np.abs(got - want)
    print(f"OU E={E} A={A}: max |x_dev - x_model| after {calls} calls {err.max():.3g}; in the second trip {err[:, 8192:].max():.3g}")
    assert err.max() <= OU_TOL, (A, err.max(), np.unravel_index(err.argmax(), err.shape))
    s = proc.state_dict()
    assert s["calls"] == calls and np.array_equal(bits(s["x"]), bits(out[-1]))
    mask = (rng.random(E) < 0.5).astype(np.uint8)
    mask[[0, 8191, 8192, 8199]] = (1, 0, 1, 0)
    proc.reset(on_device(mask))
    x, last = bits(proc.state_dict()["x"]), bits(out[-1])
    assert not x[mask == 1].any() and np.array_equal(x[mask == 0], last[mask == 0]) and last[mask == 1].all()
    proc.reset()
    assert not bits(proc.state_dict()["x"]).any() and proc.state_dict()["calls"] == calls
    proc.close()


def test_ou_counter_carries_into_its_high_word():
    """E = 3, A = 5, calls loaded as 2^32 - 2: four calls draw under the counter words (lo, hi) = (2^32 - 2, 0), (2^32 - 1, 0), (0, 1),
    (1, 1), against the model with the same count within OU_TOL.  The last two calls are flagged done, so their rows are th mu +
    ss eps of their draws alone: they differ from the rows a fresh handle draws under (0, 0) and (1, 0), and so does the row between."""
    from fleetrl_amd import DeviceOUNoise

    E, A, start = 3, 5, 2 ** 32 - 2
    mu, sigma = np.linspace(-0.2, 0.2, A), np.linspace(0.2, 0.6, A)
    done = np.array([[0] * E, [0] * E, [1] * E, [1] * E], np.uint8)

    def make():
        return DeviceOUNoise(E, A, mu=mu, sigma=sigma, seed=nm.SEED, env_id_offset=3)

    proc, fresh = make(), make()
    s = copy_state(proc.state_dict())
    assert s["calls"] == 0
    proc.load_state_dict({**s, "calls": start})
    out = run(proc, 4, done)
    assert proc.state_dict()["calls"] == 2 ** 32 + 2
    model = nm.OUModel(E, A, mu, sigma, seed=nm.SEED, env_id_offset=3)
    model.calls = start
    want = np.stack([model.next(done[c]) for c in range(4)])
    err = float(np.abs(rows64(out) - want).max())
    print(f"OU calls = 2^32 - 2 ..: max |x_dev - x_model| {err:.3g}")
    assert err <= OU_TOL
    low = bits(run(fresh, 2, done[2:]))  # counter (0, 0) from x = 0, then (1, 0) flagged done: th mu + ss eps both
    high = bits(out)
    for r in (1, 2, 3):
        for c in (0, 1):
            assert not (high[r] == low[c]).any(), (r, c)
    proc.close(), fresh.close()
