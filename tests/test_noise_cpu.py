"""Correlated action noise without a GPU: the C ABI's declarations and bindings, the host tables the library builds against the
model's, and the model of tests/noise_model.py against itself -- the direct sum against the irfft form of the colorednoise recipe,
its whiteness at beta = 0, its ensemble spectrum, and the counter domains."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import explore_model as em
import noise_model as nm
import policy_model as pm
import replay_model as rp

ROOT = pm.ROOT
ENTRIES = ("fleet_noise_pink_tables", "fleet_noise_create", "fleet_noise_destroy", "fleet_noise_last_error", "fleet_noise_set_stream",
           "fleet_noise_next_dev", "fleet_noise_reset_dev", "fleet_noise_get_state_dev", "fleet_noise_set_state_dev", "fleet_noise_describe")
FIELDS = ["struct_bytes", "kind", "num_envs", "act_dim", "env_id_offset", "seq_len", "seed", "beta", "theta", "dt", "mu", "sigma", "cache_bytes"]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_entries_equal_the_bound_symbols():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_noise_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.NOISE_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    section = hdr[hdr.index("correlated action noise on the device"):]
    assert hdr.index("int fleet_explore_act_dev(") < hdr.index("correlated action noise on the device")
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    for name, value in (("PINK", _capi.NOISE_PINK), ("OU", _capi.NOISE_OU), ("MAX_ACT_DIM", _capi.NOISE_MAX_ACT_DIM),
                        ("MAX_SEQ_LEN", _capi.NOISE_MAX_SEQ_LEN)):
        assert re.search(rf"^#define FLEET_NOISE_{name} {value}$", hdr, flags=re.M), name


def test_struct_size_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    cls = _capi.FleetNoiseParams
    assert [n for n, _ in cls._fields_] == FIELDS
    exprs = ["sizeof(FleetNoiseParams)"] + [f"offsetof(FleetNoiseParams, {n})" for n in FIELDS]
    want = [C.sizeof(cls)] + [getattr(cls, n).offset for n in FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_a_null_handle_and_bad_parameters_are_refused_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    out = C.c_float()
    assert lib.fleet_noise_next_dev(None, None, C.addressof(out)) == _capi.ERR_INVALID
    assert lib.fleet_noise_reset_dev(None, None) == _capi.ERR_INVALID
    assert lib.fleet_noise_set_stream(None, None) == _capi.ERR_INVALID
    assert lib.fleet_noise_get_state_dev(None, None, None, None, None) == _capi.ERR_INVALID
    assert lib.fleet_noise_set_state_dev(None, None, None, None, 0) == _capi.ERR_INVALID
    assert lib.fleet_noise_describe(None, None) == _capi.ERR_INVALID
    assert lib.fleet_noise_destroy(None) == _capi.OK
    # create validates before it touches a device: the reason names the entry
    p = _capi.FleetNoiseParams()
    p.struct_bytes, p.kind, p.num_envs, p.act_dim, p.seq_len, p.beta = C.sizeof(p), _capi.NOISE_PINK, 4, 3, 1, 1.0
    h = C.c_void_p()
    assert lib.fleet_noise_create(0, C.byref(p), C.byref(h)) == _capi.ERR_INVALID and not h
    why = lib.fleet_noise_last_error(None).decode()
    assert why.startswith("fleet_noise_create: ") and "seq_len" in why
    for n, beta in ((1, 1.0), (4097, 1.0), (8, -1.0), (8, float("nan")), (8, float("inf"))):
        with pytest.raises(_capi.FleetHipError) as ei:
            _capi.pink_tables(n, beta)
        assert ei.value.status == _capi.ERR_INVALID and "fleet_noise_pink_tables: " in str(ei.value)


# ---- the tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nm.NS + nm.NS_WIDE)
def test_the_librarys_host_tables_are_the_models_rounded_to_float32(n):
    from fleetrl_amd import _capi

    for beta in nm.BETAS + (0.5,):
        gain, twiddle = _capi.pink_tables(n, beta)
        g, tw = nm.tables32(n, beta)
        assert gain.shape == (n // 2 + 1,) and twiddle.shape == (n, 2)
        assert np.array_equal(gain, g), (n, beta)
        assert np.array_equal(twiddle, tw), (n, beta)


def test_table_known_answers():
    # n = 2, any beta: f = (0.5, 0.5), w = s_1 / 2, sigma = s_1 / 2: both gains sqrt(2) s / (2 s / 2) = sqrt(2)
    g, tw = nm.tables(2, 1.0)
    assert np.allclose(g, [np.sqrt(2.0), np.sqrt(2.0)]) and np.allclose(tw, [[1, 0], [-1, 0]])
    # beta = 0: s = 1, sum w^2 = (n - 1) / 2 (odd n) or n / 2 - 3 / 4 (even n: the last weight is halved), sigma^2 = 4 sum w^2 / n^2, and
    # sum gain^2 = 2 n / (n^2 sigma^2): Var = n / (n - 1) or n / (n - 3 / 2), above 1 by the DC term
    for n in (7, 64, 193):
        assert np.isclose(nm.variance(n, 0.0), n / (n - 1.0) if n % 2 else n / (n - 1.5), rtol=1e-13)
    assert nm.variance(192, 1.0) > 1.0


# ---- the model against itself ------------------------------------------------------------------------------------------------------
def test_the_models_array_generator_is_the_scalar_one():
    seed = nm.SEED
    w = nm.philox(np.array([0, 7, 2 ** 32 - 1])[:, None], (nm.PINK_TAG | np.arange(3))[None, :], 5, 96, seed)
    for i, e in enumerate((0, 7, 2 ** 32 - 1)):
        for p in range(3):
            assert tuple(int(v) for v in w[i, p]) == rp.philox4x32_10(nm.pink_counter(e, 2 * p + 1, 5, 96), em.key(seed))
    calls = 2 ** 32 + 3
    assert nm.ou_counter(9, 7, calls) == (9, nm.OU_TAG | 1, 3, 1)
    got = nm.philox(9, nm.OU_TAG | 1, 3, 1, seed)
    assert tuple(int(v) for v in got) == rp.philox4x32_10(nm.ou_counter(9, 7, calls), em.key(seed))
    # Box-Muller is explore_model's: the same words give the same normals
    assert np.array_equal(nm.normals4(em.words(seed, [3], 8, 11))[0].reshape(-1), em.normals(seed, [3], 8, 11)[0])


@pytest.mark.parametrize("n", nm.NS + nm.NS_WIDE)
def test_direct_sum_equals_the_irfft_form(n):
    for beta in nm.BETAS:
        a, b = nm.pink_coefficients(nm.SEED, np.arange(3), 5, [0, 1, 7], n)
        direct, fft = nm.direct_sum(a, b, n, beta), nm.irfft_form(a, b, n, beta)
        assert direct.shape == (3, 5, n)
        assert np.abs(direct - fft).max() <= 1e-12, (n, beta, np.abs(direct - fft).max())


# ---- the float32 chain and the tolerance of the wide lengths ----------------------------------------------------------------------
def test_the_wide_lengths_are_the_smallest_cases_of_their_paths():
    """(G, K) of every wide length: G = ceil(n / 64) groups of samples in blocks of 4, K = n / 2 + 1 frequencies in chunks of 256."""
    shape = {n: (-(-n // 64), n // 2 + 1) for n in nm.NS_WIDE}
    assert shape == {256: (4, 129), 257: (5, 129), 320: (5, 161), 386: (7, 194), 510: (8, 256), 511: (8, 256), 512: (8, 257),
                     513: (9, 257), 1030: (17, 516), 4096: (64, 2049)}
    assert max(-(-n // 64) for n in nm.NS) <= 4 and max(n // 2 + 1 for n in nm.NS) <= nm.CHUNK  # the old lengths: one block, one chunk
    assert nm.real_only(512)[256] and not nm.real_only(513)[256]  # the one term of the second chunk: the Nyquist term, a complex term


def test_the_float32_chain_is_the_direct_sum_up_to_its_roundings():
    """Known answers of `chain32` where every step is exact or a single rounding, and the chain against the float64 sum at an old
    length: undisplaced it stays within the 2K roundings, 2K x 2^-24 x the largest partial sum."""
    # n = 2: K = 2, both terms real, twiddles (1, 0), (-1, 0): y = (ga0 + ga1, ga0 - ga1), the products and one sum rounded once each
    f32 = np.float32
    a, b = np.array([[0.3, -1.7]]), np.array([[0.9, 0.4]])
    g = nm.tables32(2, 1.0)[0]
    ga = g * a[0].astype(f32)
    assert ga.dtype == f32
    want = np.array([[f32(ga[0] + ga[1]), f32(ga[0] - ga[1])]], dtype=np.float64)
    assert np.array_equal(nm.chain32(a, b, 2, 1.0), want)
    # the imaginary part of a real-only frequency is not read: NaN there leaves the sequence as it is
    for n in (7, 64):
        a, b = (c.reshape(15, -1) for c in nm.pink_coefficients(nm.SEED, np.arange(3), 5, 0, n))
        y = nm.chain32(a, b, n, 1.0)
        bad = np.where(nm.real_only(n), np.nan, b)
        assert np.array_equal(nm.chain32(a, bad, n, 1.0), y)
        ref = nm.direct_sum(a, b, n, 1.0, *nm.tables32(n, 1.0))
        K = n // 2 + 1
        assert np.abs(y - ref).max() <= 2 * K * 2.0 ** -24 * (np.abs(ref).max() + 1.0)
        # a displacement moves a sample by at most NOISE_BOUND x 2 sum gain, and does move it
        moved = nm.chain32(a, b, n, 1.0, displace=n)
        bound = 2 * nm.NOISE_BOUND * float(nm.tables32(n, 1.0)[0].sum()) + 4 * K * 2.0 ** -24 * (np.abs(ref).max() + 1.0)
        assert 0.0 < np.abs(moved - y).max() <= bound
        assert np.array_equal(moved, nm.chain32(a, b, n, 1.0, displace=n))  # seeded
    # the faults are faults: each changes the sequence, the first two by one frequency's term
    n = 513
    a, b = (c.reshape(48, -1) for c in nm.pink_coefficients(nm.SEED, np.arange(3), 16, 0, n))
    y = nm.chain32(a, b, n, 2.0)
    g = nm.tables32(n, 2.0)[0].astype(np.float64)
    for fault, k in (("drop_last", n // 2), ("drop_chunk_first", nm.CHUNK)):
        d = np.abs(nm.chain32(a, b, n, 2.0, fault=fault) - y).max(axis=1)
        amp = g[k] * np.hypot(a[:, k], b[:, k])
        assert np.all(d <= amp * (1 + 1e-3) + 1e-5) and np.all(d >= amp * 0.9 - 1e-5), fault  # (some t is within 26 degrees of the peak)
    assert np.abs(nm.chain32(a, b, n, 2.0, fault="phase_reset") - y).max() > 1e-4


@pytest.mark.parametrize("n", nm.NS_WIDE)
def test_the_wide_tolerance_table_is_twice_the_recomputed_chain_error(n):
    """pink_tol(n, beta) = 2 R(n, beta) rounded up to two digits, R recomputed here from the model alone; and the first condition:
    the tolerance is at most half the smallest gain, so one missing or misplaced frequency is larger than it."""
    R = nm.chain_errors(n)
    for beta in nm.BETAS:
        assert nm.pink_tol(n, beta) == nm.round_up2(2 * R[beta]), (n, beta, R[beta])
        assert 2 * R[beta] <= nm.pink_tol(n, beta) <= 2 * R[beta] * 1.1
        smallest = float(nm.tables32(n, beta)[0].min())
        assert nm.pink_tol(n, beta) <= smallest / 2, (n, beta, smallest)
    assert set(nm.PINK_TOL_WIDE) == {(m, b) for m in nm.NS_WIDE for b in nm.BETAS}
    assert nm.round_up2(2.5e-5) == 2.5e-5 and nm.round_up2(2.51e-5) == 2.6e-5 and nm.round_up2(9.91e-6) == 1.0e-5


@pytest.mark.parametrize("n", [512, 4096])
def test_the_wide_tolerance_sees_a_dropped_frequency_and_a_restarted_phase(n):
    """The second condition, at beta = 2 (the smallest gains): the last frequency dropped, the first frequency of the second chunk
    (k = 256) dropped, the phase walk restarted at k = 256 -- each, applied to the displaced chain, is off the float64 sum by more
    than pink_tol over the 48 columns.  At n = 512 the last frequency is the second chunk's only one, the Nyquist term."""
    tol = nm.pink_tol(n, 2.0)
    clean = nm.chain_errors(n, (2.0,))[2.0]
    assert clean <= tol / 2
    for fault in nm.FAULTS:
        err = nm.chain_errors(n, (2.0,), fault=fault)[2.0]
        assert err > tol, (n, fault, err, tol)


def test_a_sequence_depends_on_seed_env_column_and_sequence_number_alone():
    n, A = 7, 5
    full_a, full_b = nm.pink_coefficients(nm.SEED, np.arange(9), A, np.arange(9) % 3, n)
    a, b = nm.pink_coefficients(nm.SEED, [4], A, [1], n)
    assert np.array_equal(a[0], full_a[4]) and np.array_equal(b[0], full_b[4])
    a3, _ = nm.pink_coefficients(nm.SEED, [4], 3, [1], n)  # fewer columns: the same leading ones
    assert np.array_equal(a3[0], full_a[4, :3])
    for change in (dict(seed=nm.SEED + 1), dict(env=5), dict(q=2)):
        c = {**dict(seed=nm.SEED, env=4, q=1), **change}
        other, _ = nm.pink_coefficients(c["seed"], [c["env"]], A, [c["q"]], n)
        assert not np.any(other[0] == full_a[4]), change


def test_beta_zero_gives_mutually_uncorrelated_samples():
    for n in (7, 64, 193):
        for lag in range(1, n):
            assert abs(nm.correlation(n, 0.0, lag)) <= 1e-12, (n, lag)
    # ... and an ensemble of the model's sequences shows it: N = 50000 sequences of n = 8, every pair of samples within 5 / sqrt(N)
    N, n = 50000, 8
    a, b = nm.pink_coefficients(nm.SEED, np.arange(N // 50), 50, 0, n)
    y = nm.direct_sum(a, b, n, 0.0).reshape(N, n)
    c = np.corrcoef(y.T)
    assert np.abs(c - np.eye(n)).max() <= 5 / np.sqrt(N)
    assert np.abs(y.var(axis=0) - nm.variance(n, 0.0)).max() <= 5 * np.sqrt(2 / N) * nm.variance(n, 0.0)


@pytest.mark.parametrize("n,beta", [(8, 1.0), (9, 2.0), (64, 1.0)])
def test_the_ensemble_spectrum_is_the_tables(n, beta):
    N = 40000
    a, b = nm.pink_coefficients(nm.SEED, np.arange(N // 50), 50, 0, n)
    y = nm.direct_sum(a, b, n, beta).reshape(N, n)
    power = np.abs(np.fft.rfft(y, axis=-1)) ** 2
    want, sd = nm.periodogram_expectation(n, beta)
    assert np.all(np.abs(power.mean(axis=0) - want) <= 5 * sd / np.sqrt(N)), (power.mean(axis=0), want)
    assert abs(y[:, 1].var() - nm.variance(n, beta)) <= 5 * np.sqrt(2 / N) * nm.variance(n, beta)
    rho = nm.correlation(n, beta, 1)
    got = np.corrcoef(y[:, 1], y[:, 2])[0, 1]
    assert abs(got - rho) <= 5 * (1 - rho ** 2) / np.sqrt(N), (got, rho)


def test_the_counter_domains_do_not_collide():
    """Word 1 of the counter: the white noise of the exploration epilogue uses the column block j / 4 <= 127 for A <= 512, pink
    0x80000000 | (j / 2) <= 0x800000ff, OU 0x40000000 | (j / 4): three disjoint ranges, whatever the other words are."""
    A = 512
    white = {em.counter(0, j // 4, 0)[1] for j in range(A)}
    pink = {nm.pink_counter(0, j, 0, 0)[1] for j in range(A)}
    ou = {nm.ou_counter(0, j, 0)[1] for j in range(A)}
    assert max(white) == 127 and min(pink) == 0x80000000 and max(pink) == 0x800000ff and min(ou) == 0x40000000 and max(ou) == 0x4000007f
    assert not (white & pink) and not (white & ou) and not (pink & ou)
    # the same (env, word 1 low bits, words 2, 3) in the three domains gives three different blocks
    k = em.key(nm.SEED)
    blocks = {rp.philox4x32_10((3, tag | 1, 5, 0), k) for tag in (0, nm.PINK_TAG, nm.OU_TAG)}
    assert len(blocks) == 3


def test_the_state_machine_of_the_model():
    m = nm.PinkModel(4, 3, 5, beta=1.0)
    first = m.cache.copy()
    rows = [m.next() for _ in range(5)]
    assert m.t.tolist() == [5] * 4 and m.q.tolist() == [0] * 4 and np.array_equal(np.stack(rows, 1), first)
    done = np.array([0, 1, 0, 0], np.uint8)
    m.next(done)  # every env is exhausted, env 1 is done as well: one new sequence each
    assert m.t.tolist() == [1] * 4 and m.q.tolist() == [1] * 4
    m.next(done)
    assert m.t.tolist() == [2, 1, 2, 2] and m.q.tolist() == [1, 2, 1, 1]
    m.reset(np.array([1, 0, 0, 0]))
    assert m.t.tolist() == [0, 1, 2, 2] and m.q.tolist() == [2, 2, 1, 1]
    ou = nm.OUModel(2, 5, 0.0, 0.5)
    x1 = ou.next()
    assert ou.calls == 1 and np.allclose(x1, ou.ss * nm.normals4(nm.philox(np.arange(2)[:, None], (nm.OU_TAG | np.arange(2))[None, :], 0, 0, nm.SEED)).reshape(2, -1)[:, :5])
    ou.reset()
    assert not ou.x.any()
