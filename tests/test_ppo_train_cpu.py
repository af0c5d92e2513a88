"""PPO's whole update without a GPU: the C ABI's section, its position, bindings and struct layouts against a compiled probe, every
refusal that needs no device, and the NumPy restatement of tests/train_model.py on its own: the shuffle is a bijection, changes with the
epoch and the seed and is uniform on small domains; the normalisation stays within the project's bound of a float64 evaluation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import train_model as tm

ROOT = tm.ROOT
F32 = np.float32
ENTRIES = ("fleet_train_create", "fleet_train_destroy", "fleet_train_last_error", "fleet_train_describe", "fleet_train_ppo_dev",
           "fleet_train_indices_dev")
ARG_FIELDS = ["struct_bytes", "n_epochs", "batch_size", "normalize_advantage", "clip_range", "vf_coef", "ent_coef", "reserved", "lr", "beta1",
              "beta2", "eps", "max_grad_norm", "seed", "first_epoch", "stats"]
INFO_FIELDS = ["num_envs", "n_steps", "obs_dim", "act_dim", "max_batch", "n_tensors", "rounds", "min_half_bits", "tile_rows", "cache_rows",
               "staging_bytes", "staging"]
TITLE = "PPO's whole update on the device"
ADAM_TITLE = "Adam and clip_grad_norm_ on the device"
PPO_TITLE = "PPO minibatch gradients on the device"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_section_lies_between_the_targets_and_adam_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_train_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.TRAIN_SYMBOLS) and declared <= set(_capi.EXPORTED_SYMBOLS)
    assert not any(n.startswith("fleet_ppo_") for n in ENTRIES)
    assert hdr.count("---- " + TITLE) == 1 and hdr.count("---- " + ADAM_TITLE) == 1
    assert hdr.index("int fleet_qtarget_describe(") < hdr.index("---- " + TITLE) < hdr.index("---- " + ADAM_TITLE) < hdr.index("---- " + PPO_TITLE)
    section = hdr[hdr.index("---- " + TITLE):hdr.index("---- " + ADAM_TITLE)]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    for said in ("} FleetTrainPpoArgs;", "} FleetTrainInfo;", "#define FLEET_TRAIN_ROUNDS 8", "#define FLEET_TRAIN_MIN_HALF_BITS 4",
                 "#define FLEET_TRAIN_STATS 16", "F = word 0 of philox4x32_10(counter (R, r, epoch_lo, epoch_hi); key (seed_lo, seed_hi)) & mask",
                 "(L, R) = (R, L ^ F)", "until x < n", "first_epoch + e", "advn[b] = (adv[b] - mean32) / (std32 + 1e-8f)",
                 "(double)(B - 1)", "for s = 128, 64, ..., 1", "NaN when vy == 0", "FIVE launches", "must outlive", "POLICY's stream"):
        assert said in section, said
    assert not re.search(r"^(?:int|const char\*)\s+fleet_(?!train_)", section, flags=re.M)  # no entry of a neighbour in it
    assert len(re.findall(r"^/\* ---- ", section, flags=re.M)) == 0  # the section's own opener lies before the slice: none between
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is (C.c_char_p if name.endswith("last_error") else C.c_int), name
    assert len(lib.fleet_train_create.argtypes) == 4 and len(lib.fleet_train_ppo_dev.argtypes) == 5
    assert len(lib.fleet_train_indices_dev.argtypes) == 7 and len(lib.fleet_train_describe.argtypes) == 2


def test_the_family_is_built_exported_and_restated_with_the_headers_constants():
    import fleetrl_amd
    from fleetrl_amd import _capi, build, train

    assert "fleet_train.hip" in build.SOURCES and "fleet_train.h" in build.HEADERS
    assert fleetrl_amd.DevicePPOTrain is train.DevicePPOTrain and train.DevicePPOTrain._prefix == "train"
    assert train.STATS == tm.STATS and len(train.SB3_NAMES) == len(train.STATS)
    assert (_capi.TRAIN_ROUNDS, _capi.TRAIN_MIN_HALF_BITS, _capi.TRAIN_STATS) == (tm.ROUNDS, tm.MIN_HALF_BITS, tm.STATS_LEN) == (8, 4, 16)
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_train.h")).read()
    assert re.search(r"constexpr int kTrainRounds = (\d+);", src).group(1) == str(tm.ROUNDS)
    assert re.search(r"constexpr int kTrainMinHalfBits = (\d+);", src).group(1) == str(tm.MIN_HALF_BITS)
    assert re.search(r"constexpr int kTrainThreads = (\d+);", src).group(1) == str(tm.LANES)


def test_struct_sizes_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    exprs, want = [], []
    for cname, cls, fields in (("FleetTrainPpoArgs", _capi.FleetTrainPpoArgs, ARG_FIELDS), ("FleetTrainInfo", _capi.FleetTrainInfo, INFO_FIELDS)):
        assert [n for n, _ in cls._fields_] == fields
        exprs += [f"sizeof({cname})"] + [f"offsetof({cname}, {n})" for n in fields]
        want += [C.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    exprs += ["FLEET_TRAIN_ROUNDS", "FLEET_TRAIN_MIN_HALF_BITS", "FLEET_TRAIN_STATS", "sizeof(FleetPpoGradArgs)"]
    want += [_capi.TRAIN_ROUNDS, _capi.TRAIN_MIN_HALF_BITS, _capi.TRAIN_STATS, 96]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert C.sizeof(_capi.FleetTrainPpoArgs) == 96 and C.sizeof(_capi.FleetTrainInfo) == 56


# ---- refusals that need no device ------------------------------------------------------------------------------------------------
def _args(**kw):
    from fleetrl_amd import _capi

    a = _capi.FleetTrainPpoArgs()
    a.struct_bytes, a.n_epochs, a.batch_size, a.normalize_advantage = C.sizeof(a), 2, 64, 1
    a.clip_range, a.vf_coef, a.ent_coef, a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = 0.2, 0.5, 0.0, 3e-4, 0.9, 0.999, 1e-5, 0.5
    a.seed, a.first_epoch, a.stats = 1, 0, 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _ptrs(n=5, null_at=None, base=256):
    """(never dereferenced: nothing is launched)"""
    return (C.c_void_p * n)(*[None if i == null_at else base + 64 * i for i in range(n)])


NAN = float("nan")
REFUSALS = {
    "struct_bytes": (dict(struct_bytes=88), "struct_bytes"),
    "n_epochs-zero": (dict(n_epochs=0), "n_epochs must be >= 1, got 0"),
    "n_epochs-negative": (dict(n_epochs=-3), "n_epochs must be >= 1, got -3"),
    "batch_size-zero": (dict(batch_size=0), "batch_size must be >= 1, got 0"),
    "batch_size-negative": (dict(batch_size=-1), "batch_size must be >= 1, got -1"),
    "reserved": (dict(reserved=1), "reserved must be 0"),
    "stats-null": (dict(stats=None), "null stats"),
    # fleet_ppo_grad_dev's, in its words
    "clip_range-zero": (dict(clip_range=0.0), "clip_range must be in (0, 1)"),
    "clip_range-one": (dict(clip_range=1.0), "clip_range must be in (0, 1)"),
    "clip_range-nan": (dict(clip_range=NAN), "clip_range must be in (0, 1)"),
    "vf_coef-nan": (dict(vf_coef=NAN), "vf_coef is NaN"),
    "ent_coef-nan": (dict(ent_coef=NAN), "ent_coef is NaN"),
    # fleet_adam_step_dev's, in its words
    "lr-negative": (dict(lr=-1e-3), "lr must be finite and >= 0"),
    "lr-nan": (dict(lr=NAN), "lr must be finite and >= 0"),
    "lr-inf": (dict(lr=float("inf")), "lr must be finite and >= 0"),
    "eps-negative": (dict(eps=-1e-8), "eps must be finite and >= 0"),
    "eps-nan": (dict(eps=NAN), "eps must be finite and >= 0"),
    "beta1-one": (dict(beta1=1.0), "beta1 must be in [0, 1)"),
    "beta1-nan": (dict(beta1=NAN), "beta1 must be in [0, 1)"),
    "beta2-one": (dict(beta2=1.0), "beta2 must be in [0, 1)"),
    "beta2-negative": (dict(beta2=-1e-9), "beta2 must be in [0, 1)"),
    "max_grad_norm-nan": (dict(max_grad_norm=NAN), "max_grad_norm is NaN"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_the_update_refuses_bad_arguments_with_a_reason_and_without_a_device(case):
    """The arguments are looked at before the handle: with a null handle the reason goes to fleet_train_last_error(NULL)."""
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fields, word = REFUSALS[case]
    assert lib.fleet_train_ppo_dev(None, C.byref(_args(**fields)), _ptrs(), _ptrs(base=8192), 5) == _capi.ERR_INVALID
    why = lib.fleet_train_last_error(None).decode()
    assert why.startswith("fleet_train_ppo_dev: ") and word in why, why


def test_the_update_refuses_null_structs_arrays_and_aliases_and_names_the_null_handle():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    fn = lib.fleet_train_ppo_dev
    last = lambda: lib.fleet_train_last_error(None).decode()  # noqa: E731
    P, G = _ptrs(), _ptrs(base=8192)
    assert fn(None, None, P, G, 5) == _capi.ERR_INVALID and last() == "fleet_train_ppo_dev: null FleetTrainPpoArgs"
    assert fn(None, C.byref(_args()), None, G, 5) == _capi.ERR_INVALID and "null params" in last()
    assert fn(None, C.byref(_args()), P, None, 5) == _capi.ERR_INVALID and "null grads" in last()
    assert fn(None, C.byref(_args()), P, G, 0) == _capi.ERR_INVALID and "count must be the policy's tensors plus one (log_std), got 0" in last()
    assert fn(None, C.byref(_args()), _ptrs(27), _ptrs(27, base=8192), 27) == _capi.ERR_INVALID and "got 27" in last()
    assert fn(None, C.byref(_args()), _ptrs(null_at=2), G, 5) == _capi.ERR_INVALID and "parameter tensor 2 is null" in last()
    assert fn(None, C.byref(_args()), P, _ptrs(null_at=4, base=8192), 5) == _capi.ERR_INVALID and "gradient tensor 4 is null" in last()
    alias = _ptrs(base=8192)
    alias[1] = P[1]
    assert fn(None, C.byref(_args()), P, alias, 5) == _capi.ERR_INVALID and "parameter tensor 1 is its own gradient" in last()
    for ok in (_args(), _args(max_grad_norm=0.0), _args(normalize_advantage=0), _args(lr=0.0, eps=0.0, beta1=0.0, beta2=0.0),
               _args(batch_size=2 ** 31 - 1, n_epochs=10, seed=2 ** 64 - 1, first_epoch=2 ** 63)):
        assert fn(None, C.byref(ok), P, G, 5) == _capi.ERR_INVALID and last() == "fleet_train_ppo_dev: null handle"


def test_create_describe_and_indices_refuse_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    last = lambda: lib.fleet_train_last_error(None).decode()  # noqa: E731
    h = C.c_void_p()
    fake = C.c_void_p(4096)  # (never dereferenced: the null handle in front of it is met first)
    for a, word in (((None, fake, fake), "null rollout handle"), ((fake, None, fake), "null gradient handle"),
                    ((fake, fake, None), "null optimiser handle"), ((None, None, None), "null rollout handle")):
        assert lib.fleet_train_create(*a, C.byref(h)) == _capi.ERR_INVALID and not h
        assert last() == "fleet_train_create: " + word
    assert lib.fleet_train_create(None, None, None, None) == _capi.ERR_INVALID and last() == "fleet_train_create: null output handle"
    assert lib.fleet_train_destroy(None) == _capi.OK
    assert lib.fleet_train_describe(None, None) == _capi.ERR_INVALID
    fn = lib.fleet_train_indices_dev
    for a, word in (((0, 1, 0, 0, 0, 4096), "n must be >= 1, got 0"), ((-5, 1, 0, 0, 0, 4096), "n must be >= 1, got -5"),
                    ((10, 1, 0, -1, 2, 4096), "lie outside [0, 10)"), ((10, 1, 0, 0, -2, 4096), "lie outside [0, 10)"),
                    ((10, 1, 0, 8, 3, 4096), "positions 8 .. +3 lie outside [0, 10)"), ((2 ** 31 - 1, 1, 0, 2 ** 31 - 2, 2, 4096), "lie outside"),
                    ((10, 1, 0, 0, 10, None), "null out"), ((10, 1, 0, 0, 10, 4096), "null handle")):
        assert fn(None, *a) == _capi.ERR_INVALID
        assert last().startswith("fleet_train_indices_dev: ") and word in last(), last()


# ---- the permutation -------------------------------------------------------------------------------------------------------------
BIJECTION_N = (1, 2, 3, 4, 5, 15, 16, 17, 64, 65, 1000, 4097, 65537)


@pytest.mark.parametrize("n", BIJECTION_N)
def test_perm_is_a_bijection(n):
    walks = []
    for seed, epoch in ((0, 0), (7, 3), (2 ** 64 - 1, 2 ** 40 + 5)):
        v = tm.perm(n, seed, epoch, np.arange(n), walks=walks)
        print(n, seed, epoch, "longest walk", walks[0])
        assert v.min() == 0 and v.max() == n - 1 and np.unique(v).size == n
        assert walks[0] <= (1 << (2 * tm.half_bits(n))) - n + 1  # a walk leaves [0, n) through at most every value outside it
    assert tm.half_bits(n) >= tm.MIN_HALF_BITS and (1 << (2 * tm.half_bits(n))) >= n
    assert n <= 256 or (1 << (2 * (tm.half_bits(n) - 1))) < n  # the smallest domain above the minimum


def test_half_bits_at_the_edges():
    assert [tm.half_bits(n) for n in (1, 256, 257, 1024, 1025, 16384, 16385, 2 ** 31 - 1)] == [4, 4, 5, 5, 6, 7, 8, 16]


def test_small_domains_are_not_the_identity_under_every_key():
    for n in (2, 3, 4):
        seen = {tuple(row) for row in tm.perm(n, np.arange(64)[:, None], 0, np.arange(n)[None, :])}
        assert len(seen) == {2: 2, 3: 6, 4: 24}[n], (n, len(seen))  # 64 keys reach every permutation of 2, 3 and 4 values


def test_two_epochs_and_two_seeds_agree_in_less_than_one_percent_of_positions():
    n, p = 1000, np.arange(1000)
    base = tm.perm(n, 11, 4, p)
    for other in (tm.perm(n, 11, 5, p), tm.perm(n, 12, 4, p), tm.perm(n, 11, 4 + 2 ** 32, p), tm.perm(n, 11 + 2 ** 32, 4, p)):
        agree = float((base == other).mean())
        print("agreement", agree)
        assert agree < 0.01


def test_indices_are_slices_of_perm():
    full = tm.indices(4097, 3, 9)
    assert full.dtype == np.int32 and np.array_equal(full[100:117], tm.indices(4097, 3, 9, 100, 17))
    assert np.array_equal(np.sort(full), np.arange(4097))


# ---- the uniformity condition --------------------------------------------------------------------------------------------------------
def chi_square_quantile(df: int) -> float:
    """The 1 - 1e-6 quantile of chi-square with df degrees of freedom: scipy's, or Wilson-Hilferty's approximation
    df * (1 - 2 / (9 df) + z * sqrt(2 / (9 df)))^3 with z = 4.753424, the normal quantile of 1 - 1e-6."""
    try:
        from scipy.stats import chi2

        return float(chi2.ppf(1.0 - 1e-6, df))
    except ImportError:
        c = 2.0 / (9.0 * df)
        return df * (1.0 - c + 4.753424 * c ** 0.5) ** 3


@pytest.mark.parametrize("n", [5, 15, 40])
def test_position_by_value_counts_are_uniform_over_12000_keys(n):
    """Seeds 0 .. 11999 at epoch 3: the chi-square statistic of the n x n count table lies below the 1 - 1e-6 quantile for (n - 1)^2
    degrees of freedom.  The key set is fixed, so this is deterministic."""
    stat, df = tm.chi_square_table(n, np.arange(12000), 3)
    q = chi_square_quantile(df)
    print(f"n={n}: chi-square {stat:.1f} at {df} degrees of freedom, quantile {q:.1f}")
    assert df == (n - 1) ** 2 and stat < q


def test_the_four_round_smallest_domain_construction_fails_the_uniformity_condition():
    """What a careless construction does: four rounds over the smallest domain (h = 2 at n = 5)."""
    stat, df = tm.chi_square_table(5, np.arange(12000), 3, rounds=4, min_half_bits=1)
    q = chi_square_quantile(df)
    print(f"4 rounds, smallest domain, n=5: chi-square {stat:.1f}, quantile {q:.1f}")
    assert stat > 4 * q
    wh = 16 * (1.0 - 2.0 / 144 + 4.753424 * (2.0 / 144) ** 0.5) ** 3
    assert abs(wh - q) < 0.02 * q  # the two quantiles of the helper agree where both exist


# ---- the normalisation ---------------------------------------------------------------------------------------------------------------
def _advantages(B, kind, rng):
    if kind == "normal":
        return rng.standard_normal(B).astype(F32)
    if kind == "offset":  # a mean as large as the spread
        return (rng.standard_normal(B) * 0.5 + 1.5).astype(F32)
    if kind == "large":  # |adv| up to 1e4
        a = (rng.standard_normal(B) * 3e3).astype(F32)
        a[0] = F32(1e4)
        return np.clip(a, -1e4, 1e4).astype(F32)
    return np.full(B, F32(0.7251), F32)  # constant: std 0


@pytest.mark.parametrize("kind", ["normal", "offset", "large", "constant"])
@pytest.mark.parametrize("B", [2, 3, 16, 17, 257])
def test_normalisation_stays_within_the_projects_bound_of_float64(B, kind):
    """|model - ref64| <= 8 max(eps_ref, 2^-24 max|ref64|): ref64 = SB3's expression in float64, eps_ref = |SB3's expression in
    torch float32 - ref64|.  A constant vector gives 0 / 1e-8: finite, and exactly 0."""
    torch = pytest.importorskip("torch")
    a = _advantages(B, kind, np.random.default_rng(100 * B + len(kind)))
    got = tm.normalise(a)
    a64 = a.astype(np.float64)
    ref = (a64 - a64.mean()) / (a64.std(ddof=1) + 1e-8)
    t = torch.from_numpy(a)
    ref32 = ((t - t.mean()) / (t.std() + 1e-8)).numpy().astype(np.float64)
    eps_ref = float(np.abs(ref32 - ref).max())
    err, bound = float(np.abs(got.astype(np.float64) - ref).max()), 8 * max(eps_ref, 2.0 ** -24 * float(np.abs(ref).max()))
    print(f"B={B} {kind}: eps_ref {eps_ref:.3g} model {err:.3g} bound {bound:.3g}")
    assert got.dtype == F32 and np.isfinite(got).all() and err <= bound
    if kind == "constant":
        mean, std = tm.normalise_stats(a)
        assert mean == a[0] and std == 0 and not got.any()
    if kind == "large":
        assert np.abs(a).max() == 1e4


def test_normalisation_leaves_one_row_and_the_switched_off_case_alone():
    a = np.array([3.5], F32)
    assert np.array_equal(tm.normalise(a), a) and np.array_equal(tm.normalise(np.array([1.0, 2.0], F32), on=False), [1.0, 2.0])
    two = tm.normalise(np.array([1.0, 3.0], F32))  # mean 2, unbiased std sqrt(2)
    assert np.allclose(two, [-1 / np.sqrt(2), 1 / np.sqrt(2)], rtol=1e-6)


def test_the_ordered_sum_is_the_stated_tree_and_the_statistics_follow_the_header():
    x = np.random.default_rng(3).standard_normal(600)
    lanes = [sum(x[t::256].tolist(), 0.0) for t in range(256)]  # ascending inside a lane
    s = 128
    while s:
        lanes = [lanes[t] + lanes[t + s] for t in range(s)] + lanes[s:]
        s //= 2
    assert tm.tree_sum(x) == lanes[0]
    assert tm.minibatches(15, 4) == [(0, 4), (4, 4), (8, 4), (12, 3)] and tm.minibatches(15, 99) == [(0, 15)] == tm.minibatches(15, 15)
    y = np.random.default_rng(4).standard_normal((5, 3)).astype(F32)
    v = (y + 0.1 * np.random.default_rng(5).standard_normal((5, 3))).astype(F32)
    ev = tm.explained_variance(y, v)
    want = 1 - np.var(y.astype(np.float64) - v.astype(np.float64)) / np.var(y.astype(np.float64))
    assert abs(ev - want) <= 1e-12 and np.isnan(tm.explained_variance(np.full((5, 3), 2.5, F32), v))
    g = [np.array([1, 2, 3, 4, 5, 6, 0, 0], F32), np.array([3, 2, 1, 0, -1, -2, 0, 0], F32)]
    blk = tm.stats_block(g, ev, 0.5)
    assert blk.tolist()[:9] == [2.0, 2.0, 2.0, 2.0, 2.0, 0.0, 2.0, float(ev), 0.5] and not blk[9:].any()
