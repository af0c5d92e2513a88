"""Exploration on the device without a GPU: the C ABI's declarations and bindings, the struct's layout against a compiled probe, and
the model of tests/explore_model.py -- Philox's published vectors, the counter layout, the moments of the noise."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import explore_model as em
import policy_model as pm
import replay_model as rp

ROOT = pm.ROOT
ENTRIES = ("fleet_explore_act_dev",)
FIELDS = ["struct_bytes", "mode", "noise_mode", "reserved0", "seed", "step", "env_id_offset", "reserved1", "scale", "shift", "noise_lo",
          "noise_hi", "noise", "actions", "env_actions", "log_prob", "values", "mean"]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_section_is_placed_after_the_policy_section_and_every_entry_is_bound():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    declared = set(re.findall(r"^(?:int|const char\*)\s+(fleet_explore_\w+)\s*\(", hdr, flags=re.M))
    assert declared == set(ENTRIES) == set(_capi.EXPLORE_SYMBOLS)
    assert hdr.index("MLP policy on the device") < hdr.index("exploration actions on the device")
    assert hdr.index("int fleet_policy_describe(") < hdr.index("exploration actions on the device")
    section = hdr[hdr.index("exploration actions on the device"):]
    assert "entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays" in section[:400]
    assert "} FleetExploreArgs;" in section
    # the policy section keeps its words
    assert "Calls on one policy are serialised by the caller.  No atomics, no random numbers. */" in hdr
    lib = _capi.load_library()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == 5 and fn.restype is C.c_int, name
    assert set(ENTRIES) <= set(_capi.EXPORTED_SYMBOLS)
    for name, value in (("GAUSSIAN", _capi.EXPLORE_GAUSSIAN), ("ACTION_NOISE", _capi.EXPLORE_ACTION_NOISE), ("UNIFORM", _capi.EXPLORE_UNIFORM),
                        ("NOISE_DRAW", _capi.EXPLORE_NOISE_DRAW), ("NOISE_GIVEN", _capi.EXPLORE_NOISE_GIVEN)):
        assert re.search(rf"^#define FLEET_EXPLORE_{name} {value}$", hdr, flags=re.M), name


def test_struct_size_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    cls = _capi.FleetExploreArgs
    assert [n for n, _ in cls._fields_] == FIELDS
    exprs = ["sizeof(FleetExploreArgs)"] + [f"offsetof(FleetExploreArgs, {n})" for n in FIELDS]
    want = [C.sizeof(cls)] + [getattr(cls, n).offset for n in FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert cls.seed.offset == 16 and cls.actions.offset == C.sizeof(cls) - 5 * C.sizeof(C.c_void_p)


def test_a_null_handle_is_refused_without_a_device():
    from fleetrl_amd import _capi

    lib = _capi.load_library()
    a = _capi.FleetExploreArgs()
    assert lib.fleet_explore_act_dev(None, None, 1, None, C.byref(a)) == _capi.ERR_INVALID


# ---- the model -------------------------------------------------------------------------------------------------------------------
def test_philox_in_the_model_passes_the_published_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds, through the scalar generator and through the model's array form."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, k, want in kat:
        assert rp.philox4x32_10(ctr, k) == want
    # the array form: counter (env, block, step lo, step hi), key (seed lo, seed hi)
    seed, step = (0x299f31d0 << 32) | 0xa4093822, (0x03707344 << 32) | 0x13198a2e
    w = em.words(seed, [0x243f6a88], 4 * 0x10, step)  # blocks 0 .. 15
    for b in (0, 3, 15):
        assert tuple(int(v) for v in w[0, b]) == em.block_words(seed, 0x243f6a88, b, step)
    assert em.block_words(seed, 0x243f6a88, 0x85a308d3, step) == kat[2][2]  # the third vector through the model's counter scheme
    assert em.block_words(2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1) == kat[1][2] and em.block_words(0, 0, 0, 0) == kat[0][2]
    big = em.words(em.SEED, np.array([0, 7, 2 ** 32 - 1]), 9, 2 ** 32 + 5)
    for i, e in enumerate((0, 7, 2 ** 32 - 1)):
        for b in range(3):
            assert tuple(int(v) for v in big[i, b]) == em.block_words(em.SEED, e, b, 2 ** 32 + 5)


def test_the_counter_tells_env_column_block_and_both_step_halves_apart():
    base = dict(env=5, block=2, step=(3 << 32) | 9)
    ref = em.block_words(em.SEED, **base)
    seen = {ref}
    for change in (dict(env=6), dict(block=3), dict(step=(3 << 32) | 10), dict(step=(4 << 32) | 9)):
        got = em.block_words(em.SEED, **{**base, **change})
        assert all(g != r for g, r in zip(got, ref)), change  # (every word of the block changes)
        seen.add(got)
    assert len(seen) == 5
    assert em.counter(5, 2, (3 << 32) | 9) == (5, 2, 9, 3) and em.key(em.SEED) == (em.SEED & 0xffffffff, em.SEED >> 32)
    assert em.block_words(em.SEED ^ (1 << 40), **base) != ref  # the key's high half counts
    # columns 4b .. 4b+3 come from block b; the draw of a row does not depend on the batch around it
    full = em.normals(em.SEED, np.arange(37), 13, 7)
    assert np.array_equal(full[16:], em.normals(em.SEED, np.arange(16, 37), 13, 7))
    assert np.array_equal(full[:, :5], em.normals(em.SEED, np.arange(37), 5, 7))


def test_uniforms_and_box_muller_stay_in_their_ranges():
    x = np.array([0, 255, 256, 2 ** 32 - 1], dtype=np.uint64)
    assert em.u_open_low(x).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]
    assert em.u_open_high(x).tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert np.array_equal(em.u_open_low(x).astype(np.float32).astype(np.float64), em.u_open_low(x))  # exact in float32
    assert abs(em.EPS_MAX - 5.768) < 1e-3 and em.EPS_MAX <= 5.77
    u = em.uniforms(em.SEED, np.arange(64), 7, 1)
    assert u.shape == (64, 7) and (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 0.05


def test_model_noise_has_the_moments_of_a_standard_normal():
    """The seed and shape the GPU test uses: n = 4096 x 50 draws, every check at 5 standard errors."""
    E, A = em.STAT_SHAPE
    ids = np.arange(E)
    m = em.moments(em.normals(em.SEED, ids, A, 0), em.normals(em.SEED, ids, A, 1))
    print(m)
    assert m["n"] == 204800 and em.check_moments(m) == []


def test_model_modes_known_answers():
    a, env, lp = em.gaussian([[0.5, -0.9]], [0.0, np.log(2.0)], [[1.0, -1.0]])
    assert np.allclose(a, [[1.5, -2.9]]) and env.tolist() == [[1.0, -1.0]]
    assert np.isclose(lp[0], -0.5 - em.LOG_SQRT_2PI - 0.5 - np.log(2.0) - em.LOG_SQRT_2PI)
    assert np.allclose(lp, em.log_prob_torch32(a, [[0.5, -0.9]], [0.0, np.log(2.0)]), atol=1e-6)
    assert em.action_noise([[0.9, 0.0]], [0.5, 0.5], [0.0, 0.25], [[1.0, -1.0]]).tolist() == [[1.0, -0.25]]
    assert em.uniform(-1.0, 3.0, [0.0, 0.25]).tolist() == [-1.0, 0.0]
