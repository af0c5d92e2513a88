"""The data log summarised on the device, without a GPU: the C ABI's entry (exported, typed, where the header puts it), the args
struct against a compiled probe, the build lists, and the NumPy restatement of the reduction (tests/logsum_model.py) against the
reference's own arithmetic on the three committed reference logs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import logsum_model as lm

ROOT = lm.ROOT
ARG_FIELDS = ["drop_last", "bins", "hist_ev", "reserved", "lo", "hi", "scal", "deg_sum", "soh_last", "prof_sum", "prof_cnt", "hist"]
LOG_TITLE = "device-side data log"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_typed_and_sits_in_the_data_log_section():
    from fleetrl_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "fleet_hip.h")).read()
    assert re.search(r"^#define FLEET_ABI_VERSION 11$", hdr, flags=re.M) and _capi.ABI_VERSION == 11
    assert "fleet_log_summary_dev" in _capi.EXPORTED_SYMBOLS
    assert re.search(r"^int fleet_log_summary_dev\(fleet_handle h, const FleetLogSummaryArgs\* args, size_t args_size\);$", hdr, flags=re.M)
    titles = re.findall(r"^/\* ---- (.*?) [(-]", hdr, flags=re.M)
    assert titles.count(LOG_TITLE) == 1
    start = hdr.index("/* ---- " + LOG_TITLE)
    section = hdr[start:hdr.index("/* ---- ", start + 1)]
    # the entry and its struct lie in the existing section, behind fleet_log_read, and open no section of their own
    assert section.index("int fleet_log_read(") < section.index("} FleetLogSummaryArgs;") < section.index("int fleet_log_summary_dev(")
    assert hdr.count("} FleetLogSummaryArgs;") == 1
    assert "entry added under FLEET_ABI_VERSION 11" in re.sub(r"\s*\n \*\s*", " ", section)
    lib = _capi.load_library()
    fn = lib.fleet_log_summary_dev
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.POINTER(_capi.FleetLogSummaryArgs), C.c_size_t]
    assert _capi.LOG_SUMMARY_SCALARS == lm.SCALARS and _capi.LOG_SUMMARY_MAX_BINS == 256


def test_struct_size_and_offsets_match_the_header(tmp_path):
    from fleetrl_amd import _capi

    cls = _capi.FleetLogSummaryArgs
    assert [n for n, _ in cls._fields_] == ARG_FIELDS
    exprs = ["sizeof(FleetLogSummaryArgs)"] + [f"offsetof(FleetLogSummaryArgs, {n})" for n in ARG_FIELDS]
    want = [C.sizeof(cls)] + [getattr(cls, n).offset for n in ARG_FIELDS]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fleet_hip.h"\nint main(){' +
                   "".join(f'printf("%zu ", (size_t){e});' for e in exprs) + "return 0;}")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want and C.sizeof(cls) == 80


def test_the_source_is_built_and_the_python_surface_is_exported():
    import fleetrl_amd
    from fleetrl_amd import build, evaluation
    from fleetrl_amd.batch import FleetBatch

    assert "fleet_logsum.hip" in build.SOURCES and "fleet_logsum.h" in build.HEADERS
    for name in ("LogSummary", "summarize_log", "compare", "evaluate_strategies"):
        assert getattr(fleetrl_amd, name) is getattr(evaluation, name)
    assert callable(FleetBatch.log_summary)
    src = open(os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_logsum.h")).read()
    assert re.search(r"constexpr int kLogsumRows = (\d+);", src).group(1) == str(lm.BLOCK)
    assert re.search(r"constexpr int kLogsumMaxBins = (\d+);", src).group(1) == "256"


# ---- the model against the reference's arithmetic --------------------------------------------------------------------------------
def ring_from_fixture(g, cap: int, shift: int = 0) -> dict:
    """`fleet_log_read`-shaped arrays that hold the fixture's DataLogger rows: row k of env e (k counted from `shift`, as if
    `shift` older rows had been written and overwritten) in slot k % cap.  The per-EV energy is what the Q8 carry-over of
    `log_charge` came from: the logged value minus the carried energy of the other sign."""
    E, N = g.E, g.N
    dates = np.asarray(g.tab_dates).astype("datetime64[s]").astype(np.int64)
    lg = {"pos": np.zeros(E, np.int32), "row": np.zeros((cap, E), np.int32), "env": np.zeros((cap, E, 4)),
          "ev": np.zeros((cap, E, 4, N))}
    for e in range(E):
        n = int(g.log_n[e])
        assert n <= cap
        t = np.searchsorted(dates, g.log_time[e, :n])
        assert (dates[t] == g.log_time[e, :n]).all()
        ep = g.log_episode[e, :n]
        is_reset = np.r_[True, ep[1:] != ep[:-1]]  # the first row of every episode is the one reset() writes
        act, charge = g.log_action[e, :n], g.log_charge[e, :n]
        energy = np.zeros((n, N))
        last = np.zeros((n, 2))  # carried charging / discharging energy
        for c in range(N):
            neg = (act[:, c] < 0).astype(int)
            pos_or_neg = (act[:, c] >= 0) | (act[:, c] < 0)
            other = last[np.arange(n), 1 - neg]
            energy[:, c] = np.where(pos_or_neg, charge[:, c] - other, 0.0)
            last[np.arange(n)[pos_or_neg], neg[pos_or_neg]] = energy[pos_or_neg, c]
        assert not charge[is_reset].any() and not g.log_reward[e, :n][is_reset].any()
        slots = (shift + np.arange(n)) % cap
        lg["pos"][e] = shift + n
        lg["row"][slots, e] = (t.astype(np.int64) | np.where(is_reset, 0x80000000, 0)).astype(np.uint32).view(np.int32)
        lg["env"][slots, e] = np.stack([g.log_reward[e, :n], g.log_cashflow[e, :n], g.log_grid[e, :n], g.log_socv[e, :n]], axis=1)
        lg["ev"][slots, e] = np.stack([act, energy, g.log_deg[e, :n], g.log_soh[e, :n]], axis=1)
    return lg


def model_of(g, lg, **kw):
    return lm.summarize(lg, g.tables.hour, g.tables.minute, minutes_per_step=int(g.rc.minutes),
                        price_multiplier=g.rc.price_multiplier, calc_deg=g.rc.calc_deg, **kw)


@pytest.mark.parametrize("name,prefix", lm.FIXTURES)
def test_model_meets_the_reference_arithmetic_on_the_committed_logs(name, prefix):
    g = lm.load_fixture(name, prefix)
    n = int(g.log_n.max())
    viol, degs, edge = set(), set(), 0
    for cap, shift, drop, hist_ev in ((n, 0, 0, 0), (n + 9, 0, 2, 0), (n, 37, 2, -1), (n, 64, 0, g.N - 1)):  # 37, 64: a wrapped ring
        lg = ring_from_fixture(g, cap, shift)
        got = model_of(g, lg, drop_last=drop, hist_ev=hist_ev)
        for e in range(g.E):
            ref = lm.reference_aggregates(g, e, drop, hist_ev=hist_ev)
            lm.assert_meets_reference(got, e, ref, f"{name} env {e} cap {cap} shift {shift} drop {drop}")
            # the blocked order against NumPy's own sum of the same column: far inside the tolerance
            assert abs(got["scal"][e, 1] - ref["reward"]) <= 1e-12 * max(1.0, abs(ref["reward"]))
            viol.add(ref["violations"])
            degs.add(int(got["scal"][e, 7]))
            a = g.log_action[e, :ref["rows"]]
            edge += int(np.isin(a, (-1.0, 0.0, 1.0)).sum())
    print(name, "violation rows", sorted(viol), "degradation rows", sorted(degs), "actions on a bin edge", edge)
    assert edge >= 100 and min(degs) >= 1  # the edge rule and the 14:45 rows are exercised


def test_model_windows_and_histogram_rule():
    assert lm.window(0, 50, 0) == (0, 0) and lm.window(7, 50, 9) == (0, 0) and lm.window(120, 50, 2) == (70, 118)
    a = np.array([-1.0, -0.96, -0.9600000000000001, 0.0, 0.5, 1.0, 1.0000001, -1.0000001, np.nan, 0.96])
    for bins, lo, hi in ((50, -1.0, 1.0), (7, -0.5, 0.75), (256, -1.0, 1.0), (1, 0.0, 1.0)):
        np.testing.assert_array_equal(lm.histogram(a, bins, lo, hi), np.histogram(a[~np.isnan(a)], bins=bins, range=(lo, hi))[0])
    rng = np.random.default_rng(3)
    x = np.round(rng.uniform(-1.2, 1.2, 20000), 2)
    np.testing.assert_array_equal(lm.histogram(x, 50, -1.0, 1.0), np.histogram(x, bins=50, range=(-1.0, 1.0))[0])
    # the butterfly is a fixed pairing: exact on integers, and not the left-to-right sum in general
    v = rng.integers(-5, 6, size=(4, 130)).astype(np.float64)
    np.testing.assert_array_equal(lm.butterfly_ev_sum(v), v.sum(axis=1))
    def serial(n):
        s = 0.0
        for _ in range(n):
            s = s + 0.1
        return s

    assert lm.blocked_sum([0.1] * 130) == (serial(64) + serial(64)) + serial(2) != serial(130)
