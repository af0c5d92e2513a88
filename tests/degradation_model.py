"""Plain float64 restatement of the reference's two degradation models, run on a given series of logged SOC samples.

The kernels' rainflow count and SEI pass are checked against THIS, fed with the kernels' own samples: every exact-equality
decision of the reversal extraction (an equal-sample skip, a `X < Y` tie of the three-point rule) is then taken on the same
numbers on both sides, so the only differences left are the documented stress approximation (<= 1.4e-9 relative) and
summation order.  Against the CPU oracle, which logs its own samples, a last-bit SOC difference can flip such a tie; the
attribution helper at the end proves that this -- and nothing else -- is what happened to an EV whose bookkeeping differs.

  * SeiModel: RainflowSeiDegradation.calculate_degradation (rainflow_sei_degradation.py:91-212), one row per EV.  The cycles
    are the C `extract_cycles` of the oracle (oracle.fleet_oracle.rainflow_many; pinned by tests/test_oracle_rainflow.py);
    the per-cycle stresses are computed elementwise over all new cycles at once with the same numpy array operations as the
    reference's pandas columns, the scalar terms with the libm `pow` Python uses, the sums per EV with np.sum on the
    EV's own slice (the reference's Series.sum / Series.mean).
  * EmpiricalModel: EmpiricalDegradation.calculate_degradation (empirical_degradation.py:29-99; quirks Q1, Q5).
  * Recount: E envs x N EVs as FleetEnv drives them -- LogDataDeg.soc_log cleared and the env-side SoH set back at reset()
    (fleet_environment.py:338-345), one sample appended per step (:655-656), the model run on the whole log on every 14:45 row
    (:665) and its degradation subtracted from the env-side SoH (:671).  The model's own state (fd_cyc, fd_cal, l,
    rainflow_length, its soh) persists across episodes (quirk Q6).

Test infrastructure: imported by tests only (like golden_util).  Never a conftest.
"""
from __future__ import annotations

import math

import numpy as np

from fleetrl_amd import _capi

# rainflow_sei_degradation.py:36-54
ALPHA_SEI, BETA_SEI = 5.75E-2, 121
KD1, KD2, KD3 = 1.4E5, -5.01E-1, -1.23E5
K_SIGMA, SIGMA_REF = 1.04, 0.5
K_TEMP, TEMP_REF = 6.93E-2, 25
K_DT = 4.14E-10
E = math.e  # np.e


def deg_rows(tables, t):
    """The degradation rows: a step whose NEW time row (after `time += dt`, fleet_environment.py:508) reads 14:45 runs the model
    (:665; fleet_oracle.c step_env_once, `tb->hour[t] == 14 && tb->minute[t] == 45` with t the advanced row)."""
    t = np.asarray(t)
    return (np.asarray(tables.hour)[t] == 14) & (np.asarray(tables.minute)[t] == 45)


class SeiModel:
    """RainflowSeiDegradation for M EVs (row m = one EV), float64, the reference's operation order."""

    def __init__(self, M: int, init_soh: float, temp: float):
        self.init_soh, self.temp = float(init_soh), float(temp)
        self.soh = np.ones(M) * self.init_soh  # :31
        self.l = np.ones(M) - self.soh  # :34
        self.rf_len = np.ones(M)  # :57
        self.fd_cyc = np.zeros(M)  # :60
        self.fd_cal = np.zeros(M)  # :63
        self.err = np.zeros(M, dtype=np.uint32)  # DOD_RANGE / NEG_LIFE / SOH_MISMATCH, where the reference raises
        t = self.temp
        self.stress_temp = E ** (K_TEMP * (t - TEMP_REF) * ((TEMP_REF + 273.15) / (t + 273.15)))  # :72-73 (a Python float)

    def evaluate(self, rows, series, lengths, dt: float) -> np.ndarray:
        """calculate_degradation for the EVs `rows` on their logs `series[k, :lengths[k]]`; returns their degradation."""
        from oracle.fleet_oracle import rainflow_many

        rows = np.asarray(rows)
        cyc, nc = rainflow_many(series, lengths)  # [K, S, (range, mean, count, end)]
        deg = np.zeros(len(rows))
        upd = np.flatnonzero(nc > self.rf_len[rows])  # :143
        if upd.size:
            # the new complete entries, iloc[rainflow_length - 1 : len - 1] (:146), of every updating EV, concatenated
            lo = self.rf_len[rows[upd]].astype(np.int64) - 1
            hi = nc[upd].astype(np.int64) - 1
            owner = np.repeat(np.arange(upd.size), hi - lo)
            pos = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if owner.size else np.zeros(0, np.int64)
            new = cyc[upd[owner], pos]  # [cycles, 4], contiguous: numpy runs the same loops as on a pandas column
            dod, avg_soc, sev = new[:, 0].copy(), new[:, 1].copy(), new[:, 2].copy()
            eff = np.clip(dod * sev, 0, 1)  # :170
            with np.errstate(divide="ignore"):
                s_dod = (KD1 * (eff ** KD2) + KD3) ** -1  # :68 (an effective DoD of 0 gives 0 ** -0.501 = inf -> 0)
            s_soc = E ** (K_SIGMA * (avg_soc - SIGMA_REF))  # :70
            rate = s_dod * s_soc * self.stress_temp  # :77-79
            bounds = np.concatenate([[0], np.cumsum(hi - lo)])
        for k in range(upd.size):
            j = int(upd[k])
            i = int(rows[j])
            n = int(nc[j])
            c = cyc[j, :n]
            battery_age = int(c[:, 3].max()) * dt * 3600  # :138 (np.max of the object column End: a Python int)
            mean_soc_cal = np.sum(c[:, 1]) / n  # :140 (Series.mean of a float64 column)
            if dod[bounds[k]:bounds[k + 1]].max() > 5:  # :164-167
                self.err[i] |= _capi.DEVERR_DOD_RANGE
            s = np.sum(rate[bounds[k]:bounds[k + 1]])  # :174 (np.sum of the Series)
            if self.init_soh == 1.0:
                self.fd_cyc[i] += s
                self.fd_cal[i] = K_DT * battery_age * E ** (K_SIGMA * (mean_soc_cal - SIGMA_REF)) * self.stress_temp  # :175, :81-83
                fd = self.fd_cyc[i] + self.fd_cal[i]
                new_l = 1 - ALPHA_SEI * E ** (-BETA_SEI * fd) - (1 - ALPHA_SEI) * E ** (-fd)  # :176, :85-86
                if new_l < 0:
                    self.err[i] |= _capi.DEVERR_NEG_LIFE  # :179-180
            else:  # :184-186 -- `+=` of an array: well-defined for a single new cycle only; summed like the oracle (quirk Q4)
                self.fd_cyc[i] += s
                self.fd_cal[i] = K_DT * battery_age * E ** (K_SIGMA * (mean_soc_cal - SIGMA_REF)) * self.stress_temp
                new_l = 1 - (1 - self.l[i]) * E ** (-(self.fd_cyc[i] + self.fd_cal[i]))  # :89
            deg[j] = new_l - self.l[i]  # :189
            self.l[i] = new_l  # :192
            self.rf_len[i] = n  # :195
        self.soh[rows] -= deg  # :206
        bad = np.abs(self.soh[rows] - (1 - self.l[rows])) > 0.0001  # :209-210
        self.err[rows[bad]] |= _capi.DEVERR_SOH_MISMATCH
        return deg


class EmpiricalModel:
    """EmpiricalDegradation for M EVs: the last two log entries (empirical_degradation.py:63-64)."""

    def __init__(self, M: int, init_soh: float, evse_power: float):
        self.soh = np.ones(M) * float(init_soh)  # :27
        self.evse_power = float(evse_power)
        self.err = np.zeros(M, dtype=np.uint32)

    def evaluate(self, rows, old_soc, new_soc, dt: float) -> np.ndarray:
        avg_soc = (old_soc + new_soc) / 2  # :67
        cal_soc = np.asarray([0, 40, 90])  # :70-72: a SOC on a [0, 1] scale is always nearest to 0 (quirk Q1)
        closest = cal_soc[np.abs(cal_soc[None, :] - avg_soc[:, None]).argmin(axis=1)]
        cal_aging = np.where(closest == 0, 0.0065 * dt / 8760, np.where(closest == 40, 0.0293 * dt / 8760, 0.065 * dt / 8760))
        dod = np.abs(new_soc - old_soc)  # :85
        cycle_loss = dod * 0.000125 / 2 if self.evse_power <= 22.0 else dod * 0.000167 / 2  # :88-91
        deg = cal_aging + cycle_loss  # :94
        self.soh[rows] -= deg  # :96
        return deg


class Recount:
    """E envs x N EVs: the per-episode logs, the env-side SoH and one degradation model over all E * N EVs."""

    def __init__(self, E: int, N: int, deg: str, *, init_soh: float, temp: float, dt: float, evse_power: float = 0.0, cap: int = 64):
        self.E, self.N, self.deg, self.dt, self.init_soh = E, N, deg, float(dt), float(init_soh)
        self.model = SeiModel(E * N, init_soh, temp) if deg == "rainflow" else EmpiricalModel(E * N, init_soh, evse_power)
        self.log = np.zeros((E, N, cap))  # LogDataDeg.soc_log, per EV contiguous
        self.n = np.zeros(E, dtype=np.int64)
        self.soh = np.ones((E, N)) * self.init_soh  # episode.soh (the env side)

    def reset(self, envs, soc_deg):
        """reset() of `envs`: the log restarts with the reset sample `soc_deg[envs]` (:338-339, :417-418), SoH = init_soh (:345)."""
        envs = np.flatnonzero(envs) if np.asarray(envs).dtype == bool else np.asarray(envs)
        self.n[envs] = 0
        self.soh[envs] = 1.0 * self.init_soh
        self._append(envs, soc_deg)

    def _append(self, envs, soc_deg):
        need = int(self.n[envs].max(initial=0)) + 1
        if need > self.log.shape[2]:  # past done (no auto-reset) the log grows without bound, as in the reference
            grown = np.zeros((self.E, self.N, max(need, 2 * self.log.shape[2])))
            grown[:, :, :self.log.shape[2]] = self.log
            self.log = grown
        self.log[envs[:, None], np.arange(self.N)[None, :], self.n[envs][:, None]] = soc_deg[envs]
        self.n[envs] += 1

    def step(self, envs, soc_deg, at_deg_row):
        """One step of `envs`: append the sample `soc_deg[envs]`, run the model where `at_deg_row[envs]`.  Returns the envs
        evaluated."""
        envs = np.flatnonzero(envs) if np.asarray(envs).dtype == bool else np.asarray(envs)
        self._append(envs, soc_deg)
        ev = envs[np.asarray(at_deg_row)[envs]]
        if ev.size == 0:
            return ev
        N = self.N
        rows = (ev[:, None] * N + np.arange(N)[None, :]).ravel()
        if self.deg == "rainflow":
            S = int(self.n[ev].max())
            series = np.ascontiguousarray(self.log[ev, :, :S]).reshape(-1, S)
            d = self.model.evaluate(rows, series, np.repeat(self.n[ev], N), self.dt)
        else:
            k = self.n[ev]
            old = self.log[ev[:, None], np.arange(N)[None, :], (k - 2)[:, None]].ravel()
            new = self.log[ev[:, None], np.arange(N)[None, :], (k - 1)[:, None]].ravel()
            d = self.model.evaluate(rows, old, new, self.dt)
        self.soh[ev] = self.soh[ev] - d.reshape(-1, N)  # :671
        return ev

    def get(self, name):
        m = self.model
        if name == "soh":
            return self.soh
        if name == "error_bits":
            return np.bitwise_or.reduce(m.err.reshape(self.E, self.N), axis=1)
        v = {"rf_len": getattr(m, "rf_len", None), "fd_cyc": getattr(m, "fd_cyc", None), "fd_cal": getattr(m, "fd_cal", None),
             "sei_l": getattr(m, "l", None), "model_soh": m.soh}[name]
        return v.reshape(self.E, self.N)


BOOK = ("rf_len", "fd_cyc", "fd_cal", "sei_l")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - b) / np.abs(b)
    return np.where(a == b, 0.0, r)


def book_mismatch(a: dict, b: dict, rtol=1e-8):
    """[..., N] EVs whose bookkeeping differs: rainflow_length unequal or fd_cyc / fd_cal / l beyond `rtol`."""
    off = np.asarray(a["rf_len"]) != np.asarray(b["rf_len"])
    for f in BOOK[1:]:
        off |= ~(rel(a[f], b[f]) <= rtol)
    return off


# ---------------------------------------------------------------------------------------------------------------------------
# attribution of an EV whose bookkeeping differs between the kernels and the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def rerun_one_env(engine, tables, actions, steps: int, reset_after, N: int):
    """Step a ONE-env engine (FleetBatch through its stream launches, or OracleBatch; auto_reset = 0) `steps` times with
    `actions(k)` -> [1, N] and reset it after step k where `reset_after(k, done)`.  Returns the episodes seen, each a dict with
    `samples` [n, N] (the reset sample and one per step, the finishing step's included) and `deg`: per degradation row the
    number of samples logged and the engine's bookkeeping {field: [N]} there."""
    engine.reset()
    eps = [dict(samples=[engine.get("soc_deg")[0].copy()], deg=[])]
    for k in range(steps):
        _, _, done, _ = engine.step(actions(k))
        ep = eps[-1]
        ep["samples"].append(engine.get("soc_deg")[0].copy())
        if deg_rows(tables, engine.get("time_idx"))[0]:
            ep["deg"].append((len(ep["samples"]), {f: engine.get(f)[0].copy() for f in BOOK}, int(engine.get("error_bits")[0])))
        if reset_after(k, bool(done[0])):
            engine.reset()
            eps.append(dict(samples=[engine.get("soc_deg")[0].copy()], deg=[]))
    for ep in eps:
        ep["samples"] = np.asarray(ep["samples"])
    return eps


def model_over_episodes(eps, c: int, *, init_soh: float, temp: float, dt: float):
    """SeiModel of ONE EV (`c`) over the episodes of rerun_one_env: its bookkeeping at every degradation row, in order."""
    m = SeiModel(1, init_soh, temp)
    out = []
    for ep in eps:
        s = ep["samples"][:, c]
        for n, _, _ in ep["deg"]:
            m.evaluate([0], s[None, :n], [n], dt)
            out.append({"rf_len": m.rf_len[0], "fd_cyc": m.fd_cyc[0], "fd_cal": m.fd_cal[0], "sei_l": m.l[0]})
    return out


def rainflow_decisions(s):
    """The decisions rainflow.extract_cycles (3.2.0, the C restatement in oracle/fleet_oracle.c) takes on a series, in
    order: ("skip", i, equal) per sample, ("rev", i, reversal) per slope comparison, ("close", push, closes, X == Y) per
    three-point test.  The fourth field says whether the decision was an exact equality."""
    out = []
    if len(s) < 2:
        return out
    stack, pushes = [], [0]

    def push(x):
        stack.append(x)
        pushes[0] += 1
        while len(stack) >= 3:
            X, Y = abs(stack[-1] - stack[-2]), abs(stack[-2] - stack[-3])
            out.append(("close", pushes[0], not X < Y, X == Y))
            if X < Y:
                break
            if len(stack) == 3:
                stack.pop(0)
            else:
                last = stack.pop(); stack.pop(); stack.pop(); stack.append(last)

    x_last, x = s[0], s[1]
    d_last = x - x_last
    push(x_last)
    x_next = None
    for i in range(2, len(s)):
        x_next = s[i]
        eq = x_next == x
        out.append(("skip", i, eq, eq))
        if eq:
            continue
        d_next = x_next - x
        r = d_last * d_next < 0
        out.append(("rev", i, r, d_last * d_next == 0))
        if r:
            push(x)
        x, d_last = x_next, d_next
    if x_next is not None:
        push(x_next)
    return out


def attribute(eps_gpu, eps_cpu, c: int, *, init_soh: float, temp: float, dt: float, what: str = "") -> dict:
    """Prove that EV `c`'s bookkeeping differs between the two engines only through an exact tie of the reversal extraction:
      1. each engine's bookkeeping equals the model on its OWN samples, at every degradation row (rainflow_length exact, the
         floats 1e-8 for the kernels, 1e-13 for the oracle);
      2. the two series are not identical (identical inputs with a different count would be a counting bug);
      3. up to the first degradation row where the bookkeeping differs, the samples agree to <= 1e-12 relative (floor 1e-3);
      4. the first rainflow decision that differs is an exact equality in one series and not in the other.
    Returns a short record for the test's report."""
    assert [len(e["deg"]) for e in eps_gpu] == [len(e["deg"]) for e in eps_cpu], f"{what}: degradation rows differ"
    res = {}
    for name, eps, tol in (("gpu", eps_gpu, 1e-8), ("cpu", eps_cpu, 1e-13)):
        mod = model_over_episodes(eps, c, init_soh=init_soh, temp=temp, dt=dt)
        got = [b for ep in eps for _, b, _ in ep["deg"]]
        for j, (m, g) in enumerate(zip(mod, got)):
            assert g["rf_len"][c] == m["rf_len"], f"{what}: {name} rainflow_length {g['rf_len'][c]} vs model {m['rf_len']} at degradation row {j}"
            for f in BOOK[1:]:
                assert rel(g[f][c], m[f]) <= tol, f"{what}: {name} {f} {g[f][c]!r} vs model {m[f]!r} at degradation row {j}"
        res[name] = mod
    first = next((j for j, (a, b) in enumerate(zip(res["gpu"], res["cpu"]))
                  if a["rf_len"] != b["rf_len"] or not rel(a["fd_cyc"], b["fd_cyc"]) <= 1e-8), None)
    assert first is not None, f"{what}: the bookkeeping of the re-run agrees: the difference did not reproduce"
    # the samples up to that degradation row, episode by episode
    prefix_g, prefix_c, j = [], [], 0
    for eg, ec in zip(eps_gpu, eps_cpu):
        for (n, _, _) in eg["deg"]:
            if j == first:
                prefix_g.append(eg["samples"][:n, c]); prefix_c.append(ec["samples"][:n, c])
                break
            j += 1
        else:
            prefix_g.append(eg["samples"][:, c]); prefix_c.append(ec["samples"][:len(eg["samples"]), c])
            continue
        break
    sg, sc = np.concatenate(prefix_g), np.concatenate(prefix_c)
    assert sg.shape == sc.shape, what
    assert not np.array_equal(sg, sc), f"{what}: identical samples, different rainflow count: a counting bug"
    worst = float(np.max(np.abs(sg - sc) / np.maximum(np.abs(sc), 1e-3)))  # (a floor: a drained battery's 0 vs a 1e-17 residue)
    assert worst <= 1e-12, f"{what}: samples differ by {worst:.3g} relative before the bookkeeping does"
    for pg, pc in zip(prefix_g, prefix_c):
        dg, dc = rainflow_decisions(list(pg)), rainflow_decisions(list(pc))
        k = next((k for k, (a, b) in enumerate(zip(dg, dc)) if a[:3] != b[:3]), None)
        if k is None:
            assert len(dg) == len(dc), what
            continue
        a, b = dg[k], dc[k]
        assert a[0] in ("skip", "close") and a[3] != b[3], \
            f"{what}: the first rainflow decision that differs is no exact tie: kernels {a}, oracle {b}"
        return dict(first_row=first, decision=a[0], tie_in="kernels" if a[3] else "oracle", sample_rel=worst)
    raise AssertionError(f"{what}: the samples differ but no rainflow decision does")


# ---------------------------------------------------------------------------------------------------------------------------
# a whole run: an engine stepped, its own samples recounted, its bookkeeping checked at every degradation row
# ---------------------------------------------------------------------------------------------------------------------------
BOOK_RTOL = 1e-8  # fd_cyc / fd_cal / l: the bound fleet_selftest_stress asserts for the kernels' stress approximation
SOH_ATOL = 1e-10


class RecountCheck:
    """Feeds `recount` the samples an engine logged and compares the engine's state with it: after every step the env-side SoH
    of every EV (atol SOH_ATOL) and the error bits; on every degradation row of an env ALL its EVs' rainflow_length (exact) and
    fd_cyc / fd_cal / l (rtol `rtol`).  Keeps the worst relative error per field."""

    def __init__(self, recount: Recount, tables, rtol: float = BOOK_RTOL, soh_atol: float = SOH_ATOL):
        self.rc, self.tables, self.rtol, self.soh_atol = recount, tables, rtol, soh_atol
        self.worst = {f: 0.0 for f in BOOK[1:] + ("soh",)}
        self.deg_rows = 0  # env-level degradation rows checked
        self.ev_steps = 0

    def reset(self, get, envs=None):
        m = np.ones(self.rc.E, bool) if envs is None else np.asarray(envs, bool)
        self.rc.reset(m, get("soc_deg"))

    def step(self, get, what: str, stepped=None, finished=None):
        """After one step of the engine.  `stepped`: envs that took the step (default all); `finished`: envs whose episode ended
        and that were reset in place (auto-reset: their visible sample is the next episode's reset sample -- the caller
        guarantees that the finishing row was no degradation row)."""
        E, N = self.rc.E, self.rc.N
        stepped = np.ones(E, bool) if stepped is None else np.asarray(stepped, bool)
        fin = np.zeros(E, bool) if finished is None else np.asarray(finished, bool)
        soc_deg, t = get("soc_deg"), get("time_idx")
        if fin.any():
            self.rc.reset(stepped & fin, soc_deg)
        at = deg_rows(self.tables, t) & stepped & ~fin
        ev = self.rc.step(stepped & ~fin, soc_deg, at)
        self.ev_steps += int(stepped.sum()) * N
        soh = get("soh")
        d = np.abs(soh - self.rc.soh)
        self.worst["soh"] = max(self.worst["soh"], float(d.max(initial=0.0)))
        if not (d <= self.soh_atol).all():
            e, c = np.argwhere(~(d <= self.soh_atol))[0]
            raise AssertionError(f"soh, {what}: env {e} EV {c}: engine {soh[e, c]!r}, recount {self.rc.soh[e, c]!r}")
        bits, want = get("error_bits"), self.rc.get("error_bits")
        if not np.array_equal(bits, want):
            e = int(np.flatnonzero(bits != want)[0])
            raise AssertionError(f"error bits, {what}: env {e}: engine {bits[e]:#x}, recount {want[e]:#x}")
        if ev.size == 0 or self.rc.deg != "rainflow":
            return ev
        self.deg_rows += ev.size
        got_len, want_len = get("rf_len")[ev], self.rc.get("rf_len")[ev]
        if not np.array_equal(got_len, want_len):
            k, c = np.argwhere(got_len != want_len)[0]
            raise AssertionError(f"rainflow_length, {what}: env {ev[k]} EV {c}: engine {got_len[k, c]}, recount {int(want_len[k, c])}")
        for f in BOOK[1:]:
            g, w = get(f)[ev], self.rc.get(f)[ev]
            r = rel(g, w)
            self.worst[f] = max(self.worst[f], float(r.max(initial=0.0)))
            if not (r <= self.rtol).all():
                k, c = np.argwhere(~(r <= self.rtol))[0]
                raise AssertionError(f"{f}, {what}: env {ev[k]} EV {c}: engine {g[k, c]!r}, recount {w[k, c]!r} ({r[k, c]:.3g} rel)")
        return ev

    def report(self, name: str) -> str:
        w = ", ".join(f"{f} {v:.3g}" for f, v in self.worst.items())
        return f"{name}: {self.deg_rows} env degradation rows, {self.ev_steps} EV-steps; worst relative error {w} (soh: absolute)"


def starts_avoiding_deg_finish(rng, tables, lo: int, hi: int, episode_steps: int, shape):
    """Start rows in [lo, hi] whose episode does not finish on a 14:45 row (with auto-reset the finishing step's own sample is
    replaced by the next episode's reset sample before the host can read it; a finishing row that is no degradation row makes
    that sample unneeded: the count stops at the episode's last degradation row, `rf_until`, and reset() clears the log)."""
    s = rng.integers(lo, hi + 1, size=shape)
    bad = deg_rows(tables, s + episode_steps)
    s[bad] = np.where(s[bad] + 1 <= hi, s[bad] + 1, s[bad] - 1)
    assert not deg_rows(tables, s + episode_steps).any()
    return s.astype(np.int32)


def attribute_by_rerun(make_gpu, make_cpu, tables, actions, steps: int, reset_after, e: int, evs, *, init_soh, temp, dt,
                       final_gpu=None, what=""):
    """Re-run env `e` alone on both engines (`make_gpu()` / `make_cpu()`: one-env handles, auto_reset = 0, the env's own
    start rows) and attribute() each EV in `evs`.  `final_gpu` {field: [N]}: the batch's final state of env e, which the
    one-env re-run through stream launches must reproduce bit for bit.  Returns {EV: attribute() record}."""
    g, c = make_gpu(), make_cpu()
    try:
        N = len(c.get("soc_deg")[0])
        eps_g = rerun_one_env(g, tables, actions, steps, reset_after, N)
        eps_c = rerun_one_env(c, tables, actions, steps, reset_after, N)
        if final_gpu is not None:
            for f, v in final_gpu.items():
                np.testing.assert_array_equal(g.get(f)[0], v, err_msg=f"{what}: the one-env re-run of env {e} does not reproduce {f}")
        return {int(ev): attribute(eps_g, eps_c, int(ev), init_soh=init_soh, temp=temp, dt=dt, what=f"{what}, env {e} EV {ev}")
                for ev in evs}
    finally:
        g.close(); c.close()
