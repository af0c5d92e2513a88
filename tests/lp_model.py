"""Restatement of the linear-optimisation benchmark's model for ONE EV (the reference's
benchmarking/linear_optimization.py:55-247), independent of the HIP planner:

  * `build_lp` / `solve_scipy`: the model as a scipy (HiGHS) LP or MILP, variables c, d, u, b per row and soc per node;
  * `solve_numpy`: a slow exact solver of the LP relaxation: a forward DP over each parking session with the value function
    held as breakpoints, and a backward recovery of the SOC trajectory;
  * `realise` / `check_tape`: decision 2's one-sided realisation of a SOC trajectory and a feasibility check of an action tape
    against every MILP constraint;
  * `relaxed_cost_of_trajectory`: what a SOC trajectory costs in the relaxation (the bound, if and only if it is optimal);
  * `adversarial_columns` / `adversarial_tables` / `instances_of`: table columns in blocks of named families (grid-bound rows,
    prices <= 0, PV shares up to above the charger's power, returns outside [0, target]) for the product, and the instances of
    every (env, EV) of a batch on them; `coverage` / `assert_covered`: what an instance set exercises, from the model alone.

An instance is a dict: there [H] bool, sor [H] SOC_on_return, price [H] EUR/kWh, tariff [H] EUR/kWh (after the feed-in
deduction), pv [H], load [H] kW, and the scalars P, cap, eta_c, eta_d, dt, target, p_trafo, N, soc0.
"""
from __future__ import annotations

import numpy as np

UNREACHABLE, NEG_RETURN, ABOVE_TARGET, GRID_NEGATIVE = 1, 2, 4, 8


def _fixed(v, target):
    if v < 0:
        return 0.0, NEG_RETURN
    if v > target:
        return float(target), ABOVE_TARGET
    return float(v), 0


def headroom(inst):
    """Grid headroom per row, p_trafo - load + pv, taken as 0 where negative."""
    G = inst["p_trafo"] - np.asarray(inst["load"], float) + np.asarray(inst["pv"], float)
    return np.maximum(G, 0.0), int((G < 0).any()) * GRID_NEGATIVE


def row_kind(inst, i):
    """'away', 'dep' (present, away on the next row, not the last row) or 'dyn' (dynamics to the next node)."""
    th, H = inst["there"], len(inst["there"])
    if not th[i]:
        return "away"
    if i < H - 1 and not th[i + 1]:
        return "dep"
    return "dyn"


def sessions(inst):
    """Decisions 1 and 3: fixed start SOC of every session, departure targets lowered where unreachable, status bits."""
    H, target = len(inst["there"]), inst["target"]
    G, bits = headroom(inst)
    start, tau = {}, {}
    m = None
    for i in range(H):
        k = row_kind(inst, i)
        if inst["there"][i] and (i == 0 or not inst["there"][i - 1]):
            v, b = _fixed(inst["soc0"] if i == 0 else inst["sor"][i], target)
            start[i], m = v, v
            bits |= b
        if k == "dep":
            tau[i] = min(target, m)
            if m < target:
                bits |= UNREACHABLE
        elif k == "dyn":
            m = min(target, m + inst["eta_c"] * min(inst["P"], G[i]) * inst["dt"] / inst["cap"])
    return start, tau, bits


# ---- scipy (HiGHS) -------------------------------------------------------------------------------------------------
def build_lp(inst, binary: bool):
    """(c, A_ub, b_ub, A_eq, b_eq, bounds, integrality) over x = [c(H), d(H), u(H), b(H), soc(H+1)]."""
    H = len(inst["there"])
    P, dt, cap, ec, target = inst["P"], inst["dt"], inst["cap"], inst["eta_c"], inst["target"]
    G, _ = headroom(inst)
    start, tau, _ = sessions(inst)
    nv = 4 * H + H + 1
    C, D, U, B, S = 0, H, 2 * H, 3 * H, 4 * H
    obj = np.zeros(nv)
    price, tariff = np.asarray(inst["price"], float), np.asarray(inst["tariff"], float)
    obj[C:C + H] = dt * price * P
    obj[U:U + H] = -dt * price
    obj[D:D + H] = dt * tariff * inst["eta_d"] * P
    bounds = []
    for i in range(H):
        bounds.append((0.0, 1.0 if inst["there"][i] else 0.0))
    for i in range(H):
        bounds.append((-1.0 if inst["there"][i] else 0.0, 0.0))
    for i in range(H):
        bounds.append((0.0, max(float(inst["pv"][i]), 0.0) / inst["N"]))
    bounds += [(0.0, 1.0)] * H
    bounds += [(0.0, target)] * (H + 1)
    aub, bub, aeq, beq = [], [], [], []

    def row(pairs):
        r = np.zeros(nv)
        for j, v in pairs:
            r[j] += v
        return r

    for i in range(H):
        aub.append(row([(U + i, 1.0), (C + i, -P)]))
        bub.append(0.0)
        aub.append(row([(C + i, P), (D + i, P)]))
        bub.append(G[i])
        aub.append(row([(C + i, 1.0), (B + i, -1.0)]))  # c <= b
        bub.append(0.0)
        aub.append(row([(B + i, 1.0), (D + i, -1.0)]))  # d >= b - 1
        bub.append(1.0)
    for i, v in start.items():
        aeq.append(row([(S + i, 1.0)]))
        beq.append(v)
    for i in range(H):
        k = row_kind(inst, i)
        dyn = [(S + i + 1, 1.0), (S + i, -1.0), (C + i, -ec * P * dt / cap), (D + i, -P * dt / cap)]
        if i == H - 1:
            aeq.append(row(dyn))
            beq.append(0.0)
        elif k == "dyn":
            aeq.append(row(dyn))
            beq.append(0.0)
        elif k == "dep":
            for pairs, v in (([(S + i, 1.0)], tau[i]), ([(S + i + 1, 1.0)], 0.0), ([(D + i, 1.0)], 0.0)):
                aeq.append(row(pairs))
                beq.append(v)
        else:
            aeq.append(row([(S + i, 1.0)]))
            beq.append(0.0)
    if not inst["there"][0]:
        aeq.append(row([(S, 1.0)]))
        beq.append(0.0)
    integrality = np.zeros(nv)
    if binary:
        integrality[B:B + H] = 1
    return obj, np.array(aub), np.array(bub), np.array(aeq), np.array(beq), bounds, integrality


def solve_scipy(inst, binary: bool = False):
    """Optimum of the relaxed (binary=False, linprog) or the binary model (binary=True, milp): (objective, soc [H+1])."""
    from scipy.optimize import Bounds, LinearConstraint, linprog, milp

    obj, aub, bub, aeq, beq, bounds, integ = build_lp(inst, binary)
    H = len(inst["there"])
    if not binary:
        res = linprog(obj, A_ub=aub, b_ub=bub, A_eq=aeq, b_eq=beq, bounds=bounds, method="highs",
                      options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
        assert res.status == 0, res.message
        return float(res.fun), res.x[4 * H:]
    lb, ub = np.array([b[0] for b in bounds]), np.array([b[1] for b in bounds])
    cons = [LinearConstraint(aub, -np.inf, bub), LinearConstraint(aeq, beq, beq)]
    res = milp(obj, constraints=cons, bounds=Bounds(lb, ub), integrality=integ, options={"mip_rel_gap": 1e-12})
    assert res.status == 0, res.message
    return float(res.fun), res.x[4 * H:]


# ---- slow exact NumPy solver of the relaxation ----------------------------------------------------------------------
def row_cost(inst, i, G):
    """The relaxed row cost r_i(delta) as breakpoints (xs ascending, ys): minimum of the row's objective over c, d, u (b relaxed)
    at a given SOC change.  Lower convex hull of the row polygon's vertices, the polygon split where the charge cost bends."""
    P, dt, cap, ec = inst["P"], inst["dt"], inst["cap"], inst["eta_c"]
    pr, g, s = float(inst["price"][i]), float(inst["tariff"][i]) * inst["eta_d"], max(float(inst["pv"][i]), 0.0) / inst["N"]
    verts = [(0.0, 0.0), (0.0, P), (min(P, G), 0.0)]
    if G < P:
        verts.append(((P + G) / 2, (P - G) / 2))
    if pr > 0:
        verts += [(s, 0.0), (s, P - s), (s, s - G)]
    pts = set()
    for x, y in verts:
        if x < -1e-15 or y < -1e-15 or x + y > P * (1 + 1e-15) or x - y > G + 1e-12:
            continue
        cx = pr * max(0.0, x - s) if pr > 0 else pr * x
        pts.add(((ec * x - y) * dt / cap, dt * (cx - g * y)))
    pts = sorted(pts)
    hull = []
    for p in pts:
        if hull and abs(p[0] - hull[-1][0]) <= 1e-300:
            continue
        while len(hull) >= 2 and (hull[-1][0] - hull[-2][0]) * (p[1] - hull[-2][1]) - (hull[-1][1] - hull[-2][1]) * (p[0] - hull[-2][0]) <= 0:
            hull.pop()
        hull.append(p)
    return np.array([h[0] for h in hull]), np.array([h[1] for h in hull])


def dep_action(inst, i, G):
    return min(inst["P"], G) / inst["P"] if inst["price"][i] < 0 else 0.0


def action_cost(inst, i, a):
    P, dt = inst["P"], inst["dt"]
    pr, s = float(inst["price"][i]), max(float(inst["pv"][i]), 0.0) / inst["N"]
    x = a * P
    if a > 0:
        return dt * (pr * max(0.0, x - s) if pr > 0 else pr * x)
    return dt * float(inst["tariff"][i]) * inst["eta_d"] * x


def solve_numpy(inst):
    """(bound, soc [H+1]) of the LP relaxation.  Forward DP per session: V_{i+1} = (V_i inf-conv r_i) restricted to [0, target],
    V as (x0, y0, slopes, lengths) with slopes ascending; every merged list is kept to recover the trajectory backwards."""
    H, target = len(inst["there"]), inst["target"]
    G, _ = headroom(inst)
    start, tau, _ = sessions(inst)
    soc = np.zeros(H + 1)
    total = 0.0
    i = 0
    while i < H:
        if not inst["there"][i]:
            i += 1
            continue
        x0, y0, sl, ln = start[i], 0.0, np.zeros(0), np.zeros(0)
        hist = []
        j = i
        while True:
            k = row_kind(inst, j)
            if k == "dep":
                break
            bx, by = row_cost(inst, j, G[j])
            rs, rl = np.diff(by) / np.diff(bx), np.diff(bx)
            nx0, ny0 = x0 + bx[0], y0 + by[0]
            ms = np.concatenate([sl, rs])
            ml = np.concatenate([ln, rl])
            src = np.concatenate([np.zeros(len(sl), int), np.ones(len(rs), int)])
            o = np.argsort(ms, kind="stable")
            ms, ml, src = ms[o], ml[o], src[o]
            hist.append((nx0, ms, ml, src, x0, bx[0]))
            # restrict to [0, target]
            cum = np.concatenate([[0.0], np.cumsum(ml)])
            lo, hi = max(0.0, nx0), min(target, nx0 + cum[-1])
            x0, y0 = lo, _pwl_eval(nx0, ny0, ms, ml, lo)
            a_, b_ = lo - nx0, hi - nx0
            nsl, nln = [], []
            for s_, l_, c0 in zip(ms, ml, cum[:-1]):
                seg = min(c0 + l_, b_) - max(c0, a_)
                if seg > 0:
                    nsl.append(s_)
                    nln.append(seg)
            sl, ln = np.array(nsl), np.array(nln)
            j += 1
            if j == H:
                break
        if j < H:  # departure row j: SOC fixed at tau[j]
            end = tau[j]
            total += _pwl_eval(x0, y0, sl, ln, end) + action_cost(inst, j, dep_action(inst, j, G[j]))
        else:  # open end: the cheapest SOC
            cands = x0 + np.concatenate([[0.0], np.cumsum(ln)])
            vals = [_pwl_eval(x0, y0, sl, ln, c) for c in cands]
            end = float(cands[int(np.argmin(vals))])
            total += min(vals)
        # backward recovery through the merged lists
        s_next = end
        soc[j] = end
        for r in range(len(hist) - 1, -1, -1):
            nx0, ms, ml, src, px0, b0 = hist[r]
            off = min(max(s_next - nx0, 0.0), float(ml.sum()))
            used = np.zeros(2)
            for s_, l_, w in zip(ms, ml, src):
                take = min(l_, off)
                used[w] += take
                off -= take
                if off <= 0:
                    break
            s_prev = px0 + used[0]
            soc[i + r] = s_prev
            s_next = s_prev
        soc[i] = start[i]
        i = j + 1
    return total, soc


def _pwl_eval(x0, y0, sl, ln, x):
    v, pos = y0, x0
    for s_, l_ in zip(sl, ln):
        if pos >= x:
            break
        take = min(l_, x - pos)
        v += s_ * take
        pos += take
    return v


# ---- decision 2: realisation and feasibility -------------------------------------------------------------------------
def realise(inst, soc):
    """One-sided actions [H] that keep the SOC trajectory `soc` [H+1], and their MILP objective."""
    H = len(inst["there"])
    G, _ = headroom(inst)
    k = inst["P"] * inst["dt"] / inst["cap"]
    a = np.zeros(H)
    for i in range(H):
        kind = row_kind(inst, i)
        if kind == "away":
            continue
        if kind == "dep":
            a[i] = dep_action(inst, i, G[i])
            continue
        d = soc[i + 1] - soc[i]
        a[i] = d / (inst["eta_c"] * k) if d > 0 else d / k
    a = np.clip(a, -1.0, 1.0)
    return a, float(sum(action_cost(inst, i, a[i]) for i in range(H)))


def tape_soc(inst, a):
    """The SOC trajectory the model's rules give an action tape (fixed rows from the sessions, dynamics elsewhere)."""
    H = len(inst["there"])
    start, tau, _ = sessions(inst)
    k = inst["P"] * inst["dt"] / inst["cap"]
    soc = np.zeros(H + 1)
    s = start.get(0, 0.0)
    for i in range(H):
        if i in start:
            s = start[i]
        soc[i] = s if inst["there"][i] else 0.0
        kind = row_kind(inst, i)
        if kind == "dyn":
            c, d = max(a[i], 0.0), min(a[i], 0.0)
            s = s + k * (inst["eta_c"] * c + d)
        else:
            s = 0.0
    soc[H] = s
    return soc


def check_tape(inst, a, tol=1e-9):
    """Assert that the tape `a` [H] (c = max(a, 0), d = min(a, 0), b = [a > 0]) satisfies every MILP constraint; returns the
    SOC trajectory it produces."""
    H = len(inst["there"])
    G, _ = headroom(inst)
    start, tau, _ = sessions(inst)
    soc = tape_soc(inst, a)
    for i in range(H):
        c, d = max(a[i], 0.0), min(a[i], 0.0)
        assert -1 - tol <= a[i] <= 1 + tol, (i, a[i])
        if not inst["there"][i]:
            assert a[i] == 0.0, (i, a[i])
        assert (c + d) * inst["P"] <= G[i] + tol, (i, a[i], G[i])
        kind = row_kind(inst, i)
        if kind == "dep":
            assert d == 0.0 and abs(soc[i] - tau[i]) <= tol, (i, soc[i], tau[i])
        if kind == "away" and i < H - 1:
            assert soc[i] == 0.0
    assert np.all(soc >= -tol) and np.all(soc <= inst["target"] + tol), soc
    return soc


def random_instance(rng, H, *, pv=True, gap_zero=False, N=3):
    there = np.ones(H, bool)
    i = int(rng.integers(0, 3))
    while i < H:  # alternating parking / driving blocks
        i += int(rng.integers(2, 8))
        j = i + int(rng.integers(1, 4))
        there[i:j] = False
        i = j
    if rng.random() < 0.3:
        there[0] = False
    price = rng.normal(0.08, 0.06, H)
    tariff = rng.normal(0.05, 0.03, H)
    eta_c, eta_d = 0.91, 0.91
    if gap_zero:
        tariff = np.minimum(tariff, price / eta_c / eta_d - 1e-3)
    load = rng.uniform(5, 20, H)
    pvv = np.where(rng.random(H) < 0.6, rng.uniform(0, 40, H), 0.0) if pv else np.zeros(H)
    return dict(there=there, sor=rng.uniform(-0.05, 0.6, H), price=price, tariff=tariff, pv=pvv, load=load, P=11.0, cap=60.0,
                eta_c=eta_c, eta_d=eta_d, dt=0.25, target=0.85, p_trafo=float(rng.choice([25.0, 40.0])), N=N,
                soc0=float(rng.uniform(0.1, 0.8)))


# ---- what a trajectory costs in the relaxation ---------------------------------------------------------------------------
def relaxed_cost_of_trajectory(inst, soc):
    """Cost of the SOC trajectory `soc` [H+1] in the relaxation: the sum over the dynamic rows of r_i(soc[i+1] - soc[i]) (linear
    interpolation on `row_cost`'s breakpoints; the step must lie in [b_0, b_m] within 1e-12) plus the departure rows' action
    costs.  For an optimal trajectory of the relaxation this is the bound; for any other feasible one it is dearer."""
    G, _ = headroom(inst)
    total = 0.0
    for i in range(len(inst["there"])):
        k = row_kind(inst, i)
        if k == "dep":
            total += action_cost(inst, i, dep_action(inst, i, G[i]))
        elif k == "dyn":
            bx, by = row_cost(inst, i, G[i])
            d = float(soc[i + 1]) - float(soc[i])
            assert bx[0] - 1e-12 <= d <= bx[-1] + 1e-12, (i, d, bx)
            total += float(np.interp(d, bx, by))
    return total


# ---- adversarial per-row series, as table columns -------------------------------------------------------------------------
FAMILIES = ("hourly", "negative", "arbitrage", "grid", "pv", "returns", "gap_zero")
BLOCK = 8 * 96  # rows per family block of an adversarial table: a 7-day horizon that starts on a block's first day stays inside


def family_of_row(t):
    return FAMILIES[(int(t) // BLOCK) % len(FAMILIES)]


def block_start(family, k=0):
    """First row of the k-th block of `family` in an adversarial table."""
    return (FAMILIES.index(family) + k * len(FAMILIES)) * BLOCK


def adversarial_columns(T, N, *, P, grid, eta_c=0.91, eta_d=0.91, fixed_markup=10.0, variable_multiplier=1.5,
                        feed_in_deduction=0.25, seed=0):
    """Table columns `delu`, `tariff` [EUR/MWh], `load`, `pv` [kW] (each [T]) and `soc_on_return` [T, N] for a fleet of N EVs
    with chargers of P kW behind a grid connection of `grid` kW, in blocks of BLOCK rows that cycle through FAMILIES:

      hourly     four equal rows per hour from a handful of price levels (equal slopes coalesce, ties everywhere), no PV, G >= P
      negative   hourly prices around 0: negative, positive and exactly 0; the tariff follows the spot price
      arbitrage  a price per row, the tariff on both sides of price / (eta_c eta_d): discharging pays on some rows
      grid       load (and on half the rows PV) such that the headroom G = grid - load + pv crosses P and 0
      pv         the PV share s = pv / N from 0 to above P, G from below 0 to above P: s crosses G and P on either side of G < P
      returns    SOC_on_return from below 0 to above any target, prices, G and s as in "pv" but milder
      gap_zero   no PV, tariff' eta_d <= price / eta_c on every row (G crosses P, prices of both signs): relaxation = MILP

    Prices are what the kernel derives: price = (delu + fixed_markup) variable_multiplier / 1000, tariff' = tariff (1 -
    feed_in_deduction) / 1000.  delu and tariff have two decimals, like the shipped data, so a price is exactly 0 (delu =
    -fixed_markup) or at least 1e-5 away from it, in whichever order the factors are applied.  load >= 0 needs grid >= 2 P."""
    assert grid >= 2 * P
    rng = np.random.default_rng([seed, N])
    nb = -(-T // BLOCK)
    k_price = variable_multiplier / 1000.0
    k_tar = (1 - feed_in_deduction) / 1000.0
    delu, tariff, load, pv = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    sor = rng.uniform(0.0, 0.8, size=(T, N))
    sor = sor[(np.arange(T) // 8) * 8]  # a value holds for two hours: the rows of one arrival's neighbourhood share it

    def hourly(a, n):
        return np.repeat(a, 4)[:n]

    for b in range(nb):
        r = slice(b * BLOCK, min(T, (b + 1) * BLOCK))
        n = r.stop - r.start
        nh = -(-n // 4)
        fam = FAMILIES[b % len(FAMILIES)]
        G = np.full(n, float(grid))
        s = np.zeros(n)
        if fam == "hourly":
            d = hourly(rng.choice([18.0, 22.0, 22.0, 25.5, 31.0], size=nh), n)
            f = np.full(n, 40.0)
        elif fam == "negative":
            d = hourly(np.round(rng.normal(-10.0, 12.0, nh), 2), n)
            d[hourly(rng.random(nh) < 0.2, n)] = -fixed_markup
            f = d.copy()
        elif fam == "arbitrage":
            d = np.round(rng.normal(25.0, 15.0, n), 2)
            f = np.round((d + fixed_markup) * k_price / (eta_c * eta_d) / k_tar * rng.uniform(0.5, 1.6, n), 2)
        elif fam == "grid":
            d = hourly(np.round(rng.normal(20.0, 25.0, nh), 2), n)
            f = np.round(rng.normal(30.0, 20.0, n), 2)
            G = rng.uniform(-0.4 * P, 2.0 * P, n)
            s = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.3 * P, n), 0.0)
        elif fam == "pv":
            d = hourly(np.round(rng.normal(25.0, 20.0, nh), 2), n)
            f = np.round(rng.normal(45.0, 25.0, n), 2)
            G = rng.uniform(-0.2 * P, 2.0 * P, n)
            s = np.where(rng.random(n) < 0.85, rng.uniform(0.0, 1.6 * P, n), 0.0)
        elif fam == "returns":
            d = hourly(np.round(rng.normal(25.0, 20.0, nh), 2), n)
            f = np.round(rng.normal(35.0, 20.0, n), 2)
            G = rng.uniform(0.3 * P, 2.0 * P, n)
            s = np.where(rng.random(n) < 0.4, rng.uniform(0.0, 1.2 * P, n), 0.0)
            sor[r] = rng.uniform(-0.15, 1.1, size=(nh, N))[np.arange(n) // 4]
        else:  # gap_zero
            d = hourly(np.round(rng.normal(12.0, 25.0, nh), 2), n)
            f = np.floor(((d + fixed_markup) * k_price / (eta_c * eta_d) / k_tar - rng.uniform(0.5, 30.0, n)) * 100) / 100
            G = rng.uniform(-0.2 * P, 2.0 * P, n)
        delu[r], tariff[r] = d, f
        pv[r] = s * N
        load[r] = grid + pv[r] - G
    assert (load >= 0).all()
    return dict(delu=delu, tariff=tariff, load=load, pv=pv, soc_on_return=sor)


def adversarial_tables(use_case, N, *, P, grid, seed=0, **column_kw):
    """A `FleetTables` for the product: `synth_tables(use_case, N)` keeps its schedule columns (`there`, `time_left`, ...
    consistent with each other), and `delu`, `tariff`, `load`, `pv` and `soc_on_return` are `adversarial_columns`'."""
    import dataclasses

    from fleetrl_amd.synth import synth_tables

    base = synth_tables(use_case, N, seed=1234 + seed, include_building=True, include_pv=True)
    cols = adversarial_columns(base.T, N, P=P, grid=grid, seed=seed, **column_kw)
    return dataclasses.replace(base, meta=dict(base.meta), **cols)


def instances_of(tables, p, t0, soc, H):
    """The instance of every (env, EV) that plans H rows from row t0[e] with the SOCs soc[e, c], on `tables` under the
    parameters `p` (a `FleetParams`, or anything with its field names): {(e, c): instance}.  The EVs of an env share their
    per-row series (the same arrays)."""
    there, sor = np.asarray(tables.there) != 0, np.asarray(tables.soc_on_return, float)
    delu, tariff = np.asarray(tables.delu, float), np.asarray(tables.tariff, float)
    load = np.asarray(tables.load, float) if p.include_building else np.zeros(tables.T)
    pv = np.asarray(tables.pv, float) if p.include_pv else np.zeros(tables.T)
    N = there.shape[1]
    out = {}
    for e in range(len(t0)):
        r = slice(int(t0[e]), int(t0[e]) + H)
        price = (delu[r] + p.fixed_markup) * p.variable_multiplier / 1000
        tar = tariff[r] * (1 - p.feed_in_deduction) / 1000
        pv_r, load_r = pv[r], load[r]
        for c in range(N):
            out[e, c] = dict(there=there[r, c], sor=sor[r, c], price=price, tariff=tar, pv=pv_r, load=load_r, P=p.evse_power,
                             cap=p.init_battery_cap, eta_c=p.charging_eff, eta_d=p.discharging_eff, dt=p.dt, target=p.target_soc,
                             p_trafo=p.grid_connection, N=N, soc0=float(soc[e][c]))
    return out


# ---- what an instance set exercises ------------------------------------------------------------------------------------------
ROW_CATEGORIES = ("G<P", "G<0", "price<0", "price==0", "0<s<P", "s>=P", "0<s<G<P", "s>G", "discharging_pays")


def coverage(insts):
    """What the instances exercise, from the model alone: {"rows": dynamic rows of all lanes per ROW_CATEGORIES entry,
    "pieces": {pieces of r_i: dynamic rows}, "bit_set" / "bit_clear": {status bit: lanes}, "away_at_row_0", "present_on_last_row",
    "whole_horizon_session", "start_above_target": lanes, "lanes", "dyn_rows"}.  "s>G" counts the rows on which the hull has the
    (s, s - G) vertex to consider: price > 0, s < P and G < s < (P + G) / 2."""
    rows = dict.fromkeys(ROW_CATEGORIES, 0)
    pieces = {}
    bit_set = dict.fromkeys((UNREACHABLE, NEG_RETURN, ABOVE_TARGET, GRID_NEGATIVE), 0)
    bit_clear = dict(bit_set)
    cov = dict(rows=rows, pieces=pieces, bit_set=bit_set, bit_clear=bit_clear, away_at_row_0=0, present_on_last_row=0,
               whole_horizon_session=0, start_above_target=0, lanes=0, dyn_rows=0)
    per_series = {}
    for inst in insts.values() if isinstance(insts, dict) else insts:
        H, P = len(inst["there"]), inst["P"]
        key = (id(inst["price"]), id(inst["load"]), id(inst["pv"]), inst["N"])
        if key not in per_series:
            Graw = inst["p_trafo"] - np.asarray(inst["load"], float) + np.asarray(inst["pv"], float)
            G = np.maximum(Graw, 0.0)
            s = np.maximum(np.asarray(inst["pv"], float), 0.0) / inst["N"]
            pr, tar = np.asarray(inst["price"], float), np.asarray(inst["tariff"], float)
            cat = {"G<P": Graw < P, "G<0": Graw < 0, "price<0": pr < 0, "price==0": pr == 0, "0<s<P": (s > 0) & (s < P), "s>=P": s >= P,
                   "0<s<G<P": (s > 0) & (s < G) & (G < P), "s>G": (pr > 0) & (s < P) & (s > G) & (s < 0.5 * (P + G)),
                   "discharging_pays": tar * inst["eta_d"] * inst["eta_c"] > pr}
            npieces = np.array([len(row_cost(inst, i, G[i])[0]) - 1 for i in range(H)])
            per_series[key] = (cat, npieces)
        cat, npieces = per_series[key]
        th = np.asarray(inst["there"], bool)
        dyn = th & np.r_[th[1:], True]
        for name in ROW_CATEGORIES:
            rows[name] += int((cat[name] & dyn).sum())
        for m, n in zip(*np.unique(npieces[dyn], return_counts=True)):
            pieces[int(m)] = pieces.get(int(m), 0) + int(n)
        bits = sessions(inst)[2]
        for b in bit_set:
            (bit_set if bits & b else bit_clear)[b] += 1
        cov["away_at_row_0"] += int(not th[0])
        cov["present_on_last_row"] += int(th[-1])
        cov["whole_horizon_session"] += int(th.all())
        cov["start_above_target"] += int(th[0] and inst["soc0"] > inst["target"])
        cov["lanes"] += 1
        cov["dyn_rows"] += int(dyn.sum())
    return cov


def merge_coverage(a, b):
    """Sum of two `coverage` results (a may be None)."""
    if a is None:
        return b
    out = {}
    for k, v in a.items():
        if isinstance(v, dict):
            out[k] = {j: v.get(j, 0) + b[k].get(j, 0) for j in set(v) | set(b[k])}
        else:
            out[k] = v + b[k]
    return out


# ---- the adversarial cases of the GPU suite (tests/test_lp_plan_gpu.py); the CPU suite checks the model and the coverage on them --
EVSE_KW = {"ct": 4.6, "lmd": 11.0, "ut": 22.0}  # evse_max_power of the use cases (fleetrl_amd/config.py `company`)
# (envs, EVs, rows, use case, seed: the first env's family): one lane; horizons of 2 and 3 rows (the kernel's i == H - 1, i < H - 1, i + 1 < H - 1 cases); a
# ragged count of EVs and rows; N = 64 and N > 64; 900 lanes = four workgroups of 256, the last partly filled, at an odd
# horizon; a 7-day episode
ADVERSARIAL_SHAPES = ((1, 1, 1, "ct", 4), (3, 7, 2, "ct", 3), (3, 7, 3, "lmd", 4), (7, 50, 96, "lmd", 0), (5, 64, 192, "ct", 2),
                      (2, 130, 192, "ct", 3), (300, 3, 95, "lmd", 0), (4, 5, 672, "ct", 3))


def grid_kw(use_case):
    """The grid connection of the adversarial cases: 2.5 chargers' worth, so that load and PV decide whether it binds."""
    return 2.5 * EVSE_KW[use_case]


def adversarial_starts(E, H, seed=0):
    """Start rows [E] and family names [E]: env e plans the family FAMILIES[(e + seed) % 7], from a row on the first day of one of
    that family's blocks, so that up to seven days of rows stay inside the block."""
    assert H <= BLOCK - 96
    rng = np.random.default_rng([seed, E, H])
    fam = [FAMILIES[(e + seed) % len(FAMILIES)] for e in range(E)]
    starts = np.array([block_start(f, int(rng.integers(0, 6))) + int(rng.integers(0, 96)) for f in fam], dtype=np.int32)
    return starts, fam


def assert_covered(cov):
    """Every row category, a 4-piece row cost (the most the hull can have, tests/test_lp_model_cpu.py), every status bit set and
    clear, an EV away at row 0 and one present on the last row occur in the instance set that `cov` summarises."""
    for name in ("G<P", "G<0", "price<0", "price==0", "s>=P", "0<s<G<P", "s>G", "0<s<P", "discharging_pays"):
        assert cov["rows"][name] > 0, (name, cov)
    assert all(cov["pieces"].get(m, 0) > 0 for m in (1, 2, 3, 4)), cov["pieces"]
    for b in (UNREACHABLE, NEG_RETURN, ABOVE_TARGET, GRID_NEGATIVE):
        assert cov["bit_set"][b] > 0 and cov["bit_clear"][b] > 0, (b, cov)
    assert cov["away_at_row_0"] > 0 and cov["present_on_last_row"] > 0, cov
