"""Restatement of the linear-optimisation benchmark's model for ONE EV (the reference's
benchmarking/linear_optimization.py:55-247), independent of the HIP planner:

  * `build_lp` / `solve_scipy`: the model as a scipy (HiGHS) LP or MILP, variables c, d, u, b per row and soc per node;
  * `solve_numpy`: a slow exact solver of the LP relaxation: a forward DP over each parking session with the value function
    held as breakpoints, and a backward recovery of the SOC trajectory;
  * `realise` / `check_tape`: decision 2's one-sided realisation of a SOC trajectory and a feasibility check of an action tape
    against every MILP constraint.

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
