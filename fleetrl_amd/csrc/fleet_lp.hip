// fleet_lp.hip -- the linear-optimisation benchmark (benchmarking/linear_optimization.py:55-247 of the reference), solved
// exactly per (env, EV) on the GPU.  One lane per (env, EV); the model, the per-row relaxed cost r_i and the method are derived
// in DESIGN.md section 8 "The linear-optimisation benchmark".  In short:
//   * a plan splits into parking sessions separated by fixed-SOC rows (arrival, departure, away);
//   * inside a session the relaxed problem is a path of convex piecewise-linear row costs r_i(delta) with the SOC box
//     [0, target] on every node: a backward DP whose value function W_i is held as (slope, length) segments sorted by slope;
//     W_i = (W_{i+1} infimal-convolved with r_i(-x)) is a merge of the two segment lists, the box is a trim of both ends;
//   * while merging, the planner stores per row and r_i piece the SOC at which W_{i+1}'s slope crosses minus that piece's
//     slope; the forward pass recovers every delta_i from those thresholds and realises it with one-sided actions.
// Exact to round-off (no iteration, no tolerance), no atomics: two calls give bit-identical results.
#include "fleet_lp.h"

namespace {

constexpr int KM = FLEET_LP_MAX_PIECES;

// bits of the per-(env, EV) status word (include/fleet_hip.h FLEET_LP_*)
constexpr int32_t kUnreachable = FLEET_LP_UNREACHABLE;
constexpr int32_t kNegReturn = FLEET_LP_NEG_RETURN;
constexpr int32_t kAboveTarget = FLEET_LP_ABOVE_TARGET;
constexpr int32_t kGridNegative = FLEET_LP_GRID_NEGATIVE;

// r_i: breakpoints b[0] < ... < b[m] (net SOC change per row), slopes sg[0] < ... < sg[m-1] (EUR per unit of SOC),
// r_i(b[0]) = c_left, r_i(b[m]) = c_right
struct LpRow {
  int m;
  double b[KM + 1];
  double sg[KM];
  double c_left, c_right;
};

// Per-row constants of the model: price [EUR/kWh], g = eta_d * tariff' [EUR/kWh], grid headroom G [kW]
// and the EV's PV share s [kW]
struct LpIn {
  double price, g, G, spv;
};

__device__ inline LpIn lp_in(const FleetDev& d, int t, int N, int32_t& bits) {
  const PhysRow& ph = d.tab_phys[t];
  LpIn in;
  in.price = ph.k_cost;
  in.g = -ph.k_rev;
  double G = d.grid_connection - ph.load + ph.pv;
  if (G < 0.0) {
    bits |= kGridNegative;
    G = 0.0;
  }
  in.G = G;
  in.spv = ph.pv > 0.0 ? ph.pv / (double)N : 0.0;
  return in;
}

// Lower convex hull of the images (delta, cost) of the vertices of the row's feasible polygon in (charge x, discharge y) [kW],
// split at x = s where the charge cost changes slope.  The relaxed row cost is that hull.
__device__ inline void lp_row(const FleetDev& d, const LpIn& in, LpRow& r) {
  const double P = d.evse_power, G = in.G, s = in.spv, pr = in.price, g = in.g, dt = d.dt, cap = d.init_cap, ec = d.eta_c;
  double px[6], pc[6];
  int n = 0;
  auto add = [&](double x, double y) {
    const double cx = pr > 0.0 ? pr * fmax(0.0, x - s) : pr * x;
    px[n] = (ec * x - y) * dt / cap;
    pc[n] = dt * (cx - g * y);
    n += 1;
  };
  const double xc = fmin(P, G);
  const double xd = 0.5 * (P + G);  // x of the corner x + y = P, x - y = G
  add(0.0, 0.0);
  add(0.0, P);
  add(xc, 0.0);
  if (G < P) add(xd, 0.5 * (P - G));
  if (pr > 0.0 && s > 0.0 && s < P) {
    if (s < xc) add(s, 0.0);
    if (s <= xd) add(s, P - s);
    if (s > G && s < xd) add(s, s - G);
  }
  // sort by (delta, cost): n <= 6
  for (int i = 1; i < 6; ++i) {
    if (i >= n) break;
    const double kx = px[i], kc = pc[i];
    int j = i - 1;
    while (j >= 0 && (px[j] > kx || (px[j] == kx && pc[j] > kc))) {
      px[j + 1] = px[j];
      pc[j + 1] = pc[j];
      --j;
    }
    px[j + 1] = kx;
    pc[j + 1] = kc;
  }
  // Andrew's monotone chain, lower half; equal deltas keep the cheaper point
  double hx[6], hc[6];
  int h = 0;
  for (int i = 0; i < 6; ++i) {
    if (i >= n) break;
    if (h > 0 && px[i] == hx[h - 1]) continue;
    while (h >= 2 && (hx[h - 1] - hx[h - 2]) * (pc[i] - hc[h - 2]) - (hc[h - 1] - hc[h - 2]) * (px[i] - hx[h - 2]) <= 0.0) --h;
    hx[h] = px[i];
    hc[h] = pc[i];
    ++h;
  }
  r.m = h - 1;
  for (int k = 0; k < h; ++k) r.b[k] = hx[k];
  for (int k = 0; k + 1 < h; ++k) r.sg[k] = (hc[k + 1] - hc[k]) / (hx[k + 1] - hx[k]);
  r.c_left = hc[0];
  r.c_right = hc[h - 1];
}

// The one-sided realisation of a net SOC change and what the MILP's objective books for it (decision 2)
__device__ inline double lp_cost_of_action(const FleetDev& d, const LpIn& in, double a) {
  const double x = a * d.evse_power;
  if (a > 0.0) return d.dt * (in.price > 0.0 ? in.price * fmax(0.0, x - in.spv) : in.price * x);
  return d.dt * (in.g * x);
}

// departure row: d = 0 and no SOC effect; the cheapest charge action of the row (0 unless the price is negative)
__device__ inline double lp_departure_action(const FleetDev& d, const LpIn& in) {
  return in.price < 0.0 ? fmin(d.evse_power, in.G) / d.evse_power : 0.0;
}

__device__ inline double lp_fixed_soc(double v, double target, int32_t& bits, int32_t neg_bit) {
  if (v < 0.0) {
    bits |= neg_bit;
    return 0.0;
  }
  if (v > target) {
    bits |= kAboveTarget;
    return target;
  }
  return v;
}

__device__ inline bool lp_there(const FleetDev& d, int t, int c) { return SEG_THERE(d.seg[(size_t)t * d.N + c].se) != 0u; }

__global__ void __launch_bounds__(256) fleet_lp_plan_kernel(FleetDev d, FleetLpArgs a) {
  const int E = d.E, N = d.N, H = a.H;
  const size_t nl = (size_t)E * N;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nl) return;
  const int e = (int)(g / N), c = (int)(g % N);
  const size_t capL = (size_t)KM * H + 2;
  double2* LA = reinterpret_cast<double2*>(a.scratch);
  double2* LB = LA + capL * nl;
  double* thr = reinterpret_cast<double*>(LB + capL * nl);  // [H][KM][nl]; slot k = 0 of a departure row holds its target
  double* lane_out = thr + (size_t)H * KM * nl;              // bound [nl], plan cost [nl]
  auto TH = [&](int i, int k) -> double& { return thr[((size_t)i * KM + k) * nl + g]; };

  const double target = d.target_soc, ec = d.eta_c;
  const double kstep = d.evse_power * d.dt / d.init_cap;
  const int t0 = d.env[e].h.t;
  int32_t bits = 0;
  const Hot hot0 = d.hot[g];
  const bool pres0 = lp_there(d, t0, c);
  const double S0 = pres0 ? lp_fixed_soc(HOT_SOC(hot0), target, bits, kNegReturn) : 0.0;

  // ---- pass 1 (forward): the highest SOC each session can reach by its departure row (decision 3) ----------------------
  {
    double m = S0;
    for (int i = 0; i < H; ++i) {
      const int t = t0 + i;
      const LpIn in = lp_in(d, t, N, bits);
      if (!lp_there(d, t, c)) {
        if (i + 1 < H && lp_there(d, t + 1, c)) m = lp_fixed_soc(d.seg[(size_t)(t + 1) * N + c].sor, target, bits, kNegReturn);
        continue;
      }
      if (i < H - 1 && !lp_there(d, t + 1, c)) {
        double tau = target;
        if (m < target) {
          tau = m;
          bits |= kUnreachable;
        }
        TH(i, 0) = tau;
        continue;
      }
      LpRow r;
      lp_row(d, in, r);
      m = fmin(target, m + r.b[r.m]);
    }
  }

  // ---- pass 2 (backward): value functions, thresholds, the relaxed optimum --------------------------------------------
  double bound = 0.0;
  {
    double lo = 0.0, hi = 0.0, v0 = 0.0;
    int L = 0;
    double2* cur = LA;
    double2* nxt = LB;
    auto eval = [&](double S) {  // W(S) of the current value function, S clamped into its domain
      S = fmin(fmax(S, lo), hi);
      double v = v0, pos = lo;
      for (int j = 0; j < L && pos < S; ++j) {
        const double2 sl = cur[(size_t)j * nl + g];
        const double take = fmin(sl.y, S - pos);
        v += sl.x * take;
        pos += take;
      }
      return v;
    };
    bool pres_next = false;
    for (int i = H - 1; i >= 0; --i) {
      const int t = t0 + i;
      const bool pres = lp_there(d, t, c);
      if (!pres) {
        if (pres_next) bound += eval(lp_fixed_soc(d.seg[(size_t)(t + 1) * N + c].sor, target, bits, kNegReturn));
        pres_next = false;
        continue;
      }
      int32_t nob = 0;  // (the status bits were all collected by pass 1)
      const LpIn in = lp_in(d, t, N, nob);
      if (i == H - 1) {  // open end: W_H = 0 on [0, target]
        lo = 0.0;
        hi = target;
        v0 = 0.0;
        cur[g] = make_double2(0.0, target);
        L = 1;
      } else if (!pres_next) {  // departure row: SOC fixed at the (possibly lowered) target, no SOC effect
        lo = hi = TH(i, 0);
        v0 = 0.0;
        L = 0;
        bound += lp_cost_of_action(d, in, lp_departure_action(d, in));
        pres_next = true;
        continue;
      }
      // dynamic row: W_i(s) = min_delta r_i(delta) + W_{i+1}(s + delta), trimmed to [0, target]
      LpRow r;
      lp_row(d, in, r);
      const double nlo = lo - r.b[r.m], nhi = hi - r.b[0];
      double nv = v0 + r.c_right;
      const double olo = fmax(0.0, nlo), ohi = fmin(target, nhi);
      double cut = olo - nlo, keep = ohi - olo;
      int ia = 0, kr = r.m - 1, Lo = 0;
      double accW = 0.0;
      double ps = 0.0, pl = 0.0;  // pending output segment (equal slopes coalesce)
      bool pending = false;
      while (ia < L || kr >= 0) {
        double sl, len;
        if (kr < 0 || (ia < L && cur[(size_t)ia * nl + g].x < -r.sg[kr])) {
          const double2 w = cur[(size_t)ia * nl + g];
          sl = w.x;
          len = w.y;
          accW += len;
          ++ia;
        } else {
          TH(i, kr) = lo + accW;
          sl = -r.sg[kr];
          len = r.b[kr + 1] - r.b[kr];
          --kr;
        }
        if (cut > 0.0) {
          const double take = fmin(len, cut);
          nv += sl * take;
          cut -= take;
          len -= take;
        }
        if (len > 0.0 && keep > 0.0) {
          const double take = fmin(len, keep);
          keep -= take;
          if (pending && ps == sl) {
            pl += take;
          } else {
            if (pending) nxt[(size_t)(Lo++) * nl + g] = make_double2(ps, pl);
            ps = sl;
            pl = take;
            pending = true;
          }
        } else if (keep <= 0.0 && kr < 0) {
          break;
        }
      }
      if (pending) nxt[(size_t)(Lo++) * nl + g] = make_double2(ps, pl);
      lo = olo;
      hi = ohi;
      v0 = nv;
      L = Lo;
      double2* tmp = cur;
      cur = nxt;
      nxt = tmp;
      pres_next = true;
    }
    if (pres0) bound += eval(S0);
  }

  // ---- pass 3 (forward): the plan ----------------------------------------------------------------------------------------
  double cost = 0.0;
  {
    double s = S0;
    int32_t nob = 0;
    for (int i = 0; i < H; ++i) {
      const int t = t0 + i;
      const bool pres = lp_there(d, t, c);
      const bool pres_next = i + 1 < H && lp_there(d, t + 1, c);
      if (a.soc_plan) a.soc_plan[(size_t)i * nl + g] = pres ? s : 0.0;
      double act = 0.0, sn = 0.0;
      if (pres) {
        const LpIn in = lp_in(d, t, N, nob);
        if (i < H - 1 && !pres_next) {
          act = lp_departure_action(d, in);
        } else {
          LpRow r;
          lp_row(d, in, r);
          double delta = r.b[0];
          for (int k = 0; k < r.m; ++k) {
            const double want = TH(i, k) - s;
            if (want <= r.b[k]) break;
            delta = fmin(want, r.b[k + 1]);
          }
          sn = fmin(fmax(s + delta, 0.0), target);
          if (i + 1 < H - 1 && !lp_there(d, t + 2, c)) sn = TH(i + 1, 0);  // the next row is a departure row
          delta = sn - s;
          act = delta > 0.0 ? delta / (ec * kstep) : delta / kstep;
          act = fmin(fmax(act, -1.0), 1.0);
        }
        cost += lp_cost_of_action(d, in, act);
      } else if (pres_next) {
        sn = lp_fixed_soc(d.seg[(size_t)(t + 1) * N + c].sor, target, nob, kNegReturn);
      }
      const size_t o = (size_t)i * nl + g;
      if (a.act_dtype == FLEET_ACT_F64)
        static_cast<double*>(a.actions)[o] = act;
      else
        static_cast<float*>(a.actions)[o] = (float)act;
      s = sn;
    }
    if (a.soc_plan) a.soc_plan[(size_t)H * nl + g] = s;
  }
  a.status[g] = bits;
  lane_out[g] = bound;
  lane_out[nl + g] = cost;
}

// per-env sums over the EVs in a fixed order (deterministic)
__global__ void fleet_lp_sum_kernel(int E, int N, const double* lane_out, double* bound, double* plan_cost) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const size_t nl = (size_t)E * N;
  double b = 0.0, p = 0.0;
  for (int c = 0; c < N; ++c) {
    b += lane_out[(size_t)e * N + c];
    p += lane_out[nl + (size_t)e * N + c];
  }
  bound[e] = b;
  plan_cost[e] = p;
}

}  // namespace

size_t fleet_lp_scratch_bytes(size_t lanes, int H) {
  const size_t capL = (size_t)KM * H + 2;
  return lanes * (2 * capL * sizeof(double2) + (size_t)H * KM * sizeof(double) + 2 * sizeof(double));
}

hipError_t fleet_launch_lp_plan(const FleetDev& d, const FleetLpArgs& a, hipStream_t s) {
  const size_t nl = (size_t)d.E * d.N;
  const unsigned block = 256;
  hipLaunchKernelGGL(fleet_lp_plan_kernel, dim3((unsigned)((nl + block - 1) / block)), dim3(block), 0, s, d, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const size_t capL = (size_t)KM * a.H + 2;
  const double* lane_out = a.scratch + nl * (4 * capL + (size_t)a.H * KM);
  hipLaunchKernelGGL(fleet_lp_sum_kernel, dim3((unsigned)((d.E + 127) / 128)), dim3(128), 0, s, d.E, d.N, lane_out, a.bound,
                     a.plan_cost);
  return hipGetLastError();
}
