// fleet_rainflow.h -- battery degradation: streaming rainflow + SEI model, the linear model, and the EV's hot record.
//
// Provides: exp_small / pow_m0501 / cycle_stress (the stress of one cycle); rf_request / rf_begin / rf_finish / rf_finish_win (one SOC sample per
// step pushed into the EV's rainflow state); sei_evaluate (the daily evaluation); linear_degradation; hot_encode (struct Hot in
// fleet_device.h).
// Restates of the reference: LogDataDeg.log_soc, RainflowSeiDegradation / EmpiricalDegradation.calculate_degradation
// (utils/battery_degradation/*.py) and the third-party rainflow.extract_cycles / rainflow.reversals.
//
// Rainflow without a history replay.  The reference re-runs rainflow over the whole episode history every
// simulated day.  Three-point rainflow is a streaming algorithm, so the kernel keeps its state per EV (a row in HBM:
// closed-cycle count, sum of cycle means, the two newest stack entries, stress sum of the closed cycles that fall into the
// reference's slice, reversal stack; slope sign and stack size in the hot record) and feeds it ONE sample per step; the row
// is only touched by a step that pushes a reversal point, requested in the middle of the step and consumed at its end.  On the daily 14:45 row
// the forced last point and the residual half cycles are evaluated on a *virtual* copy of the stack (registers
// only), which reproduces the reference's full recount, including its cross-episode bookkeeping
// (rainflow_length, quirk Q6), at O(stack depth) instead of O(history).
//
// Expects of its caller: rf_begin ... rf_finish bracket one EV's step -- rf_begin right after the state machine (it requests the
// row when a point is pushed; with `early` the caller has issued rf_request itself), rf_finish after the observation stores and the
// money terms, with the RfReq rf_begin filled; sei_evaluate runs after the step's rf_finish and is told whether the registers hold
// a newer stack top than the row (`have_top`).  The workspace is sized for one episode (`stack_cap`); error bits are OR-ed into `err`.
#pragma once
#include "fleet_device.h"
#include "fleet_obs.h"
#include "fleet_stamps.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// battery degradation
// ---------------------------------------------------------------------------------------------------------
// exp(z) by its Taylor polynomial of degree 14: truncation < 2e-15 relative for |z| <= 0.55 (a mean SOC in [0, 1]) and
// < 8e-13 for |z| <= 1; beyond that -- a mean SOC far outside [0, 1], which the reference does not clip (quirk Q9) and a
// schedule whose trips use more than a battery charge can produce -- the library exp takes over.
__device__ __forceinline__ double exp_small(double z) {
  if (fabs(z) > 1.0) return exp(z);
  double r = 1.0 / 87178291200.0;  // 1/14!
  r = fma(r, z, 1.0 / 6227020800.0);
  r = fma(r, z, 1.0 / 479001600.0);
  r = fma(r, z, 1.0 / 39916800.0);
  r = fma(r, z, 1.0 / 3628800.0);
  r = fma(r, z, 1.0 / 362880.0);
  r = fma(r, z, 1.0 / 40320.0);
  r = fma(r, z, 1.0 / 5040.0);
  r = fma(r, z, 1.0 / 720.0);
  r = fma(r, z, 1.0 / 120.0);
  r = fma(r, z, 1.0 / 24.0);
  r = fma(r, z, 1.0 / 6.0);
  r = fma(r, z, 0.5);
  r = fma(r, z, 1.0);
  r = fma(r, z, 1.0);
  return r;
}

// x^(-0.501) for 0 < x <= 1, as x^(-1/2) * exp(-0.001 * ln x):
//   x^(-1/2): hardware reciprocal-square-root seed + two Newton steps (full float64 accuracy);
//   ln x    : hardware float32 log2 (relative error ~1e-7, i.e. <= 4e-6 absolute for x >= 1e-17); multiplied by
//             0.001 that leaves <= 4e-9 relative error in the result; exp of an argument <= 0.04 by Taylor.
// The library pow() would be exact to 1 ulp but costs several hundred instructions inside a divergent branch.
__device__ __forceinline__ double pow_m0501(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * fma(-0.5 * x * y, y, 1.5);
  y = y * fma(-0.5 * x * y, y, 1.5);
  const double lnx = (double)(__builtin_amdgcn_logf((float)x)) * 0.6931471805599453;  // log2 -> ln
  const double z = -0.001 * lnx;
  double r = 1.0 / 720.0;
  r = fma(r, z, 1.0 / 120.0);
  r = fma(r, z, 1.0 / 24.0);
  r = fma(r, z, 1.0 / 6.0);
  r = fma(r, z, 0.5);
  r = fma(r, z, 1.0);
  r = fma(r, z, 1.0);
  return y * r;
}

// stress of one rainflow cycle: deg_rate_cycle(dod, avg_soc, temp) (rainflow_sei_degradation.py:68-80) for
// effective_dod = clip(range*count, 0, 1) (:170).  Relative accuracy ~1e-8 (see pow_m0501), which moves SoH by
// < 1e-12 relative (the degradation is a 1e-5-sized correction to 1.0); DESIGN.md "Numerics".
__device__ __forceinline__ double cycle_stress(double rng, double mean, double count, double stress_temp) {
  double eff = rng * count;
  eff = eff > 1.0 ? 1.0 : eff;
  if (!(eff > 0.0)) return 0.0;  // pow(0, -0.501) = inf -> 1/inf = 0
  const double s_dod = 1.0 / (1.4E5 * pow_m0501(eff) + -1.23E5);   // (kd1 * dod**kd2 + kd3) ** -1
  const double s_soc = exp_small(1.04 * (mean - 0.5));              // e ** (k_sigma * (soc - sigma_ref)), |arg| <= 0.55
  return s_dod * s_soc * stress_temp;
}

// A real reversal point `p` arrives (rainflow.reversals yielded it): push it and close every cycle the
// three-point rule allows (rainflow.extract_cycles, the `while len(points) >= 3` loop).
// The stack of the EV always starts at slot 0 (`tail` = its size; when the three-point rule drops the FIRST point -- the
// stack is exactly [a, b, p] then -- the survivor below the top is rewritten to slot 0, so no head index exists and the size
// alone describes it).  Its newest entry lives in the row header only (s2; s1 caches the one below), the entries below it in
// the stack words behind the header (struct RfHdr in fleet_device.h).
// The push is split in two so that its memory round trip hides behind the rest of the step: `rf_begin`, right after the
// state machine, knows the new sample and therefore whether a reversal point is pushed, and REQUESTS the EV's row (header
// head, stack top, the two entries below the top two: three 16-byte loads of one cache line; `deep`: see rf_request); `rf_finish`, after the
// observation stores and the money terms, consumes it.  A step that pushes nothing -- three in four -- never touches the row.
struct RfReq {
  double p;        // the reversal point to push
  RfAccHead acc;   // requested when a point is pushed
  RfTop top;       // stack[tail-2], stack[tail-1]
  double w0, w1;   // stack[tail-3], [tail-4] (before the push)
  double w2, w3;   // stack[tail-5], [tail-6]: `deep` requests only
  bool push;
  bool win;        // w0 / w1 were requested (else the pops read the stack words)
};
// `early`: the row's header and the entries below the top two were already requested at the start of the EV's step (K steps
// per launch: the same row lines serve all K steps of the launch from the cache, and a wavefront that advances on its own is
// bound by its own dependent round trips, which this removes from every step that pushes).
// `deep` (a constant at every call; for rf_finish_win): the window reaches two entries further down -- one more 16-byte load of
// the same line, issued with the other three.  The K-step kernel, at its register limit, keeps the shallow request.
__device__ __forceinline__ void rf_request(const FleetDev& d, const EvIx& i, int tail, RfReq& q, bool deep = false) {
  const double* row = rf_row_of(d, i);
  q.acc = *reinterpret_cast<const RfAccHead*>(row);
  q.top = *reinterpret_cast<const RfTop*>(row + 2);
  // stack[tail-4], stack[tail-3]; for a shallow stack they fall into the row's own header (never used: `nwin`)
  const double* w = rf_row_of(d, i, (unsigned)(RF_HDR_WORDS + tail - 4));  // tail >= 1
  q.w1 = w[0];
  q.w0 = w[1];
  q.win = true;
  if (deep) {
    // stack[tail-6], stack[tail-5]: row words tail, tail + 1 -- header words again for a shallow stack, never before the row's first
    // word (tail >= 1), and never used then: a closure that reads them has found the stack deep enough
    q.w3 = w[-2];
    q.w2 = w[-1];
  }
}
__device__ __forceinline__ void rf_begin(const FleetDev& d, const EvIx& i, double old_deg, double soc_deg, int tail, int& sgn, RfReq& q,
                                         bool early = false, bool deep = false) {
  q.push = false;
  q.p = old_deg;
  // rainflow.reversals, one sample per step: equal samples are skipped, a strict slope sign change makes the previous
  // sample a reversal point
  if (soc_deg != old_deg) {
    const int s_next = (soc_deg > old_deg) ? 1 : 2;
    q.push = (sgn != 0 && sgn != s_next);
    sgn = s_next;
  }
  if (q.push && !early) rf_request(d, i, tail, q, deep);
}
// `top`: the stack top after the push (only written when a point was pushed)
// `acc_out`: the accumulator head after the push (only written when the push closed a cycle)
// Shape (round 5): the push that closes nothing, the half cycle and the FIRST full cycle are one straight line of selects -- the
// only memory they need is what rf_request brought (top two entries, the two below, the accumulators) -- and only a second closure
// of the same push (the new top against what lies below: rare) enters a loop that reads stack words.  The general loop of rounds
// 2-4 walked every push through its loop control and the first-point test: 8.3 -> 7.9 us per 4096x50 launch for the same
// algorithm (profiles/r05_experiments/ab7_rf_finish_peeled.log).
// `OWN_B` (one step per launch, one EV per lane, where the request is issued well before this runs): `b` gets a register of its own
// -- see where it is used.  Nothing checks the compiled code for this (the scheduling depends on the register coalescer): after a
// compiler update, look at the block that issues rf_request's loads in `G64.rainflow.single.f32` (EXPERIMENTS.md has the excerpt).
template <bool OWN_B>
__device__ __forceinline__ void rf_finish_as(const FleetDev& d, const EvIx& i, const RfReq& q, int& tail, RfTop& top, RfAccHead& acc_out,
                                          uint32_t& err) {
  if (!q.push) return;
  double* row = rf_row_of(d, i);
  double* stk = row + RF_HDR_WORDS;
  // Within an episode this cannot happen (pushes <= samples < stack_cap).  Past the finish row (no auto-reset) the samples keep
  // coming while the workspace stays sized for one episode: what must fit then is the stack depth, which only a long run of
  // ever smaller swings makes grow.  Refuse instead of overrunning -- the step that would overflow raises the error bit.
  if (tail >= d.stack_cap) {
    err |= FLEET_DEVERR_TABLE_END;
    return;
  }
  const double p = q.p;
  const double a0 = q.top.s1, b0 = q.top.s2;  // stack[tail-2] (also in the stack words), stack[tail-1] (only in the header)
  const int size = tail + 1;                  // points on the stack with p pushed
  const bool closes = (size >= 3) && !(fabs(p - b0) < fabs(b0 - a0));
  const bool half = closes && (size == 3);    // Y contains the starting point: half cycle, the first point is dropped
  // ONE store for b0: it joins the stack words when nothing closes (slot tail-1) and is rewritten to slot 0 when the first point
  // is dropped; a full cycle leaves the stack words as they are
  if (!closes || half) st_plain(rf_row_of(d, i, (unsigned)(RF_HDR_WORDS + (half ? 0 : tail - 1))), b0);
  const int L = q.acc.rf_len;
  int nc = q.acc.nc;
  double mean_sum = q.acc.mean_sum, dcsum = 0.0;
  bool has_csum = false;
  double a = a0, b = b0;
  // (a value of its own: otherwise `b`, which the closures below rewrite, shares its register with the requested word `b0`, and the
  // copy that separates the two is a phi copy: it lands at the end of the block that issued the request, behind a wait for the row
  // -- in every wavefront, right after the loads)
  if (OWN_B) asm volatile("" : "+v"(b));
  int t = size;
  if (closes) {
    if (nc >= L - 1) {  // only the closed cycles beyond the last evaluation's count carry stress: none in the steady state
      dcsum = cycle_stress(fabs(a0 - b0), 0.5 * (a0 + b0), half ? 0.5 : 1.0, d.self->stress_temp);
      has_csum = true;
    }
    mean_sum += 0.5 * (a0 + b0);
    nc += 1;
    if (half) {
      t = 2;  // stack = [b0, p]
    } else {  // full cycle: its two points vanish, p lives in s2, the entries below come from the request
      t = size - 2;
      const int nwin = q.win ? (tail - 2 > 2 ? 2 : tail - 2) : 0;
      b = (nwin >= 1) ? q.w0 : stk[t - 2];
      a = (t >= 3) ? ((nwin >= 2) ? q.w1 : stk[t - 3]) : 0.0;
      while (t >= 3) {  // further closures of the new top against what lies below: rare, from the stack words
        if (fabs(p - b) < fabs(b - a)) break;
        if (nc >= L - 1) {
          dcsum += cycle_stress(fabs(a - b), 0.5 * (a + b), (t == 3) ? 0.5 : 1.0, d.self->stress_temp);
          has_csum = true;
        }
        mean_sum += 0.5 * (a + b);
        nc += 1;
        if (t == 3) {
          stk[0] = b;
          t = 2;
        } else {
          t -= 2;
          b = stk[t - 2];
          a = (t >= 3) ? stk[t - 3] : 0.0;
        }
      }
    }
  }
  tail = t;
  top.s1 = b;  // stack[tail-2]
  top.s2 = p;  // stack[tail-1]
  st_plain(reinterpret_cast<RfTop*>(row + 2), top);
  if (closes) {
    RfAccHead out;
    out.mean_sum = mean_sum;
    out.nc = nc;
    out.rf_len = L;
    acc_out = out;
    st_plain(reinterpret_cast<RfAccHead*>(row), out);
    if (has_csum) reinterpret_cast<RfHdr*>(row)->csum += dcsum;
  }
}
// (two plain functions in front of the one body: with callers instantiating the template themselves, or with a run-time flag, instances
// that never push -- other degradation modes, K-step -- came out with another register allocation; EXPERIMENTS.md "What perturbs ...")
__device__ __forceinline__ void rf_finish(const FleetDev& d, const EvIx& i, const RfReq& q, int& tail, RfTop& top, RfAccHead& acc_out,
                                          uint32_t& err) {
  rf_finish_as<false>(d, i, q, tail, top, acc_out, err);
}
__device__ __forceinline__ void rf_finish_own_b(const FleetDev& d, const EvIx& i, const RfReq& q, int& tail, RfTop& top, RfAccHead& acc_out,
                                                uint32_t& err) {
  rf_finish_as<true>(d, i, q, tail, top, acc_out, err);
}
// The same push for the state-only twin of the one-step, one-EV-per-lane kernel with float32 actions -- 1999 of a direct run's 2000
// launches --, where the request (`deep`) is issued well before this runs and a wavefront pays for its worst lane:
// a second closure is rare per push (8 %) and common per wavefront (one launch in two has a
// lane with one), and in the loop above it is a dependent load at the very end of the wavefront's step.  Here the second closure
// too -- the new top against the two entries below the first cycle, a full cycle or the half cycle at size 3 with its rewrite of
// slot 0 -- is decided and performed from the request's window, by selects inside the one `closes` region; the loop starts at the
// third closure and is entered only by a wavefront that has such a lane (0.9 % of pushes).  Every sum is added in the order of
// the loop above: results are the same bit for bit.  (A window two entries deeper still, and `csum` fetched with the request, were
// built and measured: EXPERIMENTS.md "The second closure from the request's window".)
// The live instances and the float64 twins keep rf_finish_own_b: with the deeper window they fall from five resident wavefronts per
// SIMD to four (99 / 98 VGPRs), which the closed loop pays for at the large shapes (+2.7 % at 16384 x 50, +6.5 % at c5).
// `b` gets a register of its own as in rf_finish_as<true>; the same care for the closed-cycle count (`k`).
// stress_temp is read as the kernel argument (`d.stress_temp`), which the twin fetches with its entry's argument loads
// (fleet_kernels.hip), not from the device-resident copy of the argument block as in rf_finish_as: that was a vector load of a launch
// constant with a `vmcnt(0)` behind it in each inlined cycle_stress, a wait that also covers the push's stores -- and the copy's
// pointer was one more late scalar fetch on every wavefront's path (EXPERIMENTS.md "Rainflow push in the twin: no load wait behind a
// store", which also has the two re-orderings of this function's stores and of its `csum` update that were measured and not kept).
__device__ __forceinline__ void rf_finish_win(const FleetDev& d, const EvIx& i, const RfReq& q, int& tail, RfTop& top, RfAccHead& acc_out,
                                                uint32_t& err) {
  if (!q.push) return;
  double* row = rf_row_of(d, i);
  double* stk = row + RF_HDR_WORDS;
  if (tail >= d.stack_cap) {  // (see rf_finish)
    err |= FLEET_DEVERR_TABLE_END;
    return;
  }
  const double p = q.p;
  const double a0 = q.top.s1, b0 = q.top.s2;  // stack[tail-2] (also in the stack words), stack[tail-1] (only in the header)
  const int size = tail + 1;                  // points on the stack with p pushed
  const bool closes = (size >= 3) && !(fabs(p - b0) < fabs(b0 - a0));
  const bool half = closes && (size == 3);    // Y contains the starting point: half cycle, the first point is dropped
  // ONE store for b0: it joins the stack words when nothing closes (slot tail-1) and is rewritten to slot 0 when the first point
  // is dropped; a full cycle leaves the stack words as they are
  if (!closes || half) st_plain(rf_row_of(d, i, (unsigned)(RF_HDR_WORDS + (half ? 0 : tail - 1))), b0);
  const int L = q.acc.rf_len;
  // closed cycles of this push, and the first of them that carries stress: only the closed cycles beyond the last evaluation's
  // count do (index >= L - 1), none in the steady state.  (The requested count itself is only ever read: a count that the closures
  // rewrite costs what `b` below would.)
  int k = 0;
  const int k_stress = L - 1 - q.acc.nc;
  double mean_sum = q.acc.mean_sum, dcsum = 0.0;
  bool has_csum = false;
  double a = a0, b = b0;
  // (a value of its own: otherwise `b`, which the closures below rewrite, shares its register with the requested word `b0`, and the
  // copy that separates the two is a phi copy: it lands at the end of the block that issued the request, behind a wait for the row
  // -- in every wavefront, right after the loads)
  asm volatile("" : "+v"(b));
  int t = size;
  if (closes) {
    mean_sum += 0.5 * (a0 + b0);
    // the first cycle was a full one (its two points vanish, p lives in s2): the new top against the two entries below it.  A
    // window word of a shallow stack is a header word: `t >= 3` keeps it out of the test, and the word that becomes `b` after a
    // full closure (t >= 4 before it) is always a stack word.
    const double a1 = q.w1, b1 = q.w0;
    const int t1 = size - 2;
    const bool closes2 = !half && (t1 >= 3) && !(fabs(p - b1) < fabs(b1 - a1));
    const bool half2 = closes2 && (t1 == 3);
    const bool full2 = closes2 && !half2;
    mean_sum = closes2 ? mean_sum + 0.5 * (a1 + b1) : mean_sum;
    k = closes2 ? 2 : 1;
    t = half ? 2 : (closes2 ? (half2 ? 2 : t1 - 2) : t1);  // half: stack = [b0, p]; half2: [b1, p]
    b = half ? b : (full2 ? q.w2 : b1);
    a = full2 ? q.w3 : a1;
    if (half2) stk[0] = b1;
    if (k > k_stress) {  // the last closure has the largest index: one test for both
      if (0 >= k_stress) {
        dcsum = cycle_stress(fabs(a0 - b0), 0.5 * (a0 + b0), half ? 0.5 : 1.0, d.stress_temp);
        has_csum = true;
      }
      if (closes2) {
        dcsum += cycle_stress(fabs(a1 - b1), 0.5 * (a1 + b1), half2 ? 0.5 : 1.0, d.stress_temp);
        has_csum = true;
      }
    }
    // from the third closure on: the first pair is still the request's, the ones below it come from the stack words
    if (full2 && (t >= 3) && !(fabs(p - b) < fabs(b - a))) {
      do {
        if (k >= k_stress) {
          dcsum += cycle_stress(fabs(a - b), 0.5 * (a + b), (t == 3) ? 0.5 : 1.0, d.stress_temp);
          has_csum = true;
        }
        mean_sum += 0.5 * (a + b);
        k += 1;
        if (t == 3) {
          stk[0] = b;
          t = 2;
        } else {
          t -= 2;
          b = stk[t - 2];
          a = (t >= 3) ? stk[t - 3] : 0.0;
        }
      } while (t >= 3 && !(fabs(p - b) < fabs(b - a)));
    }
  }
  tail = t;
  top.s1 = b;  // stack[tail-2]
  top.s2 = p;  // stack[tail-1]
  st_plain(reinterpret_cast<RfTop*>(row + 2), top);
  if (closes) {
    RfAccHead out;
    out.mean_sum = mean_sum;
    out.nc = q.acc.nc + k;
    out.rf_len = L;
    acc_out = out;
    st_plain(reinterpret_cast<RfAccHead*>(row), out);
    if (has_csum) reinterpret_cast<RfHdr*>(row)->csum += dcsum;
  }
}
// RainflowSeiDegradation.calculate_degradation for one EV on the daily row (rainflow_sei_degradation.py:91-212).
// `v` = the sample just logged (forced last reversal), `n` = number of logged samples.  The forced point and the
// residual half cycles are evaluated on a virtual stack (vt, vh, registers a/b); nothing of the streaming state
// is modified except rainflow_length / fd_cyc / fd_cal / l / csum when the reference would update them.
// `top` / `have_top`: the stack top when this step's push has just written it (registers are newer than the row).
__device__ __forceinline__ double sei_evaluate(const FleetDev& d, const EvIx& ix, double v, int n, int tail, const RfTop& top, bool have_top,
                                             uint32_t& err, double dt_hours, int* new_len = nullptr) {
  const size_t i = ix.flat();
  double* row = d.rf_rows + i * (size_t)d.rf_row_stride;
  const double* stk = row + RF_HDR_WORDS;
  // everything this needs from memory is requested up front (one round trip)
  const RfHdr hd = *reinterpret_cast<const RfHdr*>(row);
  SeiRec sr = d.sei[i];
  const int L = hd.rf_len;
  const int nc = hd.nc;
  const double mean_sum0 = hd.mean_sum, csum0 = hd.csum, fd_cyc0 = sr.fd_cyc, sei_l0 = sr.sei_l, sei_soh0 = sr.sei_soh;
  const double st = d.stress_temp;
#ifdef FLEET_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  FLEET_STAMP(11);  // records arrived

  // The walk below emits at most one cycle per stack entry (`tail` entries and the forced last point make at most `tail`
  // ranges), and the model is only updated when the cycle count passes rainflow_length (`len > L` below): an EV whose closed
  // cycles plus stack entries stay within it -- typically the first 14:45 row of an episode, whose rainflow_length still is the
  // previous episode's (quirk Q6) -- gets no update whatever the walk finds: degradation 0, records as they are.  Nothing to
  // walk, nothing to store.  (These wavefronts end their launch: -1.3 % per launch at 4096 x 50, -16 % at 2048 x 50.)
  if (nc + tail <= L) return 0.0;
  int nv = 0;
  double vmean = 0.0, vsum = 0.0, pend = 0.0, max_dod = 0.0;
  bool has_pend = false;
  auto emit = [&](double x1, double x2, double count) {
    if (has_pend) vsum += pend;  // the previous cycle is not the last one
    has_pend = false;
    const double rng = fabs(x1 - x2), mean = 0.5 * (x1 + x2);
    if (nc + nv >= L - 1) {
      pend = cycle_stress(rng, mean, count, st);
      has_pend = true;
      max_dod = rng > max_dod ? rng : max_dod;
    }
    vmean += mean;
    nv += 1;
  };
  if (n >= 3) {  // with two samples rainflow.reversals yields only the first point: no cycle at all
    int vt = tail, vh = 0;
    int size = vt - vh + 1;
    double a = have_top ? top.s1 : hd.s1, b = have_top ? top.s2 : hd.s2;
    while (size >= 3) {
      const double X = fabs(v - b), Y = fabs(b - a);
      if (X < Y) break;
      emit(a, b, (size == 3) ? 0.5 : 1.0);
      if (size == 3) {
        vh += 1;
        size = 2;
      } else {
        vt -= 2;
        size -= 2;
        b = stk[vt - 1];
        a = (size >= 3) ? stk[vt - 2] : 0.0;
      }
    }
    // remaining ranges are half cycles: stack[vh..vt) followed by the forced point
    double prev = (vt - vh >= 2) ? stk[vh] : b;
    for (int j = vh + 1; j < vt; ++j) {
      const double cur = (j == vt - 1) ? b : stk[j];
      emit(prev, cur, 0.5);
      prev = cur;
    }
    emit(b, v, 0.5);
  }

  FLEET_STAMP(12);  // stack walked, cycle stresses evaluated
  double degradation = 0.0;
  double sei_l = sei_l0;
  const int len = nc + nv;
  if (len > 0 && len > L) {
    if (max_dod > 5.0) err |= FLEET_DEVERR_DOD_RANGE;
    const double battery_age = (double)(n - 1) * dt_hours * 3600.0;  // max(End) is always the last sample's index
    const double mean_soc_cal = (mean_sum0 + vmean) / (double)len;
    const double fd_cyc = fd_cyc0 + (csum0 + vsum);
    const double fd_cal = (4.14E-10 * battery_age) * exp(1.04 * (mean_soc_cal - 0.5)) * st;
    const double fd = fd_cyc + fd_cal;
    const double alpha = 5.75E-2, beta = 121.0;
    sei_l = 1.0 - alpha * exp(-beta * fd) - (1.0 - alpha) * exp(-fd);
    if (sei_l < 0.0) err |= FLEET_DEVERR_NEG_LIFE;
    degradation = sei_l - sei_l0;
    sr.fd_cyc = fd_cyc;
    sr.fd_cal = fd_cal;
    sr.sei_l = sei_l;
    RfAccHead out;  // rainflow_length moves on; every closed cycle so far now lies below the new rainflow_length-1
    out.mean_sum = mean_sum0;
    out.nc = nc;
    out.rf_len = len;
    *reinterpret_cast<RfAccHead*>(row) = out;
    reinterpret_cast<RfHdr*>(row)->csum = 0.0;
    if (new_len) *new_len = len;
  }
  FLEET_STAMP(13);  // SEI model evaluated
  const double s = sei_soh0 - degradation;
  sr.sei_soh = s;
  d.sei[i] = sr;
  if (fabs(s - (1.0 - sei_l)) > 0.0001) err |= FLEET_DEVERR_SOH_MISMATCH;
  return degradation;
}

// EmpiricalDegradation.calculate_degradation for one EV (empirical_degradation.py:29-99; quirks Q1, Q5):
// the last two log entries are the SOC sample before and after this step.
__device__ __forceinline__ double linear_degradation(const FleetDev& d, double old_soc, double new_soc, double dt_hours) {
  const double avg = (old_soc + new_soc) / 2.0;
  // nearest of {0, 40, 90} to a SOC on a [0,1] scale -- replicated literally (argmin, first wins ties)
  int best = 0;
  double bd = fabs(0.0 - avg);
  if (fabs(40.0 - avg) < bd) { best = 1; bd = fabs(40.0 - avg); }
  if (fabs(90.0 - avg) < bd) best = 2;
  const double cal = (best == 0 ? 0.0065 : best == 1 ? 0.0293 : 0.065) * dt_hours / 8760.0;
  const double dod = fabs(new_soc - old_soc);
  const double cyc = (d.evse_power <= 22.0) ? dod * 0.000125 / 2.0 : dod * 0.000167 / 2.0;
  return cal + cyc;
}

// The hot record of an EV whose soc / soc_deg / hours_left are given (struct Hot in fleet_device.h): the shared float64
// field, the FROZEN / INPLANE flags, and the soc_deg plane entry in the one case that needs it.  `plane_has` = the
// plane already holds this soc_deg (the EV was INPLANE before and soc_deg has not changed since).
__device__ __forceinline__ Hot hot_encode(const FleetDev& d, const EvIx& i, double soc, double soc_deg, float hl, int tail, int sgn,
                                          uint32_t there, bool t090, bool plane_has) {
  Hot h;
  h.hl = hl;
  bool frozen = false, inplane = false;
  h.x = soc;
  if (__double_as_longlong(soc_deg) != __double_as_longlong(soc)) {
    frozen = true;
    if (__double_as_longlong(soc) == 0ll) {
      h.x = soc_deg;  // soc == +0.0 is implied
    } else {
      inplane = true;
      if (!plane_has) d.soc_deg[i.flat()] = soc_deg;
    }
  }
  h.bits = HOT_PACK(tail, sgn, frozen, inplane, there, t090);
  return h;
}

}  // namespace
