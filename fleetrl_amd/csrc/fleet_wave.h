// fleet_wave.h -- wavefront and lane-group primitives of the step / reset kernels, and the small arithmetic they share.
//
// Provides: sums over an aligned group of G lanes (DPP row shifts / row broadcasts: group_sum_to_last; four quantities at once for
// a whole wavefront with the gfx950 lane swaps: wave_sum4_to_last) and group_any; the Philox start-row sampler and choose_start;
// division by a reciprocal (rcp_newton, rcp_newton1, div_rcp); the two sigmoid penalties.
// Restates of the reference: the time pickers' choice of a start row (fleet_environment.py:351-355, same Philox specification as
// the oracle's) and ScoreConfig.soc_violation_penalty / overloading_penalty (fleet_env/config/score_config.py:26-41).
// Expects of its caller: the reductions are executed by ALL 64 lanes of a wavefront (uniform control flow) and leave their result
// in the LAST lane of the group; div_rcp is given rc ~ 1 / c good to 2^-44 or better.
#pragma once
#include "fleet_device.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// wavefront helpers
// ---------------------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  // old = 0 and bound_ctrl = 1: lanes whose source is out of range (or whose row is masked off) add 0.0
  int l2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xF, true);
  int h2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xF, true);
  return v + __hiloint2double(h2, l2);
}

// Sum over the G lanes of an aligned group; the result is valid in the LAST lane of the group.
// row_shr:1/2/4/8 (0x111..0x118) scan inside a 16-lane row, row_bcast:15 (0x142) and row_bcast:31 (0x143)
// carry row totals across rows.  All 64 lanes must execute this (uniform control flow).
// true in every lane of the group if `v` holds in any of its lanes (real_time event test)
template <int G>
__device__ __forceinline__ bool group_any(bool v) {
  const unsigned long long m = __ballot(v);
  if (G >= 64) return m != 0ull;  // (groups of several wavefronts never run the event-skipping loop: plan_step_gd)
  const int base = (int)(threadIdx.x % 64) & ~(G - 1);
  return ((m >> base) & ((1ull << (G % 64)) - 1ull)) != 0ull;
}

template <int G>
__device__ __forceinline__ double group_sum_to_last(double v) {
  if (G >= 2) v = dpp_add<0x111, 0xF>(v);
  if (G >= 4) v = dpp_add<0x112, 0xF>(v);
  if (G >= 8) v = dpp_add<0x114, 0xF>(v);
  if (G >= 16) v = dpp_add<0x118, 0xF>(v);
  if (G >= 32) v = dpp_add<0x142, 0xA>(v);
  if (G >= 64) v = dpp_add<0x143, 0xC>(v);
  return v;
}

// Four per-env sums at once for one env per wavefront (G == 64); the totals are valid in the LAST lane.  The quantities are
// folded pairwise with the gfx950 lane-swap instructions -- after `v_permlane32_swap` one register holds the lower half's
// values of a AND b, the other the upper half's, so ONE add folds two quantities from 64 to 32 lanes; `v_permlane16_swap`
// does the same from 32 to 16 -- which leaves each quantity spread over one 16-lane row; four DPP row shifts finish the rows
// and three lane reads bring the other rows' totals to the last lane: 27 vector instructions instead of 18 per quantity.
__device__ __forceinline__ double swap_fold32(double a, double b) {
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);  // lanes 0-31: a folded, 32-63: b folded
}
__device__ __forceinline__ double swap_fold16(double x, double y) {
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);  // rows: x.r0+x.r1, y.r0+y.r1, x.r2+x.r3, y.r2+y.r3
}
__device__ __forceinline__ double lane_read(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ void wave_sum4_to_last(double& a, double& b, double& c, double& dd) {
  double z = swap_fold16(swap_fold32(a, b), swap_fold32(c, dd));  // row 0: a, row 1: c, row 2: b, row 3: dd (16 partial sums each)
  z = dpp_add<0x111, 0xF>(z);
  z = dpp_add<0x112, 0xF>(z);
  z = dpp_add<0x114, 0xF>(z);
  z = dpp_add<0x118, 0xF>(z);  // row totals in lanes 15, 31, 47, 63
  a = lane_read(z, 15);
  c = lane_read(z, 31);
  b = lane_read(z, 47);
  dd = z;  // the last lane's own row
}

// Philox4x32-10 start-row sampler; same specification as the oracle's (counter = (global env, episode, 0, 0)).
__device__ __forceinline__ uint32_t philox_start(unsigned long long seed, uint32_t env, uint32_t episode) {
  uint32_t c0 = env, c1 = episode, c2 = 0, c3 = 0;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__device__ __forceinline__ int choose_start(const FleetCold* cd, int E, int e, int episode) {
  if (cd->sched_n > 0) return cd->sched[(size_t)(episode % cd->sched_n) * E + e];
  int k = cd->start_lo;
  if (cd->picker_mode != FLEET_PICK_STATIC) {
    const uint32_t range = (uint32_t)(cd->start_hi - cd->start_lo + 1);
    const uint32_t x = philox_start(cd->seed, (uint32_t)(cd->env_id_offset + e), (uint32_t)episode);
    k += (int)__umulhi(x, range);
  }
  return cd->pick_rows ? cd->pick_rows[k] : k;  // candidate list of the pickers' date_range on an irregular grid
}

// 1 / x for the auxiliary slots' one division: hardware reciprocal seed (v_rcp_f64, ~26 good bits) + two Newton steps = full
// float64 accuracy (<= 1 ulp) in five instructions, against ~14 of the IEEE division sequence with its special-case handling.
__device__ __forceinline__ double rcp_newton(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}
// The same with ONE Newton step: relative error <= ~2^-44 (the seed is good to ~2^-23).  Enough wherever the result is rounded
// to float32 afterwards or feeds div_rcp's residual correction (which squares the reciprocal's error once more).
__device__ __forceinline__ double rcp_newton1(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  return fma(fma(-x, r, 1.0), r, r);
}
// x / c, IEEE-correctly rounded, from a reciprocal rc ~ 1 / c (Markstein's residual correction): q0 = x * rc is within a few
// ulp of the quotient, e = x - q0 * c is EXACT in one fma, and q0 + e * rc is the quotient to a relative 2 * |rc * c - 1|^2
// (2^-104 for a correctly rounded rc, 2^-87 for rcp_newton1) before the final rounding -- i.e. the correctly rounded quotient
// unless x / c lies that close to a rounding boundary, which no pair of float64 operands of these magnitudes does in practice
// (tests/test_capi_gpu.py::test_division_by_reciprocal_is_bit_exact: 2^30 operand pairs of the charge arithmetic's ranges
// against the IEEE sequence, 0 differences).  `v_div_fixup` restores what the three fmas lose at the edges (x = +-0, inf, NaN,
// c = 0): 5 vector instructions instead of the 11 of the IEEE division sequence, none of them quarter-rate.
__device__ __forceinline__ double div_rcp(double x, double c, double rc) {
  const double q0 = x * rc;
  const double e = fma(-q0, c, x);
  return __builtin_amdgcn_div_fixup(fma(e, rc, q0), c, x);
}

// ScoreConfig.soc_violation_penalty (score_config.py:26-30)
__device__ __forceinline__ double soc_violation_penalty(double missing) {
  return -500.0 * rcp_newton(1.0 + exp(-16.48461585 * (missing - 0.29229767))) + 1.0;  // (<= 2 ulp of the quotient)
}

// ScoreConfig.overloading_penalty (score_config.py:33-41)
__device__ __forceinline__ double overloading_penalty(double rel, double scale) {
  const double pen = (rel < 1.1) ? 0.0 : -700.0 / (1.0 + exp(-15.77350877 * (rel - 1.33298382)));
  return pen * scale;
}

}  // namespace
