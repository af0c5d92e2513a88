// fleet_aux_kernels.h -- the small kernels beside step and reset: none of them is on the hot path.
//
// Provides: fleet_dist_factor_kernel, fleet_gather_field_kernel (fleet_get), fleet_term_scan_kernel / fleet_term_gather_kernel (the
// host path's compacted terminal observations) and the two self-test kernels of div_rcp and cycle_stress.
// Restates of the reference: FleetEnv.get_dist_factor (fleet_env/fleet_environment.py:782-799); the rest has no counterpart there.
// Expects of its caller: the launch geometry of fleet_step_plan.h (fleet_term_scan_kernel is ONE workgroup of 1024 threads; the
// others are flat over E * N or grid-stride).
#pragma once
#include "fleet_device.h"
#include "fleet_obs.h"
#include "fleet_rainflow.h"
#include "fleet_wave.h"

namespace {

// FleetEnv.get_dist_factor (fleet_environment.py:782-799)
__global__ void fleet_dist_factor_kernel(FleetDev d, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)d.E * d.N) return;
  const int e = (int)(i / d.N), c = (int)(i % d.N);
  const int t = d.env[e].h.t;
  const RowRec tb = seg_row(d.seg[(size_t)t * d.N + c], t, d.dt);
  const double th = (double)tb.there;
  const double tgt = HOT_T090(d.hot[i].bits) ? 0.9 : d.target_soc;
  const double cl = tgt * th - tb.sor;
  const double hn = cl * d.cold->batt_cap_nominal / d.cold->hn_denominator;
  out[i] = hn / ((double)tb.tl + 0.001);
}

// fleet_get: unpack one field into a contiguous buffer (types as documented in include/fleet_hip.h)
__global__ void fleet_gather_field_kernel(FleetDev d, int field, void* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t E = d.E, EN = (size_t)d.E * d.N;
  const bool per_car = field == FLEET_F_SOC || field == FLEET_F_HOURS_LEFT || field == FLEET_F_SOH || field == FLEET_F_SOC_DEG ||
                       field == FLEET_F_TARGET_SOC || field == FLEET_F_RF_LEN || field == FLEET_F_RF_CYCLES || field == FLEET_F_RF_STACK ||
                       field == FLEET_F_FD_CYC ||
                       field == FLEET_F_FD_CAL || field == FLEET_F_SEI_L;
  if (i >= (per_car ? EN : E)) return;
  switch (field) {
    case FLEET_F_SOC: ((double*)out)[i] = HOT_SOC(d.hot[i]); break;
    case FLEET_F_HOURS_LEFT: ((float*)out)[i] = d.hot[i].hl; break;
    case FLEET_F_SOH: ((double*)out)[i] = d.soh[i]; break;
    case FLEET_F_SOC_DEG: ((double*)out)[i] = HOT_INPLANE(d.hot[i].bits) ? d.soc_deg[i] : d.hot[i].x; break;
    case FLEET_F_TARGET_SOC: ((double*)out)[i] = HOT_T090(d.hot[i].bits) ? 0.9 : d.target_soc; break;
    case FLEET_F_RF_LEN:
      ((int32_t*)out)[i] = d.rf_rows ? reinterpret_cast<const RfHdr*>(d.rf_rows + i * (size_t)d.rf_row_stride)->rf_len : 1;
      break;
    case FLEET_F_RF_CYCLES:
      ((int32_t*)out)[i] = d.rf_rows ? reinterpret_cast<const RfHdr*>(d.rf_rows + i * (size_t)d.rf_row_stride)->nc : 0;
      break;
    case FLEET_F_RF_STACK: ((int32_t*)out)[i] = d.rf_rows ? HOT_TAIL(d.hot[i].bits) : 0; break;
    case FLEET_F_FD_CYC: ((double*)out)[i] = d.sei[i].fd_cyc; break;
    case FLEET_F_FD_CAL: ((double*)out)[i] = d.sei[i].fd_cal; break;
    case FLEET_F_SEI_L: ((double*)out)[i] = d.sei[i].sei_l; break;
    case FLEET_F_TIME_IDX: ((int32_t*)out)[i] = d.env[i].h.t; break;
    case FLEET_F_START_IDX: ((int32_t*)out)[i] = d.env[i].start_done & 0x7FFFFFFF; break;
    case FLEET_F_CASHFLOW: ((double*)out)[i] = d.env[i].cashflow; break;
    case FLEET_F_EP_RETURN: ((double*)out)[i] = d.env[i].ep_return; break;
    case FLEET_F_EP_LEN: ((int32_t*)out)[i] = d.env[i].ep_len; break;
    case FLEET_F_LAST_EP_RETURN: ((double*)out)[i] = d.env[i].last_ep_return; break;
    case FLEET_F_LAST_EP_LEN: ((int32_t*)out)[i] = d.cold->last_len[i]; break;
    case FLEET_F_LAST_EP_LEN_F64: ((double*)out)[i] = (double)d.cold->last_len[i]; break;
    case FLEET_F_RF_UNTIL: ((int32_t*)out)[i] = d.env[i].rf_until; break;
    case FLEET_F_ERROR_BITS: ((uint32_t*)out)[i] = d.env[i].err; break;
    case FLEET_F_DONE: ((uint8_t*)out)[i] = (uint8_t)(d.env[i].start_done < 0); break;
    case FLEET_F_EPISODES: ((int32_t*)out)[i] = d.env[i].h.episodes; break;
    case FLEET_F_PENALTY_RECORD: ((double*)out)[i] = d.env[i].penalty_record; break;
    default: break;
  }
}

// Host path: the terminal observations of the envs that finished in this step, compacted (fleet_step_host moves only these
// rows over PCIe instead of the whole [E, obs_dim] buffer).  One workgroup: a serial-over-chunks scan of the done flags in
// env order (deterministic), then the rows are copied by the whole launch.
__global__ __launch_bounds__(1024) void fleet_term_scan_kernel(const uint8_t* __restrict__ done, int E, int32_t* __restrict__ idx,
                                                               int32_t* __restrict__ count, const EnvRec* __restrict__ env,
                                                               const FleetCold* __restrict__ cold, double* __restrict__ ep_ret,
                                                               int32_t* __restrict__ ep_len) {
  __shared__ int s_wave[16];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int e0 = 0; e0 < E; e0 += 1024) {
    const int e = e0 + (int)threadIdx.x;
    const bool f = (e < E) && done[e] != 0;
    const unsigned long long m = __ballot(f);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (f) {  // the finished episode's return / length travel with the index (what SB3's Monitor would report)
      idx[off + before] = e;
      ep_ret[off + before] = env[e].last_ep_return;
      ep_len[off + before] = cold->last_len[e];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int w = 0; w < 16; ++w) tot += s_wave[w];
      s_base += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = s_base;
}

__global__ void fleet_term_gather_kernel(const float* __restrict__ term, int obs_dim, const int32_t* __restrict__ idx,
                                         const int32_t* __restrict__ count, float* __restrict__ compact) {
  const int n = *count;
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const float* src = term + (size_t)idx[k] * obs_dim;
    float* dst = compact + (size_t)k * obs_dim;
    for (int j = threadIdx.x; j < obs_dim; j += blockDim.x) dst[j] = src[j];
  }
}

// Self-test of div_rcp (fleet_selftest_division): operand pairs drawn the way the charge arithmetic forms them, the IEEE division
// sequence beside the reciprocal form, bit for bit.  case 0: need / eta_c with the host's correctly rounded 1 / eta_c;
// case 1: energy / cap with rcp_newton1(cap).  A few lanes in a thousand carry the edge values (+-0, a denormal-sized residue).
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double u01(unsigned long long h) { return (double)(h >> 11) * (1.0 / 9007199254740992.0); }
__global__ void fleet_selftest_division_kernel(unsigned long long n, unsigned long long seed, unsigned long long* __restrict__ bad) {
  unsigned long long b0 = 0, b1 = 0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long h = mix64(seed + i * 4ull);
    const double soc = -0.25 + 1.5 * u01(h), soh = 0.8 + 0.2 * u01(mix64(h)), init_cap = 10.0 + 90.0 * u01(mix64(h + 1));
    const double eta = 0.5 + 0.5 * u01(mix64(h + 2)), tgt = (h & 1) ? 0.85 : 0.9;
    const double a = 2.0 * u01(mix64(h + 3)) - 1.0, p_avail = 2.0 + 20.0 * u01(mix64(h + 4));
    const double cap = soh * init_cap;
    double need = (tgt - soc) * cap;
    double en = p_avail * a * 0.25;
    const unsigned sel = (unsigned)(h >> 40) % 1000u;
    if (sel == 0) need = 0.0;
    if (sel == 1) need = -0.0;
    if (sel == 2) en = -0.0;
    if (sel == 3) en = 7e-18 * cap;
    const double inv_eta = 1.0 / eta;  // IEEE: correctly rounded, like the host's
    const double q0 = need / eta, r0 = div_rcp(need, eta, inv_eta);
    const double x1 = (a >= 0.0) ? en * eta : en;
    const double q1 = x1 / cap, r1 = div_rcp(x1, cap, rcp_newton1(cap));
    b0 += (__double_as_longlong(q0) != __double_as_longlong(r0));
    b1 += (__double_as_longlong(q1) != __double_as_longlong(r1));
  }
  if (b0) atomicAdd(bad, b0);
  if (b1) atomicAdd(bad + 1, b1);
}

// cycle_stress (hardware float32 log2 inside x^-0.501, Taylor exp) against the same expression in library double precision, on n
// pseudo-random (range, mean, weight) triples of the reachable domain: worst[0] = largest relative difference as the bits of a double
__global__ void fleet_selftest_stress_kernel(unsigned long long n, unsigned long long seed, unsigned long long* __restrict__ worst) {
  double w = 0.0;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long h = mix64(seed + i * 3ull);
    // depth of discharge: half of the samples log-uniform over 1e-9 ... 1 (tiny cycles are the common ones), half uniform
    const double u = u01(h), v = u01(mix64(h + 1));
    const double rng = (h & 1) ? exp(-20.7232658 * u) : u;
    const double mean = -0.25 + 1.5 * v;  // a mean SOC a little outside [0, 1] too (quirk Q9: the reference does not clip it)
    const double count = (h & 2) ? 1.0 : 0.5;
    const double st = 0.9 + 0.2 * u01(mix64(h + 2));
    const double got = cycle_stress(rng, mean, count, st);
    double eff = rng * count;
    eff = eff > 1.0 ? 1.0 : eff;
    const double want = (eff > 0.0) ? (1.0 / (1.4E5 * pow(eff, -0.501) + -1.23E5)) * exp(1.04 * (mean - 0.5)) * st : 0.0;
    const double rel = (want != 0.0) ? fabs(got - want) / fabs(want) : fabs(got);
    w = rel > w ? rel : w;
  }
  atomicMax(worst, (unsigned long long)__double_as_longlong(w));  // non-negative doubles order like their bit patterns
}

}  // namespace
