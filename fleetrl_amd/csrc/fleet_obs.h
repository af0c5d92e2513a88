// fleet_obs.h -- addressing and store helpers of the per-EV state, and the observation writers.
//
// Provides: the store flavours (st_obs non-temporal, st_rec16, st_plain) and at_off (uniform base + 32-bit lane offset); EvIx /
// ev_at / rf_row_of (one EV of one env in the [E, N] planes and in the rainflow rows); RowRec / seg_row (the three schedule columns
// of a row, decoded from the carried segment record: struct SegRec in fleet_device.h); write_obs_ev and tail_load / tail_store /
// write_obs_tail (layout: DESIGN.md "Observation row").
// Restates of the reference: Observer*.get_obs and Unit / OracleNormalization.normalize_obs (utils/observation/observer_*.py,
// utils/normalization/*.py).  The four table-derived auxiliary slots are computed per lane from the carried record (one
// reciprocal, no division).
// Expects of its caller: `tb` of write_obs_ev is the TABLE row the step advanced to (quirk Q10); tail_load is issued early, with the
// other time-row loads, and tail_store late; a byte offset handed to at_off stays below 4 GiB (fleet_create checks).
#pragma once
#include "fleet_device.h"
#include "fleet_wave.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// observation assembly (observer_*.py + normalization/*.py); layout: DESIGN.md "Observation row"
// ---------------------------------------------------------------------------------------------------------
typedef float fleet_v4f __attribute__((ext_vector_type(4)));
// Observation rows are written once and read by nobody on the chip: non-temporal stores (-1.5 % per launch, r03 ab_nt.log).
// Everything else is stored plain: write-through (`sc1`) and non-temporal state stores were measured on every class of store
// and lose everywhere (profiles/r03_experiments/ab_stores.log).
__device__ __forceinline__ void st_obs(float* p, float v) { __builtin_nontemporal_store(v, p); }
template <typename T>
__device__ __forceinline__ void st_rec16(T* p, const T& v) {  // a 16-byte record as ONE store
  static_assert(sizeof(T) == 16, "16-byte record");
  fleet_v4f w;
  __builtin_memcpy(&w, &v, 16);
  *reinterpret_cast<fleet_v4f*>(p) = w;
}
// base + 32-bit byte offset.  The offset is made opaque at every use: its 64-bit zero-extension must be formed in the basic
// block of the access for the instruction selector to see "uniform base + 32-bit lane offset" (scalar-base addressing); a
// zero-extension hoisted into an earlier block arrives as an anonymous 64-bit vector value and costs a 64-bit vector add.
// (in place: the caller's variable is the one register all its uses share)
template <typename T>
__device__ __forceinline__ T* at_off(T* base, unsigned& byte_off) {
  asm volatile("" : "+v"(byte_off));
  return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byte_off);
}
template <typename T>
__device__ __forceinline__ const T* at_off(const T* base, unsigned& byte_off) {
  asm volatile("" : "+v"(byte_off));
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}
template <typename T>
__device__ __forceinline__ void st_plain(T* p, const T& v) { *p = v; }
__device__ __forceinline__ void st_obs_at(float* base, unsigned& byte_off, float v) { st_obs(at_off(base, byte_off), v); }

// One EV of one env: the planes [E, N] are addressed as (plane + e * N) + c -- the first part is wave-uniform when a
// wavefront is one env (G == 64) and lives in scalar registers.
struct EvIx {
  size_t eN;   // e * N
  unsigned c;  // EV of the env
  __device__ __forceinline__ size_t flat() const { return eN + c; }
};
template <typename T>
__device__ __forceinline__ T* ev_at(T* plane, const EvIx& ix) {
  unsigned off = ix.c * (unsigned)sizeof(T);
  return at_off(plane + ix.eN, off);
}
// the EV's rainflow row (row stride in float64 words; one env's rows stay below 4 GiB: fleet_create checks)
__device__ __forceinline__ double* rf_row_of(const FleetDev& d, const EvIx& ix, unsigned word = 0) {
  unsigned off = (ix.c * (unsigned)d.rf_row_stride + word) * 8u;
  return at_off(d.rf_rows + ix.eN * (size_t)d.rf_row_stride, off);
}

// The three schedule columns of one (row, EV), decoded from the record of the row's segment.
struct RowRec {
  double sor;      // db["SOC_on_return"]
  float tl;        // db["time_left"]
  uint32_t there;  // db["There"]
};
__device__ __forceinline__ RowRec seg_row(const SegRec& s, int r, double dt) {
  RowRec o;
  o.sor = s.sor;
  o.tl = seg_tl(s, r, dt);
  o.there = SEG_THERE(s.se);
  return o;
}

// Per-EV slots of EV c.  soc / hours_left come from live state; the five auxiliary slots from the TABLE row the step
// advanced to (quirk Q10): there | target_soc * there | charging_left | hours_needed | laxity (observer_bl_pv.py:85-91), each
// divided by the normaliser's constant when normalize_in_env (oracle_normalization.py:127-131).  They are computed per lane
// from the carried schedule record in float64 and rounded to float32 like the reference's; `cl * cap / (evse * eta)` and the
// normaliser's divisions are multiplications by the correctly rounded quotient / reciprocal and `time_left / (hours_needed +
// 0.001)` uses rcp_newton: <= 2 ulp of float64 before the rounding to float32, i.e. the float32 word is the reference's
// except when the float64 value lies within ~2e-16 relative of a rounding boundary (tests/test_hip_parity.py reports the
// exact-match fraction; the north-star tolerance is 1e-5).  Round 3 read these four words from a [T, N] table: 16 bytes per EV
// and step, 7 of a wavefront's 44 line requests; the two float64 divisions that had made the per-lane form lose in round 3
// (ab_seg3.log) are gone.
__device__ __forceinline__ void write_obs_ev(const FleetDev& d, float* __restrict__ row, int c, double soc, float hl, double tgt,
                                             const RowRec& tb) {
  const int N = d.N;
  // one 32-bit lane offset for all seven slots; the slot arrays' bases are wave-uniform when a wavefront is one env (scalar
  // registers, `global_store ... s[base]` addressing: no 64-bit vector address per slot)
  unsigned o4 = (unsigned)c * 4u;
  st_obs_at(row, o4, (float)soc);
  st_obs_at(row + N, o4, d.normalize ? (float)((double)hl / d.self->max_time_left) : hl);
  if (!d.aux) return;
  float* a = row + 2 * N + d.tail_a_len;
  const double th = (double)tb.there;
  const double tgt_th = tgt * th;
  const double cl = tgt_th - tb.sor;
  const double hn = cl * d.hn_scale;
  double lax = ((double)tb.tl * rcp_newton1(hn + 0.001) - 1.0) * th;
  lax = lax < 0.0 ? 0.0 : (lax > 5.0 ? 5.0 : lax);  // np.clip(., 0, 5): keeps -0.0 (an absent EV) and NaN like numpy does
  st_obs_at(a, o4, (float)tb.there);
  if (d.normalize) {
    const FleetCold* cd = d.self->cold;
    st_obs_at(a + N, o4, (float)(tgt_th * cd->inv_max_soc));
    st_obs_at(a + 2 * N, o4, (float)(cl * cd->inv_max_soc));
    st_obs_at(a + 3 * N, o4, (float)(hn * cd->inv_max_hours_needed));
    st_obs_at(a + 4 * N, o4, (float)(lax * cd->inv_max_laxity));
  } else {
    st_obs_at(a + N, o4, (float)tgt_th);
    st_obs_at(a + 2 * N, o4, (float)cl);
    st_obs_at(a + 3 * N, o4, (float)hn);
    st_obs_at(a + 4 * N, o4, (float)lax);
  }
}

// env-level blocks: a pure function of the table row, pre-assembled (and pre-normalised) on the host.  Lane j copies
// tail float j to its slot (block A right after the 2N state slots, block B after the 5N auxiliary slots).  The load
// is issued early (with the other time-row loads) and the store late: `tail_load` / `tail_store`; for the usual
// sizes (<= G floats) that is one predicated load and one store per lane, no loop.
template <int G>
__device__ __forceinline__ float tail_load(const FleetDev& d, int t, int g) {
  const int total = d.tail_a_len + d.tail_b_len;
  return (g < total) ? d.tab_tail[(size_t)t * d.tail_stride + g] : 0.0f;
}

template <int G>
__device__ __forceinline__ void tail_store(const FleetDev& d, float* __restrict__ row, int t, int g, float first) {
  const float* __restrict__ src = d.tab_tail + (size_t)t * d.tail_stride;
  const int na = d.tail_a_len, total = d.tail_a_len + d.tail_b_len;
  const unsigned base_a = 2u * (unsigned)d.N, base_b = 7u * (unsigned)d.N;  // block B: 2N + na + 5N + (j - na) = 7N + j
  int j = g;
  if (j < total) st_obs(row + ((j < na ? base_a : base_b) + (unsigned)j), first);
  if (total > G) {
    for (j += G; j < total; j += G) row[(j < na ? base_a : base_b) + (unsigned)j] = src[j];
  }
}

template <int G>
__device__ __forceinline__ void write_obs_tail(const FleetDev& d, float* __restrict__ row, int t, int g) {
  tail_store<G>(d, row, t, g, tail_load<G>(d, t, g));
}

}  // namespace
