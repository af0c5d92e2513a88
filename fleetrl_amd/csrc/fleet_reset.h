// fleet_reset.h -- reset of one env by its lane group, and the reset kernel.
//
// Provides: reset_ev (what each EV does for itself), reset_times and reset_head (what is done once per env), reset_env (both, for a
// group of G lanes -- also the auto-reset at the tail of a step) and fleet_reset_kernel.
// Restates of the reference: FleetEnv.reset, including the vec-env auto-reset (fleet_env/fleet_environment.py:330-434).
// Expects of its includer: kBlock (threads per workgroup, fleet_kernels.hip) is defined before this header.  Expects of its caller:
// `r` is the env head with `nsamp` unpacked (HEAD_NSAMP) and `episodes` already counting the episode that starts; only the group's
// leader lane writes the env record; `lp` is the env's data-log cursor.
#pragma once
#include "fleet_device.h"
#include "fleet_obs.h"
#include "fleet_rainflow.h"
#include "fleet_wave.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// reset of one env by its group (FleetEnv.reset, fleet_environment.py:330-434)
// ---------------------------------------------------------------------------------------------------------
// FleetEnv.reset in two parts -- what each EV of the env does for itself, and what is done once per env -- so that both lane
// parts can be placed independently (reset_env below runs them for a group of G lanes; round 5's flat-mapping experiment ran the
// env's part on another thread than its EVs').
// The EV's part (fleet_environment.py:345-399): state of health, SOC / hours_left from the start row, laxity fix-up, first SOC
// sample, the carried schedule record, the observation slots.  `log_obs_row` / `log_ev_soh`: the data log's row reset() writes.
__device__ __forceinline__ void reset_ev(const FleetDev& d, int e, int c, int start, float* __restrict__ obs_row,
                                         float* __restrict__ log_obs_row, double* __restrict__ log_ev) {
  const int N = d.N;
  const FleetCold* cd = d.cold;
  const int next = start + 1 > d.T - 1 ? d.T - 1 : start + 1;
  const EvIx ix = {(size_t)e * N, (unsigned)c};
  const size_t i = ix.flat();
  const SegRec s0 = d.seg[(size_t)start * N + c];
  d.run[i] = d.seg[(size_t)next * N + c];  // the record the first step of the episode advances to
  const RowRec tb = seg_row(s0, start, d.dt);
  const bool t090 = HOT_T090(d.hot[i].bits);  // target_soc survives reset (quirk Q7)
  const double soh = 1.0 * cd->init_soh;
  const double cap = soh * d.init_cap;
  double soc = tb.sor;
  const float hl = tb.tl;
  const double tgt = t090 ? 0.9 : d.target_soc;
  const double time_needed = (tgt - soc) * cap / d.p_avail;              // :384
  if ((hl > 0.0f) && (cd->min_laxity * time_needed > (double)hl))        // :388
    soc = tgt - (time_needed * d.p_avail / cap) / cd->min_laxity;        // :389-390
  const double soc_deg = (soc == 0.0) ? cd->def_soc : soc;               // :395-399
  d.hot[i] = hot_encode(d, ix, soc, soc_deg, hl, 1, 0, tb.there, t090, false);  // rainflow: the first sample is the first reversal point
  d.soh[i] = soh;
  if (d.deg_mode == FLEET_DEG_RAINFLOW) {  // LogDataDeg restarts; the SEI bookkeeping does NOT (quirk Q6)
    RfHdr* hp = reinterpret_cast<RfHdr*>(d.rf_rows + i * (size_t)d.rf_row_stride);
    RfHdr hd = *hp;  // rainflow_length survives
    hd.mean_sum = 0.0;
    hd.csum = 0.0;
    hd.nc = 0;
    hd.s1 = 0.0;
    hd.s2 = soc_deg;  // the stack is [soc_deg]: its only entry lives in the header
    *hp = hd;
  }
  if (obs_row) write_obs_ev(d, obs_row, c, soc, hl, tgt, tb);
  if (log_obs_row) {
    write_obs_ev(d, log_obs_row, c, soc, hl, tgt, tb);
    double* lev = log_ev + c;
    lev[0] = 0.0;
    lev[N] = 0.0;
    lev[2 * N] = 0.0;
    lev[3 * N] = soh;
  }
}
// Start row, finish row and sample count of the env's next episode (time pickers, :351-355) -- every lane of the env computes
// them for itself (registers, no exchange).
// `rf_until`: the last row of the new episode on which the degradation model runs (EnvRec::rf_until).  Without auto-reset the
// env may be stepped past its finish row (gymnasium.Env path: the reference keeps logging and evaluating, :655-671), so the
// count never stops there.
__device__ __forceinline__ int reset_times(const FleetDev& d, int e, EnvHead& r, int& rf_until) {
  const FleetCold* cd = d.cold;
  const int start = choose_start(cd, d.E, e, r.episodes);
  r.t = start;
  r.t_end = d.tab_finish ? d.tab_finish[start] : start + d.episode_steps;  // :355 (exact date match on an irregular grid)
  r.nsamp = (d.deg_mode != FLEET_DEG_NONE) ? 1 : 0;
  // the degradation model is evaluated on the rows (start, t_end] that carry FLEET_TFLAG_DEG; what is logged after the last of
  // them is cleared by the next reset() unread
  const int last = cd->tab_last_deg[r.t_end > d.T - 1 ? d.T - 1 : r.t_end];
  rf_until = (cd->rf_count_all || !d.auto_reset) ? INT32_MAX : (last > start ? last : -1);
  return start;
}
// The env's part: its record (episode counters zeroed :402-404, the head with the row flags the episode's first step needs).
__device__ __forceinline__ void reset_head(const FleetDev& d, int e, const EnvHead& r, int start, int rf_until) {
  EnvRec* er = d.env + e;
  EnvHead hd = r;
  hd.nsamp = HEAD_PACK(r.nsamp, d.tab_phys[start].flags_next, start < rf_until);
  er->h = hd;
  er->rf_until = rf_until;
  er->ep_return = 0.0;
  er->ep_len = 0;
  er->penalty_record = 0.0;
  er->start_done = start;  // bit 31 (episode.done) cleared
  // (an episode whose finish row lies beyond the table is legal until a step leaves the table: FLEET_DEVERR_TABLE_END is raised
  // there, like the KeyError of the reference's `db.loc[...]`)
}

// `lp`: the env's data-log cursor (rows written so far; only used when the log is on), advanced by the row reset() writes.
template <int G, bool LOG>
__device__ __forceinline__ void reset_env(const FleetDev& d, int e, int g, bool leader, EnvHead& r, float* __restrict__ obs_row, int& lp,
                                          int& rf_until) {
  const bool log_on = LOG && (d.log_pos != nullptr);
  const int N = d.N;
  const int start = reset_times(d, e, r, rf_until);
  // data log: the row reset() writes -- time, observation and SoH, zeros for everything else (:420-432)
  const size_t lrow = log_on ? (size_t)(lp % d.log_cap) * d.E + e : 0;
  float* const log_obs_row = log_on ? d.log_obs + lrow * d.obs_dim : nullptr;
  double* const log_ev = log_on ? d.log_ev + lrow * 4 * N : nullptr;
  for (int c = g; c < N; c += G) reset_ev(d, e, c, start, obs_row, log_obs_row, log_ev);
  if (obs_row) write_obs_tail<G>(d, obs_row, start, g);
  if (log_on) {
    write_obs_tail<G>(d, log_obs_row, start, g);
    if (leader) {
      d.log_row[lrow] = (int32_t)((uint32_t)start | 0x80000000u);
      double* le = d.log_env + lrow * 4;
      le[0] = le[1] = le[2] = le[3] = 0.0;
    }
    lp += 1;
  }
  if (leader) reset_head(d, e, r, start, rf_until);
}

template <int G>
__global__ __launch_bounds__(kBlock) void fleet_reset_kernel(FleetDev d, const uint8_t* __restrict__ mask, float* __restrict__ obs) {
  const int g = threadIdx.x % G;
  const int e = blockIdx.x * (kBlock / G) + threadIdx.x / G;
  if (e >= d.E) return;
  if (mask && !mask[e]) return;
  EnvHead r = d.env[e].h;
  r.nsamp = HEAD_NSAMP(r.nsamp);
  // an explicit reset of an episode that is in progress abandons it: count it so the next start row differs
  if (d.env[e].ep_len > 0 && d.env[e].start_done >= 0) r.episodes += 1;
  int lp = d.log_pos ? d.log_pos[e] : 0;
  int rf_until;
  reset_env<G, true>(d, e, g, g == G - 1, r, obs ? obs + (size_t)e * d.obs_dim : nullptr, lp, rf_until);
  if (d.log_pos && g == G - 1) d.log_pos[e] = lp;
}

}  // namespace
