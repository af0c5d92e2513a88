// fleet_logsum.h -- the reduction of the data-log ring to the evaluation's numbers (fleet_logsum.hip), called by
// fleet_log_summary_dev (fleet_capi.hip, the handle: fleet_batch.h).  DESIGN.md "The data log, summarised on the device" has the
// layout, the summation order and the two launches; tests/logsum_model.py restates them in NumPy.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fleet_device.h"

constexpr int kLogsumRows = 64;       // rows of one block partial: one wavefront per (env, block)
constexpr int kLogsumMaxBins = 256;   // histogram bins a call may ask for
constexpr int kLogsumFoldThreads = 256;

// What the two launches need beside the ring itself (FleetDev): the call's arguments, checked by the entry, and the scratch.
struct FleetLogsumArgs {
  int drop_last, bins, hist_ev;
  int calc_deg;          // FleetParams.deg_mode != FLEET_DEG_NONE
  int minutes_per_step;  // of a regular grid; 0: no time-of-day profile
  double lo, hi;         // histogram range
  double price_multiplier;
  const uint16_t* tab_hm;  // [T] hour << 8 | minute (FleetCold::tab_hm)
  double* scal;            // [E,8]
  double* deg_sum;         // [E,N] or nullptr
  double* soh_last;        // [E,N] or nullptr
  double* prof_sum;        // [E,S] or nullptr
  int32_t* prof_cnt;       // [E,S] or nullptr
  int32_t* hist;           // [E,bins] or nullptr
  void* scratch;           // fleet_logsum_scratch_bytes(E, N, log_cap) bytes
};

// the block partials of every (env, 64-row block) of a full ring: 8 scalars, N degradation sums, 64 row powers and slots, 256 bins
size_t fleet_logsum_scratch_bytes(int E, int N, int log_cap);
hipError_t fleet_launch_log_summary(const FleetDev& d, const FleetLogsumArgs& a, hipStream_t s);
