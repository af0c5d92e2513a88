// fleet_lp.h -- the linear-optimisation benchmark's per-(env, EV) planner (fleet_lp.hip), called by fleet_lp_plan_dev
// (fleet_capi.hip, the handle: fleet_batch.h).  DESIGN.md section 8 "The linear-optimisation benchmark" derives the model and the method.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "fleet_device.h"

// pieces of one row's relaxed cost r_i(delta): the lower hull of at most six candidate points
#define FLEET_LP_MAX_PIECES 5

struct FleetLpArgs {
  int H;                 // rows to plan from every env's current row
  int act_dtype;         // FLEET_ACT_F32 / FLEET_ACT_F64
  void* actions;         // [H,E,N]
  double* soc_plan;      // [H+1,E,N] or nullptr
  double* bound;         // [E]
  double* plan_cost;     // [E]
  int32_t* status;       // [E,N]
  double* scratch;       // fleet_lp_scratch_bytes(E*N, H) bytes
};

// device scratch the planner needs for E*N lanes and a horizon of H rows
size_t fleet_lp_scratch_bytes(size_t lanes, int H);
hipError_t fleet_launch_lp_plan(const FleetDev& d, const FleetLpArgs& a, hipStream_t s);
