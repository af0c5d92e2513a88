// fleet_rollout.h -- launch shapes of the rollout buffer's kernels (fleet_rollout.hip), overridable per build for measurements
// (fleetrl_amd.build.build_variant with -DFLEET_GAE_THREADS=... / -DFLEET_GAE_ROWS=...; tools/rollout_rate.py --variants).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fleet_hip.h"

// rollout_gae: lanes (= envs) per workgroup, and time rows whose loads are issued before the first of them is consumed.
// Chosen by measurement at E = 4096, K = 192.
#ifndef FLEET_GAE_THREADS
#define FLEET_GAE_THREADS 64
#endif
#ifndef FLEET_GAE_ROWS
#define FLEET_GAE_ROWS 16
#endif
static_assert(FLEET_GAE_THREADS % 64 == 0 && FLEET_GAE_THREADS >= 64 && FLEET_GAE_THREADS <= 1024, "whole wavefronts");
static_assert(FLEET_GAE_ROWS >= 1 && FLEET_GAE_ROWS <= 64, "rows in flight per lane: three registers each");

// rollout_add / rollout_gather: 256 threads, grid-stride, at most this many workgroups (8 per CU)
constexpr int kRolloutThreads = 256;
constexpr int kRolloutMaxBlocks = 2048;
