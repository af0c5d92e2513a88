// fleet_replay.h -- launch shapes of the replay buffer's kernels (fleet_replay.hip), overridable per build for measurements
// (fleetrl_amd.build.build_variant with -DFLEET_REPLAY_LDS=0 / -DFLEET_REPLAY_MAX_BLOCKS=...; tools/replay_rate.py --variants).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fleet_hip.h"

// replay_add / replay_sample: 256 threads = 4 wavefronts, one wavefront per env row (add) or per sample (sample), grid-stride,
// at most this many workgroups (8 per CU): the statistics a workgroup stages into the LDS serve every sample it takes.
constexpr int kReplayThreads = 256;
constexpr int kReplayWaves = kReplayThreads / 64;
#ifndef FLEET_REPLAY_MAX_BLOCKS
#define FLEET_REPLAY_MAX_BLOCKS 2048
#endif
constexpr int kReplayMaxBlocks = FLEET_REPLAY_MAX_BLOCKS;
// replay_sample stages mean[D] and sd[D] (float64) into the LDS once per workgroup when they fit this many bytes; 0: never
#ifndef FLEET_REPLAY_LDS
#define FLEET_REPLAY_LDS 1
#endif
constexpr size_t kReplayLdsBytes = FLEET_REPLAY_LDS ? 48 * 1024 : 0;
static_assert(kReplayThreads % 64 == 0, "whole wavefronts");
