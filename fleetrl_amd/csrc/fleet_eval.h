// fleet_eval.h -- constants of the agent's evaluation on the device (fleet_eval.hip): the launch shapes of the bookkeeping scan, of the
// closing reduction and of the snapshot's copy.  tests/eval_model.py restates them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fleet_hip.h"

// eval_episodes: ONE workgroup of 1024 threads = 16 wavefronts takes the envs in chunks of 1024, in env order.
constexpr int kEvalScanThreads = 1024;
constexpr int kEvalScanWaves = kEvalScanThreads / 64;
// eval_finish: 256 threads = 4 wavefronts; an ordered sum is 256 lane sums and a halving tree over them.
constexpr int kEvalThreads = 256;
constexpr int kEvalMaxEpisodes = 65536;
constexpr int kEvalStats = 16;
// eval_snapshot / the snapshot's way back: 256 threads per workgroup, four floats per thread and turn, at most this many workgroups
constexpr int kEvalCopyMaxBlocks = 1024;
static_assert(FLEET_EVAL_MAX_EPISODES == kEvalMaxEpisodes && FLEET_EVAL_STATS == kEvalStats, "the header states both");
static_assert(kEvalThreads == 256 && kEvalScanThreads == 1024, "the ordered sum is stated for 256 lanes, the scan for chunks of 1024");
