// fleet_collect.h -- constants of the rollout collection on the device (fleet_collect.hip): the launch shapes of the episode ring's
// scan and of the closing reduction, and the ring's slot rule, stated once for host and device.  tests/collect_model.py restates them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fleet_hip.h"

// collect_episodes: ONE workgroup of 1024 threads = 16 wavefronts takes the envs in chunks of 1024, in env order.
constexpr int kCollectScanThreads = 1024;
constexpr int kCollectScanWaves = kCollectScanThreads / 64;
// collect_finish: 256 threads = 4 wavefronts; an ordered sum is 256 lane sums and a halving tree over them.
constexpr int kCollectThreads = 256;
constexpr int kCollectMaxWindow = 4096;
constexpr int kCollectStats = 16;
static_assert(FLEET_COLLECT_MAX_WINDOW == kCollectMaxWindow && FLEET_COLLECT_STATS == kCollectStats, "the header states both");
static_assert(kCollectThreads == 256 && kCollectScanThreads == 1024, "the ordered sum is stated for 256 lanes, the scan for chunks of 1024");

// The k-th finished env of a step with c finished envs (k = 0 .. c - 1, ascending env id), the ring having taken `count` episodes
// before the step: it is kept iff c - k <= W -- only the last W of a step survive, so no two of them share a slot -- and then lies
// in slot (count + k) % W.  What collections.deque(maxlen = W).extend does with the step's episodes in env order.
__host__ __device__ inline bool collect_slot(uint64_t count, uint32_t c, uint32_t k, uint32_t W, uint32_t* slot) {
  *slot = (uint32_t)((count + k) % W);
  return c - k <= W;
}
