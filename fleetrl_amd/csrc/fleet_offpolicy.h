// fleet_offpolicy.h -- constants of TD3 / DDPG's whole update on the device (fleet_offpolicy.hip): the launch shapes of the
// image-to-image Polyak update and of the closing reduction, and the shape of a per-step statistics slot.  tests/offpolicy_model.py
// restates them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fleet_hip.h"

// offpolicy_polyak / offpolicy_finish: 256 threads = 4 wavefronts; an ordered sum is 256 lane sums and a halving tree over them.
constexpr int kOffpolicyThreads = 256;
// offpolicy_polyak: one 16-byte word per thread and pass; at most kOffpolicyMaxBlocks workgroups per launch (eight per compute unit),
// which stride over the rest.
constexpr int kOffpolicyMaxBlocks = 2048;
// a slot: the critic launch's stats f32[8], then the actor launch's
constexpr int kOffpolicySlot = 16;
constexpr int kOffpolicyActorAt = 8;
constexpr int kOffpolicyMaxSteps = 65536;
static_assert(FLEET_OFFPOLICY_SLOT_FLOATS == kOffpolicySlot && FLEET_OFFPOLICY_MAX_STEPS == kOffpolicyMaxSteps, "the header states both");
static_assert(kOffpolicyThreads == 256, "the ordered sum is stated for 256 lanes");

// The actor steps of a call of G gradient steps that starts at update count `first`: step g is one iff (first + g + 1) % delay == 0.
// *g0: the first of them (they follow at a distance of `delay`); returns their number.  Host and device: the closing launch
// derives the slots that hold an actor step from its arguments.
__host__ __device__ inline uint32_t offpolicy_actor_steps(uint64_t first, uint32_t G, uint32_t delay, uint32_t* g0) {
  const uint32_t r = (uint32_t)((first % delay + 1) % delay);
  *g0 = (delay - r) % delay;
  return *g0 < G ? (G - 1 - *g0) / delay + 1 : 0;
}
