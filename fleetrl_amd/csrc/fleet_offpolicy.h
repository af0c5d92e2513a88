// fleet_offpolicy.h -- constants of TD3 / DDPG's whole update on the device (fleet_offpolicy.hip): the launch shapes of the
// image-to-image Polyak update and of the closing reduction, and the shape of a per-step statistics slot.  tests/offpolicy_model.py
// restates them.  SAC's whole update (fleet_sactrain.hip) shares them, the ordered sum's tree, the Polyak launch and the host helpers below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fleet_hip.h"
#include "fleet_handle.h"
#include "fleet_mlp.h"

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

// SAC's whole update (fleet_sactrain_*): the same slot and the same two launch shapes; sactrain_scale takes one workgroup of
// kOffpolicyThreads per chunk of kSacTrainChunk consecutive elements of ONE gradient tensor, four per thread (adam_norm's shape).
constexpr int kSacTrainChunk = 1024;
static_assert(FLEET_SACTRAIN_SLOT_FLOATS == kOffpolicySlot && FLEET_SACTRAIN_MAX_STEPS == kOffpolicyMaxSteps &&
                  FLEET_SACTRAIN_SCALE_CHUNK == kSacTrainChunk && kSacTrainChunk == 4 * kOffpolicyThreads,
              "the header states all three");
struct SacTrainChunk {  // of the scale launch: elements start .. min(start + kSacTrainChunk, len) - 1 of `tensor`
  int32_t tensor;
  uint32_t start, len, reserved;
};

// The target updates of a SAC call of G gradient steps: step g updates the targets iff g % interval == 0 -- the index inside the call.
__host__ __device__ inline uint32_t sactrain_target_updates(uint32_t G, uint32_t interval) { return (G - 1) / interval + 1; }

// The actor steps of a call of G gradient steps that starts at update count `first`: step g is one iff (first + g + 1) % delay == 0.
// *g0: the first of them (they follow at a distance of `delay`); returns their number.  Host and device: the closing launch
// derives the slots that hold an actor step from its arguments.
__host__ __device__ inline uint32_t offpolicy_actor_steps(uint64_t first, uint32_t G, uint32_t delay, uint32_t* g0) {
  const uint32_t r = (uint32_t)((first % delay + 1) % delay);
  *g0 = (delay - r) % delay;
  return *g0 < G ? (G - 1 - *g0) / delay + 1 : 0;
}

// the ordered sum's tree: every thread's `v` in, the total out to every thread
__device__ inline double tree_total(double v, double* red) {
  __syncthreads();  // (the previous total has been read)
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kOffpolicyThreads / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// ---- host: what both families' entries share -------------------------------------------------------------------------------------------
inline std::string offpolicy_check_tau(double tau) {
  if (!(tau >= 0.0 && tau <= 1.0)) return "tau must be in [0, 1], got " + std::to_string(tau);
  return "";
}

// what fleet_adam_step_dev and the gradient entries refuse about one network's tensors, in their words behind `who`
inline std::string offpolicy_check_tensors(const char* who, float* const* params, float* const* grads, int count) {
  const std::string w = std::string(who) + ": ";
  if (!params) return w + "null params";
  if (!grads) return w + "null grads";
  if (count < 1 || count > kMlpMaxTensors) return w + "count must be in 1.." + std::to_string(kMlpMaxTensors) + ", got " + std::to_string(count);
  for (int i = 0; i < count; ++i) {
    if (!params[i]) return w + "parameter tensor " + std::to_string(i) + " is null";
    if (!grads[i]) return w + "gradient tensor " + std::to_string(i) + " is null";
    if (params[i] == grads[i]) return w + "parameter tensor " + std::to_string(i) + " is its own gradient";
  }
  return "";
}

// The handles this family is created on keep their definitions in their own files; what it needs of them is what their scaffolds
// share: a replay buffer's first base is FleetBufferBase<FleetReplayLayout> (fleet_handle.h), a gradient handle's and an optimiser's
// is FleetMlpUser (fleet_mlp.h), and mlp_borrow relies on the image's handle being its family's first base.
using ReplayBase = FleetBufferBase<FleetReplayLayout>;
inline const ReplayBase* replay_base(fleet_replay_handle r) { return reinterpret_cast<const ReplayBase*>(r); }
inline FleetMlpHandle* image_of(void* user) { return reinterpret_cast<FleetMlpUser*>(user)->img; }

// the staging arrays of both families' blocks, each at the next multiple of 256 bytes
enum { kStageObs, kStageAct, kStageNext, kStageDones, kStageRewards, kStageTargetQ, kStageArrays };

// The one launch of the image-to-image Polyak update `tgt` <- `img` (offpolicy_polyak, fleet_offpolicy.hip), on the targets' stream: the
// caller has seen that both images have one layout and launch on one stream.  h: the handle whose error a failure goes to.
int offpolicy_launch_polyak(FleetMlpUser* h, FleetMlpHandle* tgt, const FleetMlpHandle* img, double tau);
