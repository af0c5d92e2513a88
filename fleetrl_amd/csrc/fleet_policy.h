// fleet_policy.h -- launch shape of the policy forward (fleet_policy.hip) and the record its kernels read the network from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fleet_hip.h"

// policy_forward: 256 threads = 4 wavefronts take kPolicyRows env rows through every layer of one head.  A wavefront works on
// units of 64 output columns x R rows (R = 16, 8 or 4, the more rows the wider the layer: policy_forward), at most two at a time.
constexpr int kPolicyThreads = 256;
constexpr int kPolicyWaves = kPolicyThreads / 64;
constexpr int kPolicyRows = 16;
// the first layer's input is staged (and normalised) this many columns at a time
constexpr int kPolicyChunk = 128;
static_assert(kPolicyThreads % 64 == 0 && kPolicyThreads % kPolicyChunk == 0, "whole wavefronts, whole staging rows");
static_assert(kPolicyRows == 16 && kPolicyWaves == 4, "the unit shapes of policy_forward are written for 16 rows and 4 wavefronts");
static_assert(FLEET_POLICY_MAX_WIDTH <= 2 * kPolicyWaves * 64, "at most two 64-column units per wavefront");

// One layer as the kernels see it.  The weights are re-laid at upload as Wt[in4][out64]: input-major, `in` rounded up to a
// multiple of 4 and `out` to a multiple of 64, the padding zero; the bias as b[out64], zero-padded.  Offsets are in floats from
// the start of the handle's block.
struct PolicyLayer {
  int32_t in, out;      // as declared
  int32_t in4, out64;   // padded
  uint32_t w_off, b_off;
};
struct PolicyHeadDesc {
  int32_t n_layers, activation, output, reserved;
  float lo, hi;
  PolicyLayer layer[FLEET_POLICY_MAX_LAYERS];
};
struct PolicyDesc {
  int32_t obs_dim, n_heads;
  int32_t stride;  // floats between rows of an activation buffer in the LDS: the widest hidden layer's out64 (64 without one)
  int32_t reserved;
  PolicyHeadDesc head[FLEET_POLICY_MAX_HEADS];
};

// The warm-up's uniform draw needs no network, so its ONE launch (explore_uniform, fleet_policy.hip) is open to whoever holds a stream:
// fleet_explore_act_dev's UNIFORM mode on a policy, fleet_saccollect_uniform_dev (fleet_collect.hip) on SAC networks.  actions
// f32[E, A] and, when given, env_actions f32[E, A] receive lo + (hi - lo) * u kept below hi; u is the column's word of the Philox block
// of (seed, env0 + row, step), or noise[row][column] when `given`; without `given` a non-null noise receives u.  The caller has set
// the device and checked the arguments.  Returns hipGetLastError() of the launch.
struct PolicyUniformArgs {
  float *noise, *actions, *env_actions;
  uint64_t seed, step;
  uint32_t env0;
  int given;
  float lo, hi;
};
hipError_t policy_launch_uniform(hipStream_t stream, int E, int A, const PolicyUniformArgs& u);
