// fleet_qtarget.h -- the record the kernels of the TD3 / DDPG families read their networks from: fleet_qtarget.hip (the target launch)
// and fleet_td3.hip (the gradient launches, on the image of a fleet_qtarget handle that holds the online networks).  It opens the
// handle's device block (fleet_mlp.h); the layers' offsets count from the block's start.
#pragma once
#include <stdint.h>

#include "fleet_mlp.h"
#include "fleet_policy.h"

constexpr int kQNets = kMlpMaxNets;  // actor, critic 0, critic 1

struct QTargetDesc {
  int32_t obs_dim, act_dim, n_critics;
  int32_t stride;  // floats between rows of an activation buffer: the widest hidden layer's out64 over all networks (64 without one)
  int32_t act64;   // floats between rows of act[][]: the actor's last out64
  int32_t reserved[3];
  PolicyHeadDesc net[kQNets];
};
