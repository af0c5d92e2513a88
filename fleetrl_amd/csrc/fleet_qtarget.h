// fleet_qtarget.h -- the record the kernels of the TD3 / DDPG families read their networks from: fleet_qtarget.hip (the target launch)
// and fleet_td3.hip (the gradient launches, on the image of a fleet_qtarget handle that holds the online networks).  It opens the
// handle's device block (fleet_mlp.h); the layers' offsets count from the block's start.  The handle itself is defined here too:
// fleet_sac.hip makes one whose actor is a squashed Gaussian (fleet_sac_create), which every entry that only walks nets serves as it is.
#pragma once
#include <stdint.h>

#include "fleet_mlp.h"
#include "fleet_policy.h"

constexpr int kQNets = kMlpMaxNets;  // actor, critic 0, critic 1

struct QTargetDesc {
  int32_t obs_dim, act_dim, n_critics;
  int32_t stride;  // floats between rows of an activation buffer: the widest hidden layer's out64 over all networks (64 without one)
  int32_t act64;   // floats between rows of act[][]: the actor's last out64 (a squashed actor: act_dim rounded up to 64)
  int32_t reserved[3];  // [kQSquashed]: 1 when the actor's last layer is the 2 * act_dim wide (mu, log_std) of a squashed Gaussian
  PolicyHeadDesc net[kQNets];
};
constexpr int kQSquashed = 0;  // index into QTargetDesc::reserved

struct FleetQTarget : FleetMlpHandle {
  FleetQTargetParams p{};
  QTargetDesc desc{};
  size_t lds_bytes = 0;  // of one workgroup of qtarget_target (a squashed handle: of sac_target on its own)
};
static_assert(mlp_image_is_first_base<FleetQTarget>, "mlp_borrow (fleet_mlp.hip) reads a fleet_qtarget_handle as the image's handle");

// whether the record behind a fleet_qtarget image is a squashed-Gaussian actor's (fleet_sac_create)
inline bool qtarget_squashed(const FleetMlpHandle* img) { return static_cast<const QTargetDesc*>(img->record)->reserved[kQSquashed] != 0; }
