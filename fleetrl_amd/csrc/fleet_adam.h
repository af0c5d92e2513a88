// fleet_adam.h -- launch shapes of the Adam step on a weight image (fleet_adam.hip) and the tables its two kernels read: built once
// at create, kept in the handle's device block behind the state, never written again.
#pragma once
#include <stdint.h>

#include "fleet_mlp.h"

// adam_norm: one workgroup of kAdamThreads per chunk of kAdamChunk consecutive elements of ONE tensor, four per thread
constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = 1024;
// adam_step: one workgroup per work item -- a kAdamTile x kAdamTile tile of a W, or kAdamChunk elements of a bias or an extra
constexpr int kAdamTile = 32;
constexpr int kAdamMaxTensors = kMlpMaxTensors + FLEET_ADAM_MAX_EXTRA;
static_assert(kAdamChunk == 4 * kAdamThreads, "four consecutive elements per thread in the norm, four strided ones in a flat piece");
static_assert(kAdamTile * kAdamTile == 4 * kAdamThreads && kAdamThreads % kAdamTile == 0, "a tile is four passes of 8 rows of 32 lanes");

// One tensor the optimiser owns.  A W is [out][in] on torch's side and Wt[in4][out64] at img_off in the image; a bias is b[out] on
// both sides; an extra has no image.  Its exp_avg lies at state_off floats from the block's start, its exp_avg_sq n_elements behind.
constexpr int kAdamMatrix = 0, kAdamBias = 1, kAdamExtra = 2;
struct AdamTensor {
  int32_t kind, out, in, out64;  // (out: the length of a bias or an extra; in = 1 there)
  uint32_t img_off, len;         // floats from the image's start; out * in
  uint64_t state_off;
};
struct AdamChunk {  // of the norm launch: elements start .. min(start + kAdamChunk, len) - 1 of `tensor`
  int32_t tensor;
  uint32_t start;
};
struct AdamItem {  // of the step launch: the tile at rows j0, columns k0 of a W; the piece at j0 of a flat tensor
  int32_t tensor;
  uint32_t j0, k0, reserved;
};
