// fleet_policy_dev.h -- the device functions of the MLP forward that fleet_policy.hip (policy_forward, policy_forward_sample) and
// fleet_qtarget.hip (qtarget_target) share: staging the first layer's input, the accumulation chain, one layer of a tile, one head
// of a tile.  Everything here is inlined into the including kernel (an unnamed namespace: each translation unit has its own copy).
// The arithmetic is the header's chain (include/fleet_hip.h "MLP policy on the device"): acc = 0; acc = fmaf(x[k], W[j][k], acc) in
// ascending k; y = acc + b[j].
#pragma once
#include <hip/hip_runtime.h>

#include "fleet_norm.h"
#include "fleet_policy.h"

namespace {

struct ForwardArgs {
  const PolicyDesc* desc;
  const float* base;  // the block: offsets of PolicyLayer count from here
  const float* obs;
  float *actions, *values;
  const double *mean, *sd;  // the normaliser's statistics (kStageNorm)
  double clip;
  int E;
};

// where the first layer's input comes from
constexpr int kStagePlain = 0;   // obs[row][k], k < D
constexpr int kStageNorm = 1;    // ... through the normaliser's statistics
constexpr int kStageConcat = 2;  // obs[row][k] for k < d0 (row stride d0), then rows[r][k - d0] from the LDS for d0 <= k < D

// kStageConcat: the tile's rows of the columns behind the observation (the target actions of fleet_qtarget.hip)
struct StageTail {
  const float* rows;  // LDS, [kPolicyRows][stride]
  int stride;
  int d0;
};

// columns [k0, k0 + kPolicyChunk) of the tile's rows -> xs[row][col]; zeros past D and past E
template <int kStage>
__device__ __forceinline__ void stage(const ForwardArgs& a, float* xs, int row0, int k0, int D, const StageTail& tail) {
  constexpr bool kNorm = kStage == kStageNorm;
  const int col = threadIdx.x % kPolicyChunk, r0 = threadIdx.x / kPolicyChunk;
  const int k = k0 + col;
  double m = 0.0, s = 1.0;
  if (kNorm && k < D) {
    m = a.mean[k];
    s = a.sd[k];
  }
#pragma unroll
  for (int r = r0; r < kPolicyRows; r += kPolicyThreads / kPolicyChunk) {
    const int row = row0 + r;
    float v = 0.0f;
    if (kStage == kStageConcat) {
      if (k < tail.d0) {
        if (row < a.E) v = a.obs[(size_t)row * tail.d0 + k];
      } else if (k < D) {
        v = tail.rows[r * tail.stride + (k - tail.d0)];  // (k - d0 < the tail's width <= stride: inside the row)
      }
    } else if (k < D && row < a.E) {
      v = a.obs[(size_t)row * D + k];
      if (kNorm) v = fleet_norm_obs1(v, m, s, a.clip);
    }
    xs[r * kPolicyChunk + col] = v;
  }
}

// acc[r] += sum over k < kn (a multiple of 4) of xs[r][k] * W[k][j], ascending k, for column j0 (and j1 when kTwo)
template <int R, bool kTwo>
__device__ __forceinline__ void accumulate(const float* xs, int stride, int kn, const float* __restrict__ W, int O, int j0, int j1,
                                           float (&acc0)[R], float (&acc1)[R]) {
  for (int k = 0; k < kn; k += 4) {
    const float* w = W + (size_t)k * O;
    const float a0 = w[j0], a1 = w[O + j0], a2 = w[2 * O + j0], a3 = w[3 * O + j0];
    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
    if (kTwo) b0 = w[j1], b1 = w[O + j1], b2 = w[2 * O + j1], b3 = w[3 * O + j1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 x = *reinterpret_cast<const float4*>(xs + r * stride + k);  // every lane the same address
      acc0[r] = fmaf(x.w, a3, fmaf(x.z, a2, fmaf(x.y, a1, fmaf(x.x, a0, acc0[r]))));
      if (kTwo) acc1[r] = fmaf(x.w, b3, fmaf(x.z, b2, fmaf(x.y, b1, fmaf(x.x, b0, acc1[r]))));
    }
  }
}

__device__ __forceinline__ float hidden_act(float y, int activation) {
  return activation == FLEET_POLICY_ACT_RELU ? (y < 0.0f ? 0.0f : y) : tanhf(y);  // (a NaN stays one)
}

__device__ __forceinline__ float output_of(float y, int output, float lo, float hi) {
  if (output == FLEET_POLICY_OUT_CLIP) return y < lo ? lo : (y > hi ? hi : y);
  return output == FLEET_POLICY_OUT_TANH ? tanhf(y) : y;
}

// one layer for the tile: `in` -> `out` (activation buffers in the LDS, row stride S), or the staged input -> ... -> global memory;
// kSample: a last layer with `means` given -> means[16][out64] in the LDS, untransformed (every column and row of the tile: the
// padding's results are finite-or-NaN numbers nobody reads)
template <int R, int kStage, bool kSample>
__device__ __forceinline__ void run_layer(const ForwardArgs& a, const PolicyHeadDesc* H, const PolicyLayer& L, bool first, bool last,
                                          const float* in, float* out, float* xs, int S, int row0, float* gout, float* means,
                                          const StageTail& tail) {
  constexpr int kSplit = kPolicyRows / R;  // row groups per column group
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int units = (L.out64 / 64) * kSplit;
  const bool has0 = w < units, has1 = w + kPolicyWaves < units;
  const int q = w % kSplit;  // (kPolicyWaves % kSplit == 0: both units of a wavefront take the same rows)
  const int j0 = (w / kSplit) * 64 + lane, j1 = ((w + kPolicyWaves) / kSplit) * 64 + lane;
  float acc0[R], acc1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc0[r] = acc1[r] = 0.0f;
  const float* W = a.base + L.w_off;
  if (first) {
    for (int k0 = 0; k0 < L.in; k0 += kPolicyChunk) {
      const int kn = L.in4 - k0 < kPolicyChunk ? L.in4 - k0 : kPolicyChunk;
      __syncthreads();  // the readers of the chunk before are done
      stage<kStage>(a, xs, row0, k0, L.in, tail);
      __syncthreads();
      const float* x = xs + q * R * kPolicyChunk;
      const float* wk = W + (size_t)k0 * L.out64;
      if (has1) accumulate<R, true>(x, kPolicyChunk, kn, wk, L.out64, j0, j1, acc0, acc1);
      else if (has0) accumulate<R, false>(x, kPolicyChunk, kn, wk, L.out64, j0, j1, acc0, acc1);
    }
  } else if (has1) {
    accumulate<R, true>(in + q * R * S, S, L.in4, W, L.out64, j0, j1, acc0, acc1);
  } else if (has0) {
    accumulate<R, false>(in + q * R * S, S, L.in4, W, L.out64, j0, j1, acc0, acc1);
  }
  const int activation = H->activation, output = H->output;
  const float lo = H->lo, hi = H->hi;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (!(u ? has1 : has0)) continue;
    const int j = u ? j1 : j0;
    const float b = a.base[L.b_off + j];  // (padded like the columns: zero past `out`)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float y = (u ? acc1[r] : acc0[r]) + b;
      const int rr = q * R + r;
      if (!last) {
        out[rr * S + j] = hidden_act(y, activation);  // (a padding column gets act(0) = 0: the next layer's padded inputs)
      } else if (kSample && means) {
        means[rr * L.out64 + j] = y;
      } else if (j < L.out && row0 + rr < a.E) {
        gout[(size_t)(row0 + rr) * L.out + j] = output_of(y, output, lo, hi);
      }
    }
  }
}

// every layer of one head for the tile, a barrier behind each: the activations ping-pong between `cur` and `nxt` (layer l writes
// the buffer that is `nxt` on entry when l is even), the last layer goes to `gout`, or to `means` (kSample, when given)
template <int kStage, bool kSample>
__device__ __forceinline__ void run_head(const ForwardArgs& a, const PolicyHeadDesc* H, float* cur, float* nxt, float* xs, int S, int row0,
                                         float* gout, float* means, const StageTail& tail) {
  const int n = H->n_layers;
  for (int l = 0; l < n; ++l) {
    const PolicyLayer L = H->layer[l];
    const int groups = L.out64 / 64;
    if (groups >= 4) run_layer<16, kStage, kSample>(a, H, L, l == 0, l == n - 1, cur, nxt, xs, S, row0, gout, means, tail);
    else if (groups >= 2) run_layer<8, kStage, kSample>(a, H, L, l == 0, l == n - 1, cur, nxt, xs, S, row0, gout, means, tail);
    else run_layer<4, kStage, kSample>(a, H, L, l == 0, l == n - 1, cur, nxt, xs, S, row0, gout, means, tail);
    __syncthreads();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
}

}  // namespace
