// fleet_grad_dev.h -- the device functions that the gradient launches share: PPO's (fleet_ppo.hip: ppo_rows, ppo_weights) and TD3's
// (fleet_td3.hip: td3_critic_rows, td3_actor_rows, td3_weights).  One layer of a tile forward with its activations kept, one layer of
// a tile backward, the statistics' compensated sum, and the tile loop of a weight gradient.  Everything here is inlined into the
// including kernel (an unnamed namespace: each translation unit has its own copy).  The arithmetic is the header's
// (include/fleet_hip.h "PPO minibatch gradients on the device"): forward acc = fmaf(x[k], W[j][k], acc) in ascending k, backward
// d_prev[k] = (fmaf chain over j ascending of Wt[k][j] * d[j]) * act'(h[k]), dW[j][k] = fmaf(d[b][j], x[b][k], acc) in ascending b.
// At the end, the host work the two handles share: the scratch's layout, a weights launch's entries, what both refuse about sizes.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "fleet_policy.h"
#include "fleet_policy_dev.h"

namespace {

constexpr int kGradTile = 32;  // a weights launch: a workgroup's tile of dW is 32 x 32
constexpr int kGradRows = 16;  // ... and it stages this many rows at a time

// the statistics' sums are compensated (Neumaier): s + c is the sum of the terms so far to within a rounding of the result
struct CompSum {
  float s = 0.0f, c = 0.0f;
  __device__ __forceinline__ void add(float x) {
    const float t = s + x;
    c += fabsf(s) >= fabsf(x) ? (s - t) + x : (x - t) + s;
    s = t;
  }
  __device__ __forceinline__ float value() const { return s + c; }
};

// run_layer of fleet_policy_dev.h with two changes: a hidden layer's activations also go to gact[row][out64] (rows below a.E), and a
// last layer leaves y, untransformed, in out[][] (every row and column of the tile).  kStage: where a first layer's input comes from.
template <int R, int kStage>
__device__ __forceinline__ void grad_layer(const ForwardArgs& a, const PolicyHeadDesc* H, const PolicyLayer& L, bool first, bool last,
                                           const float* in, float* out, float* xs, int S, int row0, float* gact, const StageTail& tail) {
  constexpr int kSplit = kPolicyRows / R;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int units = (L.out64 / 64) * kSplit;
  const bool has0 = w < units, has1 = w + kPolicyWaves < units;
  const int q = w % kSplit;
  const int j0 = (w / kSplit) * 64 + lane, j1 = ((w + kPolicyWaves) / kSplit) * 64 + lane;
  float acc0[R], acc1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc0[r] = acc1[r] = 0.0f;
  const float* W = a.base + L.w_off;
  if (first) {
    for (int k0 = 0; k0 < L.in; k0 += kPolicyChunk) {
      const int kn = L.in4 - k0 < kPolicyChunk ? L.in4 - k0 : kPolicyChunk;
      __syncthreads();
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
  const int activation = H->activation;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    if (!(u ? has1 : has0)) continue;
    const int j = u ? j1 : j0;
    const float b = a.base[L.b_off + j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float y = (u ? acc1[r] : acc0[r]) + b;
      const int rr = q * R + r;
      if (last) {
        out[rr * S + j] = y;
      } else {
        const float hval = hidden_act(y, activation);
        out[rr * S + j] = hval;
        if (row0 + rr < a.E) gact[(size_t)(row0 + rr) * L.out64 + j] = hval;  // (j < out64: inside the row)
      }
    }
  }
}

// every layer of one head for the tile, a barrier behind each: layer l reads `cur` and writes `nxt`, then the two swap; returns the
// buffer that holds y[16][S] of the last layer (the other one is free).  act_off[l]: layer l's activations in the scratch.
template <int kStage>
__device__ __forceinline__ float* grad_head(const ForwardArgs& a, const PolicyHeadDesc* H, float*& cur, float*& nxt, float* xs, int S, int row0,
                                            float* scratch, const uint64_t* act_off, const StageTail& tail) {
  const int n = H->n_layers;
  for (int l = 0; l < n; ++l) {
    const PolicyLayer L = H->layer[l];
    const int groups = L.out64 / 64;
    float* gact = scratch + act_off[l];
    if (groups >= 4) grad_layer<16, kStage>(a, H, L, l == 0, l == n - 1, cur, nxt, xs, S, row0, gact, tail);
    else if (groups >= 2) grad_layer<8, kStage>(a, H, L, l == 0, l == n - 1, cur, nxt, xs, S, row0, gact, tail);
    else grad_layer<4, kStage>(a, H, L, l == 0, l == n - 1, cur, nxt, xs, S, row0, gact, tail);
    __syncthreads();
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
  return cur;
}

// delta of layer l, d[16][S] in the LDS (zero past `out`) -> delta of layer l - 1 into p[16][S] (zero from `in` to the previous
// layer's out64) and, with kStore, into gdelta[row][out64 of layer l - 1]; hprev: that layer's activations in the scratch
template <bool kStore>
__device__ __forceinline__ void grad_back_layer(const float* base, const PolicyLayer& L, int prev64, int activation, const float* d, float* p,
                                                int S, int row0, int B, const float* hprev, float* gdelta) {
  const float* W = base + L.w_off;
  const int out4 = (L.out + 3) & ~3;  // (<= out64; the columns out .. out4 - 1 of Wt and of d are zero: they add +0)
  for (int k = threadIdx.x; k < prev64; k += kPolicyThreads) {
    float acc[kPolicyRows];
#pragma unroll
    for (int r = 0; r < kPolicyRows; ++r) acc[r] = 0.0f;
    if (k < L.in) {
      const float* wk = W + (size_t)k * L.out64;
      for (int j = 0; j < out4; j += 4) {
        const float4 w4 = *reinterpret_cast<const float4*>(wk + j);  // (out64 is a multiple of 64: aligned)
#pragma unroll
        for (int r = 0; r < kPolicyRows; ++r) {
          const float4 d4 = *reinterpret_cast<const float4*>(d + r * S + j);
          acc[r] = fmaf(w4.w, d4.w, fmaf(w4.z, d4.z, fmaf(w4.y, d4.y, fmaf(w4.x, d4.x, acc[r]))));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kPolicyRows; ++r) {
      const int row = row0 + r;
      float v = 0.0f;
      if (k < L.in && row < B) {
        const float hv = hprev[(size_t)row * prev64 + k];
        const float g = activation == FLEET_POLICY_ACT_RELU ? (hv > 0.0f ? 1.0f : 0.0f) : fmaf(-hv, hv, 1.0f);
        v = acc[r] * g;
        if (kStore) gdelta[(size_t)row * prev64 + k] = v;
      }
      p[r * S + k] = v;
    }
  }
}

// the delta of a head's last layer in `cur` -> every layer's delta below it, a barrier behind each; delta_off / act_off: the layers'
// arrays in the scratch
template <bool kStore>
__device__ __forceinline__ void grad_back_head(const float* base, const PolicyHeadDesc* H, float*& cur, float*& nxt, int S, int row0, int B,
                                               float* scratch, const uint64_t* act_off, const uint64_t* delta_off) {
  for (int l = H->n_layers - 1; l >= 1; --l) {
    const PolicyLayer L = H->layer[l];
    const int prev64 = H->layer[l - 1].out64;
    grad_back_layer<kStore>(base, L, prev64, H->activation, cur, nxt, S, row0, B, scratch + act_off[l - 1], scratch + delta_off[l - 1]);
    __syncthreads();
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
}

// one layer of a weights launch: dW[out][in] and db[out] from delta[B][dstride] and the layer's input.  The input's columns below
// `seam` are x[B][xstride]; with kSeam, those from `seam` on are x2[B][x2stride] (a critic's first layer: the observation, then the action)
struct GradEntry {
  const float *d, *x, *x2;
  float *dW, *db;
  int out, in, dstride, xstride, x2stride, seam, tiles_k, first;  // first: the layer's first workgroup
};

// tile `tile` of E: a thread owns 2 x 2 elements of dW, each ONE chain over the rows in ascending b, 16 rows at a time staged in the
// LDS; db[j] is the ascending sum of d[b][j], kept by the threads of the first k tile.  Stored with torch's index.
template <bool kSeam>
__device__ __forceinline__ void grad_tile(const GradEntry& E, int tile, int B, float (*ds)[kGradTile], float (*xs)[kGradTile]) {
  const int j0 = (tile / E.tiles_k) * kGradTile, k0 = (tile % E.tiles_k) * kGradTile;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  float a00 = 0.0f, a01 = 0.0f, a10 = 0.0f, a11 = 0.0f, bs0 = 0.0f, bs1 = 0.0f;
  for (int b0 = 0; b0 < B; b0 += kGradRows) {
    const int nb = B - b0 < kGradRows ? B - b0 : kGradRows;
    __syncthreads();  // the readers of the rows before are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = threadIdx.x + 256 * i;
      const int r = idx >> 5, c = idx & 31;
      float dv = 0.0f, xv = 0.0f;
      if (r < nb) {
        if (j0 + c < E.out) dv = E.d[(size_t)(b0 + r) * E.dstride + j0 + c];
        if (k0 + c < E.in) {
          if (kSeam && k0 + c >= E.seam) xv = E.x2[(size_t)(b0 + r) * E.x2stride + (k0 + c - E.seam)];
          else xv = E.x[(size_t)(b0 + r) * E.xstride + k0 + c];
        }
      }
      ds[r][c] = dv, xs[r][c] = xv;
    }
    __syncthreads();
    for (int r = 0; r < nb; ++r) {
      const float d0 = ds[r][ty], d1 = ds[r][ty + 16], x0 = xs[r][tx], x1 = xs[r][tx + 16];
      a00 = fmaf(d0, x0, a00), a01 = fmaf(d0, x1, a01), a10 = fmaf(d1, x0, a10), a11 = fmaf(d1, x1, a11);
      bs0 += d0, bs1 += d1;
    }
  }
  const int ja = j0 + ty, jb = j0 + ty + 16, ka = k0 + tx, kb = k0 + tx + 16;
  if (ja < E.out) {
    if (ka < E.in) E.dW[(size_t)ja * E.in + ka] = a00;
    if (kb < E.in) E.dW[(size_t)ja * E.in + kb] = a01;
    if (k0 == 0 && tx == 0) E.db[ja] = bs0;
  }
  if (jb < E.out) {
    if (ka < E.in) E.dW[(size_t)jb * E.in + ka] = a10;
    if (kb < E.in) E.dW[(size_t)jb * E.in + kb] = a11;
    if (k0 == 0 && tx == 0) E.db[jb] = bs1;
  }
}

// the entry whose tiles hold workgroup `bid` (entries in launch order, `first` ascending)
__device__ __forceinline__ int grad_entry_of(const GradEntry* e, int n_entries, int bid) {
  int ei = 0;
  while (ei + 1 < n_entries && bid >= e[ei + 1].first) ++ei;
  return ei;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
using GradOffsets = uint64_t[FLEET_POLICY_MAX_LAYERS];  // a net's row of a scratch's act[][] or delta[][]

// the host's half of an entry: the tiles of dW[out][in], counted on from *blocks
inline void grad_entry_tiles(GradEntry& E, int* blocks) {
  E.tiles_k = (E.in + kGradTile - 1) / kGradTile;
  E.first = *blocks;
  *blocks += ((E.out + kGradTile - 1) / kGradTile) * E.tiles_k;
}

// The scratch of n_nets nets for max_batch rows, in floats from its start: per net and layer act [max_batch][out64] (hidden layers) and
// delta [max_batch][out64] (every layer).  Raises *widest to the widest out64; returns the offset behind the last array.
inline uint64_t grad_scratch_layout(const PolicyHeadDesc* nets, int n_nets, uint64_t max_batch, GradOffsets* act, GradOffsets* delta, int* widest) {
  uint64_t off = 0;
  for (int nt = 0; nt < n_nets; ++nt)
    for (int l = 0; l < nets[nt].n_layers; ++l) {
      const uint64_t w = (uint64_t)nets[nt].layer[l].out64;
      if ((int)w > *widest) *widest = (int)w;
      if (l < nets[nt].n_layers - 1) act[nt][l] = off, off += max_batch * w;
      delta[nt][l] = off, off += max_batch * w;
    }
  return off;
}

// The entries of nets net0 .. net0 + n_nets - 1 behind e[*n_entries], layer after layer, with their gradient tensors (W, b per layer)
// from grads[] in that order.  A first layer reads x[B][xstride]; with x2, its columns from xstride on are x2[B][x2stride] (a
// critic: the observation, then the action).
inline void grad_fill_entries(GradEntry* e, int* n_entries, int* blocks, const PolicyHeadDesc* nets, int net0, int n_nets, float* scratch,
                              const GradOffsets* act, const GradOffsets* delta, const float* x, int xstride, const float* x2, int x2stride,
                              float* const* grads) {
  int ti = 0;
  for (int nt = net0; nt < net0 + n_nets; ++nt)
    for (int l = 0; l < nets[nt].n_layers; ++l, ti += 2) {
      const PolicyLayer& L = nets[nt].layer[l];
      GradEntry& E = e[(*n_entries)++];
      E.d = scratch + delta[nt][l], E.dstride = L.out64;
      E.seam = L.in;  // (one input array, but for a critic's first layer)
      if (l > 0) {
        E.x = scratch + act[nt][l - 1], E.xstride = nets[nt].layer[l - 1].out64;
      } else {
        E.x = x, E.xstride = xstride;
        if (x2) E.seam = xstride, E.x2 = x2, E.x2stride = x2stride;
      }
      E.dW = grads[ti], E.db = grads[ti + 1], E.out = L.out, E.in = L.in;
      grad_entry_tiles(E, blocks);
    }
}

// what a *_grad_dev entry refuses once it has its handle: another number of gradient tensors than `want` (`order` says which they
// are), more rows than the scratch holds.  Writes the reason into *why, which the caller hands over empty.
inline void grad_check_sizes(std::string* why, int count, int want, const char* order, int B, int max_batch) {
  if (count != want) *why = "expected " + std::to_string(want) + " gradient tensors (" + order + "), got " + std::to_string(count);
  else if (B > max_batch) *why = "B must be at most max_batch = " + std::to_string(max_batch) + ", got " + std::to_string(B);
}

}  // namespace
