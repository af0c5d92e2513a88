// fleet_sac_dev.h -- the device function that every launch of a squashed-Gaussian actor shares: the epilogue behind the actor's last
// layer (include/fleet_hip.h "SAC on the device").  fleet_sac.hip runs it in sac_act and sac_target, fleet_td3.hip in sac_actor_rows
// (the actor gradient), so the action, the recorded noise and the log-probability of a row are the same bits under one key wherever
// they are formed.  Inlined into the including kernel (an unnamed namespace: each translation unit has its own copy).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fleet_philox.h"
#include "fleet_policy.h"

namespace {

// what the epilogue needs beside the forward's arguments (include/fleet_hip.h FleetSacActArgs)
struct SacEpilogue {
  float *noise, *actions, *gaussian, *log_prob, *mean, *log_std;
  uint64_t seed, step;
  uint32_t id0;  // global id of row 0
  int given, deterministic;
};

// hd[16][M2]: the actor's last layer, columns j (mu) and A + j (log_std) -> the outputs of rows row0 .. row0 + 15 below E; `act`
// (LDS, [16][M], or NULL) receives the squashed action, zeros in the rows past E; `rowlp` (LDS, [16], or NULL) the log-probability.
// The terms t replace mu and the corrections c replace log_std in place, and are summed per row behind a barrier.
// `keep` (LDS, [16][Mk], or NULL; not with deterministic) receives what a backward pass needs and the terms overwrite: eps in column
// j and the UNCLAMPED l in column A + j, of the rows below E.
__device__ __forceinline__ void sac_epilogue(const SacEpilogue& x, float* hd, int M2, int A, int E, int row0, float* act, int M, float* rowlp,
                                             float* keep, int Mk) {
  const int nb = (A + 3) / 4;  // Philox blocks per row
  for (int item = threadIdx.x; item < kPolicyRows * nb; item += kPolicyThreads) {
    const int r = item / nb, b = item - r * nb;
    const int row = row0 + r;
    if (row >= E) {
      if (act)
        for (int j = 4 * b; j < 4 * b + 4 && j < A; ++j) act[r * M + j] = 0.0f;  // (the critics run on them and nobody reads the result)
      continue;
    }
    const size_t o = (size_t)row * A;
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!x.deterministic) row_normals4(x.given, x.noise, o, b, A, x.id0 + (uint32_t)row, x.step, x.seed, z);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = 4 * b + c;
      if (j >= A) break;
      const float m = hd[r * M2 + j], l = hd[r * M2 + A + j];
      const float ls = l < -20.0f ? -20.0f : (l > 2.0f ? 2.0f : l);
      if (x.mean) x.mean[o + j] = m;
      if (x.log_std) x.log_std[o + j] = ls;
      float av;
      if (x.deterministic) {
        av = tanhf(m);
      } else {
        const float eps = z[c];
        if (!x.given && x.noise) x.noise[o + j] = eps;
        if (keep) keep[r * Mk + j] = eps, keep[r * Mk + A + j] = l;
        const float sd = expf(ls);
        const float u = fmaf(sd, eps, m);
        av = tanhf(u);
        if (x.gaussian) x.gaussian[o + j] = u;
        hd[r * M2 + j] = fmaf(-0.5f * eps, eps, -ls) - 0.9189385332f;
        hd[r * M2 + A + j] = logf((1.0f - av * av) + 1e-6f);
      }
      if (x.actions) x.actions[o + j] = av;  // (required by fleet_sac_act_dev; the target's next_actions is optional)
      if (act) act[r * M + j] = av;
    }
  }
  if (x.deterministic || (!x.log_prob && !rowlp)) return;  // (uniform over the launch)
  __syncthreads();
  // a wavefront sums 4 rows: every lane its columns lane, lane + 64, ... in ascending order, then a butterfly over the 64 lanes
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = w * (kPolicyRows / kPolicyWaves); r < (w + 1) * (kPolicyRows / kPolicyWaves); ++r) {
    float st = 0.0f, sc = 0.0f;
    for (int j = lane; j < A; j += 64) {
      st += hd[r * M2 + j];
      sc += hd[r * M2 + A + j];
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      st += __shfl_xor(st, d, 64);
      sc += __shfl_xor(sc, d, 64);
    }
    const float lp = st - sc;
    if (lane == 0) {
      if (rowlp) rowlp[r] = lp;  // (a row past E: finite-or-NaN numbers nobody reads)
      if (x.log_prob && row0 + r < E) x.log_prob[row0 + r] = lp;
    }
  }
}

}  // namespace
