// fleet_philox.h -- Philox4x32-10, the counter-based generator the replay buffer's index draw (fleet_replay.hip), the exploration
// noise (fleet_policy.hip) and the correlated noise processes (fleet_noise.hip) share, and the Box-Muller step of the latter two.
// (The env's start-row sampler keeps its own restatement: fleet_wave.h philox_start.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Philox4x32-10 (Salmon et al., SC'11): the block of counter (c0, c1, c2, c3) under key (k0, k1)
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* x) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// the four standard normals of one Philox block: Box-Muller on (x0, x1) and (x2, x3)
__device__ __forceinline__ void normals4(const uint32_t* x, float* z) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = (float)((x[2 * p] >> 8) + 1u) * 0x1p-24f;  // (0, 1], exact
    const float u2 = (float)(x[2 * p + 1] >> 8) * 0x1p-24f;     // [0, 1), exact
    const float r = sqrtf(-2.0f * logf(u1));
    const float t = 6.283185307179586f * u2;
    z[2 * p] = r * cosf(t);
    z[2 * p + 1] = r * sinf(t);
  }
}
