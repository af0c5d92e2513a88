// fleet_philox.h -- Philox4x32-10, the counter-based generator the replay buffer's index draw (fleet_replay.hip), the exploration
// noise (fleet_policy.hip), the targets' smoothing noise (fleet_qtarget.hip) and the correlated noise processes (fleet_noise.hip)
// share, the Box-Muller step of all but the first, and the per-row draw of the second and third.
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

// the Philox block of (global row id, block b of the row) at (step, seed): the counter scheme of the exploration and target noise
__device__ __forceinline__ void philox_row_block(uint32_t id, int b, uint64_t step, uint64_t seed, uint32_t* w) {
  philox4x32_10(id, (uint32_t)b, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
}

// the four normals of columns 4b .. 4b + 3 of a row of A columns: drawn (philox_row_block of the row's global id), or, `given`, read
// from noise[o + column], o the row's offset, zeros past A
__device__ __forceinline__ void row_normals4(int given, const float* noise, size_t o, int b, int A, uint32_t id, uint64_t step,
                                             uint64_t seed, float* z) {
  if (given) {
#pragma unroll
    for (int c = 0; c < 4; ++c) z[c] = 4 * b + c < A ? noise[o + 4 * b + c] : 0.0f;
  } else {
    uint32_t w[4];
    philox_row_block(id, b, step, seed, w);
    normals4(w, z);
  }
}
