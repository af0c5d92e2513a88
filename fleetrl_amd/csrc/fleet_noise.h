// fleet_noise.h -- the arithmetic of the correlated noise processes (fleet_noise.hip; include/fleet_hip.h "correlated action noise on
// the device"), stated once: the host's tables, the device's float32 chains, the Philox counters.  tests/noise_model.py restates it.
//
// PINK, one sequence of n samples for (seed, global env id g, column j, sequence number q); K = n / 2 + 1 frequencies.
//   tables (host, float64, rounded to float32 once): gain[k], k < K, and twiddle[m] = (cos, sin)(2 pi m / n), m < n
//   (fleet_noise_build_pink_tables below).
//   draws: block k of the pair p = j / 2 is philox4x32_10 of counter (g, 0x80000000 | p, q, k) under key (seed lo, seed hi); normals4
//   (fleet_philox.h) of its words gives z0..z3: column 2p has (a_k, b_k) = (z0, z1), column 2p + 1 has (z2, z3).
//   staged per k:  ga = gain[k] * a_k;  gb = gain[k] * b_k, but gb = +0 for k = 0 and for 2k = n     (float32 products)
//   sample t:      acc = 0;  for k = 0 .. K-1 ascending:  m = (k * t) mod n  (integers: m starts at 0 and grows by t, minus n when >= n)
//                    acc = fmaf(ga, twiddle[m].cos, acc);  acc = fmaf(-gb, twiddle[m].sin, acc)
//                  y[t] = acc.  No sinf / cosf, no FFT: a sample is that chain of 2K fused multiply-adds bit for bit.
// OU, per (env row e, column j) and call number c (the calls before this one):
//   tables (host, float64 -> float32): th = theta * dt, ss[j] = sigma[j] * sqrt(dt), mu[j]
//   eps: block j / 4 is philox4x32_10 of counter (g, 0x40000000 | (j / 4), c lo, c hi); normals4 gives columns 4(j/4) .. 4(j/4)+3
//   x0 = done[e] ? 0 : x;  d = mu[j] - x0;  u = fmaf(th, d, x0);  x = fmaf(ss[j], eps, u);  the output is x.
// The tags 0x80000000 / 0x40000000 in counter word 1 keep these draws apart from the exploration epilogue's white noise under the
// same seed: its word 1 is the column block j / 4 <= 127.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

constexpr uint32_t kNoisePinkTag = 0x80000000u;
constexpr uint32_t kNoiseOuTag = 0x40000000u;

// colorednoise.powerlaw_psd_gaussian(beta, n) folded into one gain per frequency: s_k = f_k^(-beta/2) with f_k = k / n and f_0 := f_1,
// sigma = 2 sqrt(sum w^2) / n over w = s[1:] with its last element times (1 + n mod 2) / 2, and
//   gain[0] = sqrt(2) s_0 / (n sigma);  gain[k] = 2 s_k / (n sigma) for 0 < 2k < n;  gain[n/2] = sqrt(2) s_{n/2} / (n sigma) for even n
// (the sqrt(2) of the two real coefficients, irfft's 1/n and 2/n weights, and 1/sigma).  gain: K = n/2 + 1 floats; twiddle: 2n floats.
inline void fleet_noise_build_pink_tables(int n, double beta, float* gain, float* twiddle) {
  const int K = n / 2 + 1;
  std::vector<double> s(K);
  for (int k = 0; k < K; ++k) s[k] = std::pow((double)(k ? k : 1) / (double)n, -beta / 2.0);
  double sum = 0.0;
  for (int k = 1; k < K; ++k) {
    const double w = k == K - 1 ? s[k] * (double)(1 + n % 2) / 2.0 : s[k];
    sum += w * w;
  }
  const double sigma = 2.0 * std::sqrt(sum) / (double)n;
  const double root2 = std::sqrt(2.0);
  for (int k = 0; k < K; ++k) {
    const bool real_only = k == 0 || 2 * k == n;
    gain[k] = (float)((real_only ? root2 : 2.0) * s[k] / ((double)n * sigma));
  }
  const double two_pi = 6.283185307179586476925286766559;
  for (int m = 0; m < n; ++m) {
    twiddle[2 * m] = (float)std::cos(two_pi * (double)m / (double)n);
    twiddle[2 * m + 1] = (float)std::sin(two_pi * (double)m / (double)n);
  }
}
