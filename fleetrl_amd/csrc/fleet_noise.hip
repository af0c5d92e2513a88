// fleet_noise.hip -- temporally correlated action noise on the device (include/fleet_hip.h "correlated action noise on the device"):
// the processes that produce the eps rows fleet_explore_act_dev reads in its GIVEN mode.  The arithmetic is stated in fleet_noise.h.
//
// PINK keeps, per env, a position t, a sequence number q and a cache [n][A] of the env's current sequences.  One launch per call:
//   pink_step   grid E, one workgroup per env.  Thread 0 reads the env's (t, q) and its done / mask byte, decides, writes the new
//               state back and hands the decision to the workgroup through the LDS: nothing else reads or writes that env's state.
//               An env that keeps its sequences copies cache[t][:] to eps_out: adjacent threads, adjacent columns.
//               An env that regenerates stages the twiddle table in the LDS and fills its cache: a wavefront takes a pair of columns
//               (one Philox block per frequency), stages gain x coefficient for up to 256 frequencies in the LDS -- lanes over k --
//               and then owns samples: lane l has t = l, l + 64, ..., up to four of them at a time in registers, and walks k upwards
//               with the staged float4 read by all lanes at one address (a broadcast) and twiddle[(k t) mod n] gathered.  Sample 0
//               goes to eps_out from the registers that hold it.  The work is n^2 / 2 fused multiply-adds x 2 per column; the
//               twiddle gather conflicts in the LDS banks by gcd(k, 32).
// OU is one elementwise kernel: a thread per (env, 4 columns), one Philox block each.
// Launch boundaries are the only visibility mechanism between calls.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fleet_handle.h"
#include "fleet_noise.h"
#include "fleet_philox.h"

namespace {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kChunk = 256;  // frequencies staged at a time, per wavefront
constexpr int kMaxSamples = 4;  // samples a lane carries at a time
enum { kNext = 0, kReset = 1, kRefill = 2 };

struct PinkArgs {
  const float* gain;       // [K]
  const float2* twiddle;   // [n]
  float* cache;            // [E][n][A]
  int32_t* t;              // [E]
  uint32_t* q;             // [E]
  const uint8_t* flag;     // [E] or NULL: done (kNext), mask (kReset)
  float* out;              // [E][A] (kNext)
  uint64_t seed;
  uint32_t env0;
  int A, n, K, mode;
};

// gain x coefficient of frequencies [k0, k0 + count) of pair p -> coef[0 .. count)
__device__ __forceinline__ void stage_pair(const PinkArgs& a, float4* coef, uint32_t env, uint32_t p, uint32_t q, int k0, int count) {
  for (int kk = threadIdx.x & 63; kk < count; kk += 64) {
    const int k = k0 + kk;
    uint32_t w[4];
    float z[4];
    philox4x32_10(env, kNoisePinkTag | p, q, (uint32_t)k, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
    normals4(w, z);
    const float g = a.gain[k];
    const bool real_only = k == 0 || 2 * k == a.n;
    coef[kk] = make_float4(g * z[0], real_only ? 0.0f : g * z[1], g * z[2], real_only ? 0.0f : g * z[3]);
  }
}

// samples t = lane + 64 (g0 + i), i < TT, of the pair this wavefront holds (p < P), every frequency in ascending order
template <int TT>
__device__ __forceinline__ void fill_samples(const PinkArgs& a, const float2* tw, float4* coef, uint32_t env, int e, int p, bool have,
                                             uint32_t q, int g0, bool emit) {
  const int lane = threadIdx.x & 63;
  float acc0[TT], acc1[TT];
  int m[TT], step[TT];
#pragma unroll
  for (int i = 0; i < TT; ++i) {
    acc0[i] = acc1[i] = 0.0f;
    m[i] = 0;
    const int t = lane + 64 * (g0 + i);
    step[i] = t < a.n ? t : 0;  // (a lane past the end walks phase 0 and stores nothing)
  }
  for (int k0 = 0; k0 < a.K; k0 += kChunk) {
    const int count = a.K - k0 < kChunk ? a.K - k0 : kChunk;
    __syncthreads();  // the readers of the chunk before are done (and, the first time, the twiddle table is staged)
    if (have) stage_pair(a, coef, env, (uint32_t)p, q, k0, count);
    __syncthreads();
    if (!have) continue;
    for (int kk = 0; kk < count; ++kk) {
      const float4 c = coef[kk];  // every lane the same address
#pragma unroll
      for (int i = 0; i < TT; ++i) {
        const float2 cs = tw[m[i]];
        acc0[i] = fmaf(-c.y, cs.y, fmaf(c.x, cs.x, acc0[i]));
        acc1[i] = fmaf(-c.w, cs.y, fmaf(c.z, cs.x, acc1[i]));
        m[i] += step[i];
        if (m[i] >= a.n) m[i] -= a.n;
      }
    }
  }
  if (!have) return;
  const int j = 2 * p;
#pragma unroll
  for (int i = 0; i < TT; ++i) {
    const int t = lane + 64 * (g0 + i);
    if (t >= a.n) continue;
    float* row = a.cache + ((size_t)e * a.n + t) * a.A;
    row[j] = acc0[i];
    if (j + 1 < a.A) row[j + 1] = acc1[i];
    if (emit && t == 0) {
      a.out[(size_t)e * a.A + j] = acc0[i];
      if (j + 1 < a.A) a.out[(size_t)e * a.A + j + 1] = acc1[i];
    }
  }
}

__global__ __launch_bounds__(kThreads) void pink_step(PinkArgs a) {
  extern __shared__ float2 tw[];  // [n]
  __shared__ float4 coef[kWaves][kChunk];
  __shared__ int s_regen, s_pos;
  __shared__ uint32_t s_q;
  const int e = blockIdx.x;
  if (threadIdx.x == 0) {
    int t = a.t[e];
    uint32_t q = a.q[e];
    const bool flagged = a.flag && a.flag[e];
    const bool regen = a.mode == kRefill || (a.mode == kNext ? flagged || t >= a.n : !a.flag || flagged);
    if (regen && a.mode != kRefill) {
      q += 1u;
      t = 0;
    }
    s_regen = regen, s_pos = t, s_q = q;
    if (a.mode != kRefill) {
      a.t[e] = a.mode == kNext ? t + 1 : t;
      a.q[e] = q;
    }
  }
  __syncthreads();
  const bool regen = s_regen != 0, emit = a.mode == kNext;
  if (!regen) {
    if (emit) {
      const float* row = a.cache + ((size_t)e * a.n + s_pos) * a.A;
      for (int j = threadIdx.x; j < a.A; j += kThreads) a.out[(size_t)e * a.A + j] = row[j];
    }
    return;
  }
  const uint32_t q = s_q, env = a.env0 + (uint32_t)e;
  for (int i = threadIdx.x; i < a.n; i += kThreads) tw[i] = a.twiddle[i];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int P = (a.A + 1) / 2, G = (a.n + 63) / 64;
  for (int p0 = 0; p0 < P; p0 += kWaves) {  // (every wavefront makes every trip: the barriers inside are the workgroup's)
    const int p = p0 + w;
    const bool have = p < P;
    for (int g0 = 0; g0 < G; g0 += kMaxSamples) {
      switch (G - g0 < kMaxSamples ? G - g0 : kMaxSamples) {
        case 1: fill_samples<1>(a, tw, coef[w], env, e, p, have, q, g0, emit); break;
        case 2: fill_samples<2>(a, tw, coef[w], env, e, p, have, q, g0, emit); break;
        case 3: fill_samples<3>(a, tw, coef[w], env, e, p, have, q, g0, emit); break;
        default: fill_samples<4>(a, tw, coef[w], env, e, p, have, q, g0, emit); break;
      }
    }
  }
}

struct OuArgs {
  float* x;             // [E][A]
  const float *mu, *ss; // [A]
  const uint8_t* done;  // [E] or NULL
  float* out;           // [E][A]
  float th;
  uint64_t seed, count;
  uint32_t env0;
  int E, A;
};

__global__ __launch_bounds__(kThreads) void ou_step(OuArgs a) {
  const int nb = (a.A + 3) / 4;
  const size_t items = (size_t)a.E * nb;
  for (size_t item = (size_t)blockIdx.x * kThreads + threadIdx.x; item < items; item += (size_t)gridDim.x * kThreads) {
    const size_t row = item / nb;
    const int b = (int)(item - row * nb);
    uint32_t w[4];
    float z[4];
    philox4x32_10(a.env0 + (uint32_t)row, kNoiseOuTag | (uint32_t)b, (uint32_t)a.count, (uint32_t)(a.count >> 32), (uint32_t)a.seed,
                  (uint32_t)(a.seed >> 32), w);
    normals4(w, z);
    const bool zero = a.done && a.done[row];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = 4 * b + c;
      if (j >= a.A) break;
      const size_t o = row * a.A + j;
      const float x0 = zero ? 0.0f : a.x[o];
      const float d = a.mu[j] - x0;
      const float x = fmaf(a.ss[j], z[c], fmaf(a.th, d, x0));
      a.x[o] = x;
      a.out[o] = x;
    }
  }
}

__global__ __launch_bounds__(kThreads) void ou_reset(float* x, const uint8_t* mask, int E, int A) {
  const size_t items = (size_t)E * A;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < items; i += (size_t)gridDim.x * kThreads)
    if (!mask || mask[i / A]) x[i] = 0.0f;
}

thread_local std::string g_noise_create_error;

std::string validate(const FleetNoiseParams* p) {
  if (!p) return "null FleetNoiseParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetNoiseParams)) return "FleetNoiseParams.struct_bytes does not match this library";
  if (p->kind != FLEET_NOISE_PINK && p->kind != FLEET_NOISE_OU) return "unknown kind " + std::to_string(p->kind);
  if (p->num_envs < 1) return "num_envs must be >= 1, got " + std::to_string(p->num_envs);
  if (p->act_dim < 1 || p->act_dim > FLEET_NOISE_MAX_ACT_DIM)
    return "act_dim must be in 1.." + std::to_string(FLEET_NOISE_MAX_ACT_DIM) + ", got " + std::to_string(p->act_dim);
  if (p->env_id_offset < 0) return "env_id_offset must be >= 0, got " + std::to_string(p->env_id_offset);
  if (p->kind == FLEET_NOISE_PINK) {
    if (p->seq_len < 2 || p->seq_len > FLEET_NOISE_MAX_SEQ_LEN)
      return "seq_len must be in 2.." + std::to_string(FLEET_NOISE_MAX_SEQ_LEN) + ", got " + std::to_string(p->seq_len);
    if (!(p->beta >= 0.0) || !std::isfinite(p->beta)) return "beta must be finite and >= 0";
    // E <= 2^31, n <= 2^12, A <= 2^9, 4 bytes: the product cannot wrap 64 bits; more than 2^40 bytes is refused here, not by hipMalloc
    const uint64_t bytes = (uint64_t)p->num_envs * (uint64_t)p->seq_len * (uint64_t)p->act_dim * 4u;
    if (bytes > ((uint64_t)1 << 40)) return "the cache of num_envs * seq_len * act_dim floats (" + std::to_string(bytes) + " bytes) is too large";
  } else {
    if (!std::isfinite(p->theta) || !std::isfinite(p->dt) || !(p->dt >= 0.0)) return "theta and dt must be finite, dt >= 0";
    if (!p->mu || !p->sigma) return "null mu or sigma";
    for (int j = 0; j < p->act_dim; ++j)
      if (!std::isfinite(p->mu[j]) || !std::isfinite(p->sigma[j])) return "mu and sigma must be finite (column " + std::to_string(j) + ")";
  }
  return "";
}

uint64_t round256(uint64_t v) { return (v + 255) / 256 * 256; }

}  // namespace

// block: the tables, then the state, then (PINK) the cache; no error word
struct FleetNoise : FleetHandleBase {
  FleetNoiseParams p{};
  int E = 0, A = 0, n = 0, K = 0;
  uint64_t calls = 0;  // OU: the `next` calls so far
  // PINK
  float* gain = nullptr;
  float2* twiddle = nullptr;
  int32_t* t = nullptr;
  uint32_t* q = nullptr;
  float* cache = nullptr;
  // OU
  float *mu = nullptr, *ss = nullptr, *x = nullptr;
  float th = 0.0f;
};

namespace {

hipError_t launch_pink(FleetNoise* h, int mode, const uint8_t* flag, float* out, hipStream_t s) {
  PinkArgs a{};
  a.gain = h->gain, a.twiddle = h->twiddle, a.cache = h->cache, a.t = h->t, a.q = h->q, a.flag = flag, a.out = out;
  a.seed = h->p.seed, a.env0 = (uint32_t)h->p.env_id_offset, a.A = h->A, a.n = h->n, a.K = h->K, a.mode = mode;
  hipLaunchKernelGGL(pink_step, dim3((unsigned)h->E), dim3(kThreads), (size_t)h->n * sizeof(float2), s, a);
  return hipGetLastError();
}

int refuse(FleetNoise* h, const char* entry, const std::string& why) {
  h->error = std::string(entry) + ": " + why;
  return FLEET_ERR_INVALID;
}

}  // namespace

extern "C" {

int fleet_noise_pink_tables(int seq_len, double beta, float* gain, float* twiddle) {
  if (seq_len < 2 || seq_len > FLEET_NOISE_MAX_SEQ_LEN || !(beta >= 0.0) || !std::isfinite(beta) || !gain || !twiddle) {
    g_noise_create_error = "fleet_noise_pink_tables: seq_len must be in 2.." + std::to_string(FLEET_NOISE_MAX_SEQ_LEN) +
                           ", beta finite and >= 0, the outputs not null";
    return FLEET_ERR_INVALID;
  }
  fleet_noise_build_pink_tables(seq_len, beta, gain, twiddle);
  return FLEET_OK;
}

int fleet_noise_create(int device, const FleetNoiseParams* p, fleet_noise_handle* out) {
  if (out) *out = nullptr;
  std::string why = validate(p);  // before the device is touched
  if (why.empty() && !out) why = "null output handle";
  if (!why.empty()) {
    g_noise_create_error = "fleet_noise_create: " + why;
    return FLEET_ERR_INVALID;
  }
  FleetNoise* h = new FleetNoise();
  h->p = *p;
  h->p.mu = h->p.sigma = nullptr;  // (the caller's arrays are read here and not kept)
  h->E = p->num_envs, h->A = p->act_dim;
  const uint64_t E = h->E, A = h->A;
  std::vector<float> tables;
  uint64_t off[5] = {0, 0, 0, 0, 0}, total = 0;
  if (p->kind == FLEET_NOISE_PINK) {
    h->n = p->seq_len, h->K = h->n / 2 + 1;
    const uint64_t n = h->n, K = h->K;
    off[1] = round256(K * 4);               // twiddle
    off[2] = off[1] + round256(n * 8);      // t
    off[3] = off[2] + round256(E * 4);      // q
    off[4] = off[3] + round256(E * 4);      // cache
    total = off[4] + round256(E * n * A * 4);
    tables.assign(off[2] / 4, 0.0f);
    fleet_noise_build_pink_tables(h->n, p->beta, tables.data(), tables.data() + off[1] / 4);
    h->p.cache_bytes = E * n * A * 4;
  } else {
    off[1] = round256(A * 4);               // ss
    off[2] = off[1] + round256(A * 4);      // x
    total = off[2] + round256(E * A * 4);
    tables.assign(off[2] / 4, 0.0f);
    const double root_dt = std::sqrt(p->dt);
    for (uint64_t j = 0; j < A; ++j) {
      tables[j] = (float)p->mu[j];
      tables[off[1] / 4 + j] = (float)(p->sigma[j] * root_dt);
    }
    h->th = (float)(p->theta * p->dt);
    h->p.cache_bytes = 0;
  }
  int rc = handle_open(h, device, total, "noise process", &g_noise_create_error);
  if (rc == FLEET_OK) {
    char* b = h->block;
    if (p->kind == FLEET_NOISE_PINK) {
      h->gain = reinterpret_cast<float*>(b), h->twiddle = reinterpret_cast<float2*>(b + off[1]);
      h->t = reinterpret_cast<int32_t*>(b + off[2]), h->q = reinterpret_cast<uint32_t*>(b + off[3]);
      h->cache = reinterpret_cast<float*>(b + off[4]);
    } else {
      h->mu = reinterpret_cast<float*>(b), h->ss = reinterpret_cast<float*>(b + off[1]), h->x = reinterpret_cast<float*>(b + off[2]);
    }
    // tables, zeroed state (t = 0, q = 0; x = 0), and sequence 0 of every env
    const uint64_t state_bytes = (p->kind == FLEET_NOISE_PINK ? off[4] : total) - off[2];
    if (hipMemcpy(b, tables.data(), off[2], hipMemcpyHostToDevice) != hipSuccess || hipMemset(b + off[2], 0, state_bytes) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess ||
        (p->kind == FLEET_NOISE_PINK && launch_pink(h, kRefill, nullptr, nullptr, h->own_stream) != hipSuccess) ||
        hipStreamSynchronize(h->own_stream) != hipSuccess) {
      (void)hipGetLastError();
      g_noise_create_error = "initialising the noise process failed";
      rc = FLEET_ERR_HIP;
    }
  }
  if (rc != FLEET_OK) {
    if (g_noise_create_error.rfind("fleet_noise_create: ", 0) != 0) g_noise_create_error = "fleet_noise_create: " + g_noise_create_error;
    fleet_noise_destroy(h);
    return rc;
  }
  *out = h;
  return FLEET_OK;
}

int fleet_noise_destroy(fleet_noise_handle h) {
  if (!h) return FLEET_OK;
  handle_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_noise_last_error(fleet_noise_handle h) { return h ? h->error.c_str() : g_noise_create_error.c_str(); }

int fleet_noise_set_stream(fleet_noise_handle h, void* hip_stream) { return h ? handle_set_stream(h, hip_stream) : FLEET_ERR_INVALID; }

int fleet_noise_next_dev(fleet_noise_handle h, const uint8_t* done, float* eps_out) {
  if (!h) return FLEET_ERR_INVALID;
  if (!eps_out) return refuse(h, "fleet_noise_next_dev", "null eps_out");
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  if (h->p.kind == FLEET_NOISE_PINK) {
    FLEET_HANDLE_TRY(h, launch_pink(h, kNext, done, eps_out, h->stream));
    return FLEET_OK;
  }
  OuArgs a{};
  a.x = h->x, a.mu = h->mu, a.ss = h->ss, a.done = done, a.out = eps_out, a.th = h->th, a.seed = h->p.seed, a.count = h->calls;
  a.env0 = (uint32_t)h->p.env_id_offset, a.E = h->E, a.A = h->A;
  hipLaunchKernelGGL(ou_step, dim3(grid_for((size_t)h->E * ((h->A + 3) / 4), kThreads, 4096)), dim3(kThreads), 0, h->stream, a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  h->calls += 1;
  return FLEET_OK;
}

int fleet_noise_reset_dev(fleet_noise_handle h, const uint8_t* mask) {
  if (!h) return FLEET_ERR_INVALID;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  if (h->p.kind == FLEET_NOISE_PINK) {
    FLEET_HANDLE_TRY(h, launch_pink(h, kReset, mask, nullptr, h->stream));
    return FLEET_OK;
  }
  hipLaunchKernelGGL(ou_reset, dim3(grid_for((size_t)h->E * h->A, kThreads, 4096)), dim3(kThreads), 0, h->stream, h->x, mask, h->E, h->A);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

int fleet_noise_get_state_dev(fleet_noise_handle h, int32_t* t, uint32_t* q, float* x, uint64_t* calls) {
  if (!h) return FLEET_ERR_INVALID;
  const bool pink = h->p.kind == FLEET_NOISE_PINK;
  if (pink ? !t || !q : !x) return refuse(h, "fleet_noise_get_state_dev", pink ? "PINK needs t and q" : "OU needs x");
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  if (pink) {
    FLEET_HANDLE_TRY(h, hipMemcpyAsync(t, h->t, (size_t)h->E * 4, hipMemcpyDeviceToDevice, h->stream));
    FLEET_HANDLE_TRY(h, hipMemcpyAsync(q, h->q, (size_t)h->E * 4, hipMemcpyDeviceToDevice, h->stream));
  } else {
    FLEET_HANDLE_TRY(h, hipMemcpyAsync(x, h->x, (size_t)h->E * h->A * 4, hipMemcpyDeviceToDevice, h->stream));
  }
  if (calls) *calls = h->calls;
  return FLEET_OK;
}

int fleet_noise_set_state_dev(fleet_noise_handle h, const int32_t* t, const uint32_t* q, const float* x, uint64_t calls) {
  if (!h) return FLEET_ERR_INVALID;
  const bool pink = h->p.kind == FLEET_NOISE_PINK;
  if (pink ? !t || !q : !x) return refuse(h, "fleet_noise_set_state_dev", pink ? "PINK needs t and q" : "OU needs x");
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  if (!pink) {
    FLEET_HANDLE_TRY(h, hipMemcpyAsync(h->x, x, (size_t)h->E * h->A * 4, hipMemcpyDeviceToDevice, h->stream));
    h->calls = calls;
    return FLEET_OK;
  }
  // the positions are looked at on the host before anything changes: the one entry that waits for the stream
  std::vector<int32_t> host((size_t)h->E);
  FLEET_HANDLE_TRY(h, hipMemcpyAsync(host.data(), t, host.size() * 4, hipMemcpyDeviceToHost, h->stream));
  FLEET_HANDLE_TRY(h, hipStreamSynchronize(h->stream));
  for (int e = 0; e < h->E; ++e)
    if (host[e] < 0 || host[e] > h->n)
      return refuse(h, "fleet_noise_set_state_dev", "t of env " + std::to_string(e) + " must be in 0.." + std::to_string(h->n) + ", got " +
                                                        std::to_string(host[e]));
  FLEET_HANDLE_TRY(h, hipMemcpyAsync(h->t, t, (size_t)h->E * 4, hipMemcpyDeviceToDevice, h->stream));
  FLEET_HANDLE_TRY(h, hipMemcpyAsync(h->q, q, (size_t)h->E * 4, hipMemcpyDeviceToDevice, h->stream));
  FLEET_HANDLE_TRY(h, launch_pink(h, kRefill, nullptr, nullptr, h->stream));  // the cache is a function of q
  h->calls = calls;
  return FLEET_OK;
}

int fleet_noise_describe(fleet_noise_handle h, FleetNoiseParams* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  *out = h->p;
  return FLEET_OK;
}

}  // extern "C"
