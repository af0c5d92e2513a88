// fleet_norm.hip -- stable-baselines3 `VecNormalize` on the device: running mean / variance of the observations and of the
// discounted returns, and the normalise-and-clip pass (include/fleet_hip.h "running observation / reward normaliser").
//
// One training step is three launches on one stream; the launch boundaries make each one's results visible to the next:
//   norm_moments   grid (column tiles [+ 1 returns block], row slabs): per slab and column the sums S1 = sum(x - K),
//                  S2 = sum((x - K)^2) in float64, K = the column's value in row 0 of the batch (a shift by a sample of the
//                  batch keeps S2 - S1^2 / n free of cancellation for columns far from zero); adjacent lanes take adjacent
//                  columns (coalesced rows), the 4 waves of a workgroup take every 4th row and are summed in a fixed order.
//                  The returns block forms returns * gamma + r (without storing it) and its sums the same way.
//   norm_finalize  one workgroup per column tile [+ 1 for the returns]: the slab sums in a fixed order, the batch mean / variance,
//                  the running update (SB3's formula, its operation order), sd = sqrt(var + epsilon) for apply.
//   norm_apply     elementwise: obs' = clip((obs - mean) / sd) -- 16-byte loads and stores when D % 4 == 0 and the buffers
//                  allow it --, the terminal rows of done envs, the reward, the returns (update, then zero where done).
// The counts are exact functions of the number of updates (count + E each time): the host keeps them and passes them by value.
// No atomics of any kind: every sum is taken in an order fixed by the shapes, so results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fleet_handle.h"
#include "fleet_norm.h"

namespace {

constexpr int kRows = 64;    // rows per slab of norm_moments
constexpr int kWaves = 4;    // waves per workgroup (256 threads)
constexpr int kThreads = 64 * kWaves;
constexpr int kApplyMaxBlocks = 2048;

__global__ __launch_bounds__(kThreads) void norm_moments(const float* __restrict__ obs, int E, int D, int tiles,
                                                         const double* __restrict__ raw_reward, const double* __restrict__ returns,
                                                         double gamma, double* __restrict__ part_obs, double* __restrict__ part_ret) {
  const int slab = blockIdx.y;
  const int r0 = slab * kRows;
  const int r1 = min(E, r0 + kRows);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if ((int)blockIdx.x < tiles) {
    __shared__ double sh[2][kWaves][64];
    const int c = blockIdx.x * 64 + lane;
    double s1 = 0.0, s2 = 0.0;
    if (c < D) {
      const double K = (double)obs[c];
#pragma unroll 16  // (the loads of a thread's rows issue together; the adds keep their order)
      for (int r = r0 + w; r < r1; r += kWaves) {
        const double v = (double)obs[(size_t)r * D + c] - K;
        s1 += v;
        s2 += v * v;
      }
    }
    sh[0][w][lane] = s1;
    sh[1][w][lane] = s2;
    __syncthreads();
    if (w == 0 && c < D) {
      double a = sh[0][0][lane], b = sh[1][0][lane];
      for (int k = 1; k < kWaves; ++k) {
        a += sh[0][k][lane];
        b += sh[1][k][lane];
      }
      part_obs[((size_t)slab * 2 + 0) * D + c] = a;
      part_obs[((size_t)slab * 2 + 1) * D + c] = b;
    }
  } else if (w == 0) {  // the returns block: one row per lane (kRows == 64)
    const double K = returns[0] * gamma + (double)(float)raw_reward[0];
    const int r = r0 + lane;
    double v = 0.0;
    if (r < r1) {
      const double nr = returns[r] * gamma + (double)(float)raw_reward[r];
      v = nr - K;
    }
    double s1 = v, s2 = v * v;
    for (int off = 32; off > 0; off >>= 1) {  // a fixed tree: the same order every launch
      s1 += __shfl_down(s1, off, 64);
      s2 += __shfl_down(s2, off, 64);
    }
    if (lane == 0) {
      part_ret[(size_t)slab * 2 + 0] = s1;
      part_ret[(size_t)slab * 2 + 1] = s2;
    }
  }
}

// SB3 RunningMeanStd.update_from_moments, operation for operation; writes mean, var and sqrt(var + eps)
__device__ inline void running_update(double bm, double bv, double n, double count, double eps, double* mean, double* var,
                                      double* sd) {
  const double m = *mean, v = *var;
  const double d = bm - m;
  const double tot = count + n;
  const double new_mean = m + d * n / tot;
  const double m2 = v * count + bv * n + d * d * count * n / tot;
  const double new_var = m2 / tot;
  *mean = new_mean;
  *var = new_var;
  *sd = sqrt(new_var + eps);
}

// batch mean / population variance from sums shifted by K
__device__ inline void batch_moments(double S1, double S2, double K, double n, double* bm, double* bv) {
  *bm = K + S1 / n;
  const double m2 = S2 - S1 * S1 / n;
  *bv = m2 > 0.0 ? m2 / n : 0.0;
}

__global__ __launch_bounds__(kThreads) void norm_finalize(const float* __restrict__ obs, int E, int D, int tiles, int slabs,
                                                          const double* __restrict__ part_obs, const double* __restrict__ part_ret,
                                                          const double* __restrict__ raw_reward, const double* __restrict__ returns,
                                                          double gamma, double obs_count, double ret_count, double eps,
                                                          double* __restrict__ obs_mean, double* __restrict__ obs_var,
                                                          double* __restrict__ obs_sd, double* __restrict__ ret_stat) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double n = (double)E;
  if ((int)blockIdx.x < tiles) {
    __shared__ double sh[2][kWaves][64];
    const int c = blockIdx.x * 64 + lane;
    double a = 0.0, b = 0.0;
    if (c < D)
#pragma unroll 16
      for (int s = w; s < slabs; s += kWaves) {
        a += part_obs[((size_t)s * 2 + 0) * D + c];
        b += part_obs[((size_t)s * 2 + 1) * D + c];
      }
    sh[0][w][lane] = a;
    sh[1][w][lane] = b;
    __syncthreads();
    if (w == 0 && c < D) {
      double S1 = sh[0][0][lane], S2 = sh[1][0][lane];
      for (int k = 1; k < kWaves; ++k) {
        S1 += sh[0][k][lane];
        S2 += sh[1][k][lane];
      }
      double bm, bv;
      batch_moments(S1, S2, (double)obs[c], n, &bm, &bv);
      running_update(bm, bv, n, obs_count, eps, &obs_mean[c], &obs_var[c], &obs_sd[c]);
    }
  } else if (w == 0) {  // the returns block
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int s = lane; s < slabs; s += 64) {
      a += part_ret[(size_t)s * 2 + 0];
      b += part_ret[(size_t)s * 2 + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
      a += __shfl_down(a, off, 64);
      b += __shfl_down(b, off, 64);
    }
    if (lane == 0) {
      double bm, bv;
      batch_moments(a, b, returns[0] * gamma + (double)(float)raw_reward[0], n, &bm, &bv);
      running_update(bm, bv, n, ret_count, eps, &ret_stat[0], &ret_stat[1], &ret_stat[2]);
    }
  }
}

// sd = sqrt(var + eps) after fleet_norm_set_state / fleet_norm_configure (the same device arithmetic as norm_finalize)
__global__ __launch_bounds__(kThreads) void norm_derive(int D, double eps, const double* __restrict__ obs_var,
                                                        double* __restrict__ obs_sd, double* __restrict__ ret_stat) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < D) obs_sd[i] = sqrt(obs_var[i] + eps);
  if (i == 0) ret_stat[2] = sqrt(ret_stat[1] + eps);
}

// another normaliser's running statistics into this one (fleet_eval_sync_norm_dev), and sd from them as norm_derive forms it
__global__ __launch_bounds__(kThreads) void norm_sync(int D, double eps, const double* src_mean, const double* src_var,
                                                      const double* src_ret, double* obs_mean, double* obs_var, double* obs_sd,
                                                      double* ret_stat) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < D) {
    const double m = src_mean[i], v = src_var[i];
    obs_mean[i] = m;
    obs_var[i] = v;
    obs_sd[i] = sqrt(v + eps);
  }
  if (i == 0) {
    const double m = src_ret[0], v = src_ret[1];
    ret_stat[0] = m;
    ret_stat[1] = v;
    ret_stat[2] = sqrt(v + eps);
  }
}

struct ApplyArgs {
  const float* raw;
  float* out;
  const uint8_t* done;       // NULL on reset
  const float* raw_term;     // NULL: no terminal rows
  float* term;
  const double* mean;
  const double* sd;
  const double* raw_reward;  // NULL on reset
  double* reward;
  double* returns;
  double* raw_copy;          // keeps the raw rewards for fleet_norm_original_host
  const double* ret_stat;
  double clip_obs, clip_reward, gamma;
  int E, D;
  int norm_obs, norm_reward, update_returns, reset;
};

template <bool kVec>
__global__ __launch_bounds__(kThreads) void norm_apply(ApplyArgs a) {
  const size_t gid = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * kThreads;
  for (size_t e = gid; e < (size_t)a.E; e += stride) {
    if (a.reset) {
      a.returns[e] = 0.0;
      continue;
    }
    const double raw = a.raw_reward[e];
    const double r = (double)(float)raw;
    const bool d = a.done[e] != 0;
    const double nr = a.update_returns ? a.returns[e] * a.gamma + r : a.returns[e];
    a.returns[e] = d ? 0.0 : nr;
    a.raw_copy[e] = raw;
    a.reward[e] = a.norm_reward ? fleet_norm_reward1(r, a.ret_stat[2], a.clip_reward) : r;
  }
  const bool write_obs = a.norm_obs || a.out != a.raw;
  const bool write_term = a.raw_term && (a.norm_obs || a.term != a.raw_term);
  if (!write_obs && !write_term) return;
  const double c = a.clip_obs;
  if (kVec) {  // D % 4 == 0, every buffer 16-byte aligned: four columns of one row per item
    const size_t items = (size_t)a.E * a.D / 4;
    for (size_t i = gid; i < items; i += stride) {
      const size_t flat = i * 4;
      const int col = (int)(flat % (size_t)a.D);
      const size_t row = flat / (size_t)a.D;
      double m[4], s[4];
      for (int k = 0; k < 4; ++k) {
        m[k] = a.mean[col + k];
        s[k] = a.sd[col + k];
      }
      if (write_obs) {
        float4 x = *reinterpret_cast<const float4*>(a.raw + flat);
        if (a.norm_obs) x = make_float4(fleet_norm_obs1(x.x, m[0], s[0], c), fleet_norm_obs1(x.y, m[1], s[1], c), fleet_norm_obs1(x.z, m[2], s[2], c),
                                        fleet_norm_obs1(x.w, m[3], s[3], c));
        *reinterpret_cast<float4*>(a.out + flat) = x;
      }
      if (write_term && a.done[row]) {
        float4 x = *reinterpret_cast<const float4*>(a.raw_term + flat);
        if (a.norm_obs) x = make_float4(fleet_norm_obs1(x.x, m[0], s[0], c), fleet_norm_obs1(x.y, m[1], s[1], c), fleet_norm_obs1(x.z, m[2], s[2], c),
                                        fleet_norm_obs1(x.w, m[3], s[3], c));
        *reinterpret_cast<float4*>(a.term + flat) = x;
      }
    }
  } else {
    const size_t items = (size_t)a.E * a.D;
    for (size_t i = gid; i < items; i += stride) {
      const int col = (int)(i % (size_t)a.D);
      const size_t row = i / (size_t)a.D;
      const double m = a.mean[col], s = a.sd[col];
      if (write_obs) {
        const float x = a.raw[i];
        a.out[i] = a.norm_obs ? fleet_norm_obs1(x, m, s, c) : x;
      }
      if (write_term && a.done[row]) {
        const float x = a.raw_term[i];
        a.term[i] = a.norm_obs ? fleet_norm_obs1(x, m, s, c) : x;
      }
    }
  }
}

thread_local std::string g_norm_create_error;

const char* validate(const FleetNormParams* p) {
  if (!p) return "null FleetNormParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetNormParams)) return "FleetNormParams.struct_bytes does not match this library";
  if (p->num_envs < 1 || p->obs_dim < 1) return "num_envs and obs_dim must be >= 1";
  if (p->num_envs > 65535 * kRows) return "num_envs too large (the moments grid has one row of workgroups per 64 envs)";
  if ((size_t)p->num_envs * (size_t)p->obs_dim > ((size_t)1 << 40)) return "num_envs * obs_dim too large";
  if (!(p->clip_obs > 0) || !(p->clip_reward > 0)) return "clip_obs and clip_reward must be > 0";
  if (!(p->gamma >= 0 && p->gamma <= 1)) return "gamma must be in [0, 1]";
  if (!(p->epsilon > 0)) return "epsilon must be > 0";
  return nullptr;
}

}  // namespace

// block: everything the pointers below name (no error word)
struct FleetNorm : FleetHandleBase {
  FleetNormParams p{};
  int E = 0, D = 0, tiles = 0, slabs = 0;
  hipStream_t last_stream = nullptr;  // where the last enqueue went (state access waits for it)
  double obs_count = 1e-4, ret_count = 1e-4;
  double *obs_mean = nullptr, *obs_var = nullptr, *obs_sd = nullptr, *ret_stat = nullptr, *returns = nullptr, *raw_reward = nullptr;
  double *part_obs = nullptr, *part_ret = nullptr;
  float* out_obs = nullptr;
  const float* last_raw_obs = nullptr;  // nullptr: none (no call yet, or the last one was in place)
  bool have_reward = false;
  // readers of the statistics on other streams (fleet_norm_begin_read / _end_read), created on first use
  hipEvent_t writer_event = nullptr, reader_event = nullptr;
  bool reader_pending = false;
};

namespace {

hipError_t launch_apply(FleetNorm* n, const ApplyArgs& a, hipStream_t s) {
  const bool vec = a.D % 4 == 0 && aligned16(a.raw) && aligned16(a.out) && (!a.raw_term || (aligned16(a.raw_term) && aligned16(a.term)));
  const size_t items = (size_t)a.E * a.D / (vec ? 4 : 1);
  const unsigned blocks = grid_for(items > (size_t)a.E ? items : (size_t)a.E, kThreads, kApplyMaxBlocks);
  if (vec) hipLaunchKernelGGL(norm_apply<true>, dim3(blocks), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(norm_apply<false>, dim3(blocks), dim3(kThreads), 0, s, a);
  (void)n;
  return hipGetLastError();
}

// moments + finalize for the observations (obs_tiles > 0) and / or the returns (with_ret)
hipError_t launch_update(FleetNorm* n, const float* raw_obs, bool with_obs, const double* raw_reward, bool with_ret, hipStream_t s) {
  const int tiles = with_obs ? n->tiles : 0;
  const int gx = tiles + (with_ret ? 1 : 0);
  if (gx == 0) return hipSuccess;
  hipLaunchKernelGGL(norm_moments, dim3(gx, n->slabs), dim3(kThreads), 0, s, raw_obs, n->E, n->D, tiles, raw_reward, n->returns,
                     n->p.gamma, n->part_obs, n->part_ret);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(norm_finalize, dim3(gx), dim3(kThreads), 0, s, raw_obs, n->E, n->D, tiles, n->slabs, n->part_obs, n->part_ret,
                     raw_reward, n->returns, n->p.gamma, n->obs_count, n->ret_count, n->p.epsilon, n->obs_mean, n->obs_var, n->obs_sd,
                     n->ret_stat);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (with_obs) n->obs_count = n->obs_count + (double)n->E;
  if (with_ret) n->ret_count = n->ret_count + (double)n->E;
  return hipSuccess;
}

ApplyArgs base_args(FleetNorm* n) {
  ApplyArgs a{};
  a.mean = n->obs_mean;
  a.sd = n->obs_sd;
  a.returns = n->returns;
  a.raw_copy = n->raw_reward;
  a.ret_stat = n->ret_stat;
  a.clip_obs = n->p.clip_obs;
  a.clip_reward = n->p.clip_reward;
  a.gamma = n->p.gamma;
  a.E = n->E;
  a.D = n->D;
  a.norm_obs = n->p.norm_obs != 0;
  a.norm_reward = n->p.norm_reward != 0;
  return a;
}

// a kernel on another stream still reads the statistics: stream `s` (or the host) waits for it
hipError_t wait_reader(FleetNorm* n, hipStream_t s, bool host = false) {
  n->reader_pending = false;
  return host ? hipEventSynchronize(n->reader_event) : hipStreamWaitEvent(s, n->reader_event, 0);
}

hipError_t derive(FleetNorm* n, hipStream_t s) {
  hipLaunchKernelGGL(norm_derive, dim3((n->D + kThreads - 1) / kThreads), dim3(kThreads), 0, s, n->D, n->p.epsilon, n->obs_var,
                     n->obs_sd, n->ret_stat);
  return hipGetLastError();
}

}  // namespace

int fleet_norm_check_fit(fleet_norm_handle n, int E, int D, int device, std::string* why) {
  if (!n) {
    *why = "null normaliser";
    return FLEET_ERR_INVALID;
  }
  if (n->E != E || n->D != D || n->device != device) {
    *why = "the normaliser was made for " + std::to_string(n->E) + " envs x " + std::to_string(n->D) + " on device " +
           std::to_string(n->device) + ", the env has " + std::to_string(E) + " x " + std::to_string(D) + " on device " +
           std::to_string(device);
    return FLEET_ERR_INVALID;
  }
  return FLEET_OK;
}

float* fleet_norm_out_buffer(fleet_norm_handle n) { return n->out_obs; }

hipError_t fleet_norm_begin_read(fleet_norm_handle n, hipStream_t s, FleetNormView* out) {
  if (n->last_stream != s) {
    hipError_t e = n->writer_event ? hipSuccess : hipEventCreateWithFlags(&n->writer_event, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(n->writer_event, n->last_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, n->writer_event, 0);
    if (e != hipSuccess) return e;
  }
  out->obs_mean = n->obs_mean;
  out->obs_sd = n->obs_sd;
  out->ret_stat = n->ret_stat;
  out->clip_obs = n->p.clip_obs;
  out->clip_reward = n->p.clip_reward;
  out->norm_obs = n->p.norm_obs != 0;
  out->norm_reward = n->p.norm_reward != 0;
  out->E = n->E;
  out->D = n->D;
  out->device = n->device;
  return hipSuccess;
}

hipError_t fleet_norm_end_read(fleet_norm_handle n, hipStream_t s) {
  if (n->last_stream == s) return hipSuccess;  // (stream order already puts the next update behind the reader)
  hipError_t e = n->reader_event ? hipSuccess : hipEventCreateWithFlags(&n->reader_event, hipEventDisableTiming);
  if (e == hipSuccess && n->reader_pending) e = hipStreamWaitEvent(s, n->reader_event, 0);  // an earlier reader elsewhere: chain
  if (e == hipSuccess) e = hipEventRecord(n->reader_event, s);
  if (e == hipSuccess) n->reader_pending = true;
  return e;
}

hipError_t fleet_norm_enqueue_reset(fleet_norm_handle n, const float* raw_obs, float* obs, hipStream_t s) {
  if (n->last_stream != s) {  // work of the last call on another stream (the env's, the normaliser's own) uses the same state
    const hipError_t e = hipStreamSynchronize(n->last_stream);
    if (e != hipSuccess) return e;
  }
  n->last_stream = s;
  if (n->reader_pending) {
    const hipError_t e = wait_reader(n, s);
    if (e != hipSuccess) return e;
  }
  const bool upd = n->p.training && n->p.norm_obs;
  if (upd) {
    const hipError_t e = launch_update(n, raw_obs, true, nullptr, false, s);
    if (e != hipSuccess) return e;
  }
  ApplyArgs a = base_args(n);
  a.raw = raw_obs;
  a.out = obs;
  a.reset = 1;
  n->last_raw_obs = obs == raw_obs ? nullptr : raw_obs;
  return launch_apply(n, a, s);
}

hipError_t fleet_norm_enqueue_step(fleet_norm_handle n, const float* raw_obs, const double* raw_reward, const uint8_t* done,
                                   const float* raw_terminal, float* obs, double* reward, float* terminal, hipStream_t s) {
  if (n->last_stream != s) {  // work of the last call on another stream (the env's, the normaliser's own) uses the same state
    const hipError_t e = hipStreamSynchronize(n->last_stream);
    if (e != hipSuccess) return e;
  }
  n->last_stream = s;
  if (n->reader_pending) {
    const hipError_t e = wait_reader(n, s);
    if (e != hipSuccess) return e;
  }
  if (n->p.training) {
    const hipError_t e = launch_update(n, raw_obs, n->p.norm_obs != 0, raw_reward, true, s);
    if (e != hipSuccess) return e;
  }
  ApplyArgs a = base_args(n);
  a.raw = raw_obs;
  a.out = obs;
  a.done = done;
  a.raw_term = (raw_terminal && terminal) ? raw_terminal : nullptr;
  a.term = a.raw_term ? terminal : nullptr;
  a.raw_reward = raw_reward;
  a.reward = reward;
  a.update_returns = n->p.training != 0;
  n->last_raw_obs = obs == raw_obs ? nullptr : raw_obs;
  n->have_reward = true;
  return launch_apply(n, a, s);
}

int fleet_norm_check_sync(fleet_norm_handle dst, fleet_norm_handle src, std::string* why) {
  if (!dst || !src) *why = dst ? "null source normaliser" : "null destination normaliser";
  else if (dst->D != src->D || dst->device != src->device)
    *why = "the source normaliser has obs_dim " + std::to_string(src->D) + " on device " + std::to_string(src->device) + ", the destination " +
           std::to_string(dst->D) + " on device " + std::to_string(dst->device);
  else return FLEET_OK;
  return FLEET_ERR_INVALID;
}

hipError_t fleet_norm_enqueue_sync(fleet_norm_handle dst, fleet_norm_handle src) {
  const hipStream_t s = dst->stream;
  if (dst->last_stream != s) {  // (as the step: dst's last call on another stream uses the same state)
    const hipError_t e = hipStreamSynchronize(dst->last_stream);
    if (e != hipSuccess) return e;
  }
  dst->last_stream = s;
  if (dst->reader_pending) {
    const hipError_t e = wait_reader(dst, s);
    if (e != hipSuccess) return e;
  }
  FleetNormView v{};
  hipError_t e = dst == src ? hipSuccess : fleet_norm_begin_read(src, s, &v);  // (s waits for src's last launch elsewhere)
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(norm_sync, dim3((dst->D + kThreads - 1) / kThreads), dim3(kThreads), 0, s, dst->D, dst->p.epsilon, src->obs_mean,
                     src->obs_var, src->ret_stat, dst->obs_mean, dst->obs_var, dst->obs_sd, dst->ret_stat);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  dst->obs_count = src->obs_count;
  dst->ret_count = src->ret_count;
  return dst == src ? hipSuccess : fleet_norm_end_read(src, s);
}

extern "C" {

int fleet_norm_create(int device, const FleetNormParams* p, fleet_norm_handle* out) {
  if (out) *out = nullptr;
  const char* why = validate(p);  // before the device is touched
  if (!why && !out) why = "null output handle";
  if (why) {
    g_norm_create_error = why;
    return FLEET_ERR_INVALID;
  }
  FleetNorm* n = new FleetNorm();
  n->p = *p;
  n->E = p->num_envs;
  n->D = p->obs_dim;
  n->tiles = (n->D + 63) / 64;
  n->slabs = (n->E + kRows - 1) / kRows;
  const size_t E = n->E, D = n->D, S = n->slabs;
  // doubles: obs mean / var / sd [D], ret_stat [4], returns [E], raw rewards [E], partials [S,2,D] + [S,2]; then the floats
  const size_t nd = 3 * D + 4 + 2 * E + 2 * S * D + 2 * S;
  const int rc = handle_open(n, device, nd * 8 + E * D * 4, "normaliser", &g_norm_create_error);
  if (rc != FLEET_OK) {
    fleet_norm_destroy(n);
    return rc;
  }
  n->last_stream = n->own_stream;
  double* q = reinterpret_cast<double*>(n->block);
  n->obs_mean = q, q += D;
  n->obs_var = q, q += D;
  n->obs_sd = q, q += D;
  n->ret_stat = q, q += 4;
  n->returns = q, q += E;
  n->raw_reward = q, q += E;
  n->part_obs = q, q += 2 * S * D;
  n->part_ret = q, q += 2 * S;
  n->out_obs = reinterpret_cast<float*>(q);
  std::vector<double> init(3 * D + 4 + 2 * E, 0.0);
  for (size_t c = 0; c < D; ++c) init[D + c] = 1.0;  // var = 1
  init[3 * D + 1] = 1.0;                             // ret var = 1
  if (hipMemcpy(n->block, init.data(), init.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      derive(n, n->own_stream) != hipSuccess || hipStreamSynchronize(n->own_stream) != hipSuccess) {
    g_norm_create_error = "initialising the normaliser's state failed";
    fleet_norm_destroy(n);
    return FLEET_ERR_HIP;
  }
  *out = n;
  return FLEET_OK;
}

int fleet_norm_destroy(fleet_norm_handle n) {
  if (!n) return FLEET_OK;
  (void)hipSetDevice(n->device);
  if (n->last_stream) (void)hipStreamSynchronize(n->last_stream);
  if (n->reader_pending) (void)hipEventSynchronize(n->reader_event);
  handle_close(n);
  if (n->writer_event) (void)hipEventDestroy(n->writer_event);
  if (n->reader_event) (void)hipEventDestroy(n->reader_event);
  delete n;
  return FLEET_OK;
}

const char* fleet_norm_last_error(fleet_norm_handle n) { return n ? n->error.c_str() : g_norm_create_error.c_str(); }

int fleet_norm_set_stream(fleet_norm_handle n, void* hip_stream) {
  if (!n) return FLEET_ERR_INVALID;
  FLEET_HANDLE_TRY(n, hipSetDevice(n->device));
  FLEET_HANDLE_TRY(n, hipStreamSynchronize(n->last_stream));
  n->stream = static_cast<hipStream_t>(hip_stream);  // (NULL is the null stream: torch's default stream has that handle)
  n->last_stream = n->stream;
  return FLEET_OK;
}

int fleet_norm_configure(fleet_norm_handle n, const FleetNormParams* p) {
  if (!n) return FLEET_ERR_INVALID;
  if (const char* why = validate(p)) {
    n->error = why;
    return FLEET_ERR_INVALID;
  }
  if (p->num_envs != n->E || p->obs_dim != n->D) {
    n->error = "fleet_norm_configure: num_envs and obs_dim are fixed at creation";
    return FLEET_ERR_INVALID;
  }
  FLEET_HANDLE_TRY(n, hipSetDevice(n->device));
  FLEET_HANDLE_TRY(n, hipStreamSynchronize(n->last_stream));
  if (n->reader_pending) FLEET_HANDLE_TRY(n, wait_reader(n, nullptr, true));
  n->p = *p;
  FLEET_HANDLE_TRY(n, derive(n, n->stream));
  n->last_stream = n->stream;
  return FLEET_OK;
}

int fleet_norm_reset_dev(fleet_norm_handle n, const float* raw_obs, float* obs) {
  if (!n) return FLEET_ERR_INVALID;
  if (!raw_obs || !obs) {
    n->error = "fleet_norm_reset_dev: null buffer";
    return FLEET_ERR_INVALID;
  }
  FLEET_HANDLE_TRY(n, hipSetDevice(n->device));
  FLEET_HANDLE_TRY(n, fleet_norm_enqueue_reset(n, raw_obs, obs, n->stream));
  return FLEET_OK;
}

int fleet_norm_step_dev(fleet_norm_handle n, const float* raw_obs, const double* raw_reward, const uint8_t* done,
                        const float* raw_terminal, float* obs, double* reward, float* terminal) {
  if (!n) return FLEET_ERR_INVALID;
  if (!raw_obs || !raw_reward || !done || !obs || !reward) {
    n->error = "fleet_norm_step_dev: null buffer";
    return FLEET_ERR_INVALID;
  }
  FLEET_HANDLE_TRY(n, hipSetDevice(n->device));
  FLEET_HANDLE_TRY(n, fleet_norm_enqueue_step(n, raw_obs, raw_reward, done, raw_terminal, obs, reward, terminal, n->stream));
  return FLEET_OK;
}

int fleet_norm_get_state(fleet_norm_handle n, double* obs_mean, double* obs_var, double* obs_count, double* ret_mean,
                         double* ret_var, double* ret_count, double* returns) {
  if (!n) return FLEET_ERR_INVALID;
  FLEET_HANDLE_TRY(n, hipSetDevice(n->device));
  FLEET_HANDLE_TRY(n, hipStreamSynchronize(n->last_stream));
  const size_t D = n->D, E = n->E;
  if (obs_mean) FLEET_HANDLE_TRY(n, hipMemcpy(obs_mean, n->obs_mean, D * 8, hipMemcpyDeviceToHost));
  if (obs_var) FLEET_HANDLE_TRY(n, hipMemcpy(obs_var, n->obs_var, D * 8, hipMemcpyDeviceToHost));
  if (returns) FLEET_HANDLE_TRY(n, hipMemcpy(returns, n->returns, E * 8, hipMemcpyDeviceToHost));
  double rs[4];
  FLEET_HANDLE_TRY(n, hipMemcpy(rs, n->ret_stat, sizeof rs, hipMemcpyDeviceToHost));
  if (ret_mean) *ret_mean = rs[0];
  if (ret_var) *ret_var = rs[1];
  if (obs_count) *obs_count = n->obs_count;
  if (ret_count) *ret_count = n->ret_count;
  return FLEET_OK;
}

int fleet_norm_set_state(fleet_norm_handle n, const double* obs_mean, const double* obs_var, const double* obs_count,
                         const double* ret_mean, const double* ret_var, const double* ret_count, const double* returns) {
  if (!n) return FLEET_ERR_INVALID;
  const size_t D = n->D, E = n->E;
  for (const double* c : {obs_count, ret_count})
    if (c && !(*c > 0)) {
      n->error = "fleet_norm_set_state: counts must be > 0";
      return FLEET_ERR_INVALID;
    }
  auto bad_var = [](const double* v, size_t k) {
    for (size_t i = 0; v && i < k; ++i)
      if (!(v[i] >= 0)) return true;
    return false;
  };
  if (bad_var(obs_var, D) || bad_var(ret_var, 1)) {
    n->error = "fleet_norm_set_state: variances must be >= 0";
    return FLEET_ERR_INVALID;
  }
  FLEET_HANDLE_TRY(n, hipSetDevice(n->device));
  FLEET_HANDLE_TRY(n, hipStreamSynchronize(n->last_stream));
  if (n->reader_pending) FLEET_HANDLE_TRY(n, wait_reader(n, nullptr, true));
  if (obs_mean) FLEET_HANDLE_TRY(n, hipMemcpy(n->obs_mean, obs_mean, D * 8, hipMemcpyHostToDevice));
  if (obs_var) FLEET_HANDLE_TRY(n, hipMemcpy(n->obs_var, obs_var, D * 8, hipMemcpyHostToDevice));
  if (returns) FLEET_HANDLE_TRY(n, hipMemcpy(n->returns, returns, E * 8, hipMemcpyHostToDevice));
  if (ret_mean) FLEET_HANDLE_TRY(n, hipMemcpy(n->ret_stat + 0, ret_mean, 8, hipMemcpyHostToDevice));
  if (ret_var) FLEET_HANDLE_TRY(n, hipMemcpy(n->ret_stat + 1, ret_var, 8, hipMemcpyHostToDevice));
  if (obs_count) n->obs_count = *obs_count;
  if (ret_count) n->ret_count = *ret_count;
  FLEET_HANDLE_TRY(n, derive(n, n->stream));
  FLEET_HANDLE_TRY(n, hipStreamSynchronize(n->stream));
  n->last_stream = n->stream;
  return FLEET_OK;
}

int fleet_norm_original_host(fleet_norm_handle n, float* obs, double* reward) {
  if (!n) return FLEET_ERR_INVALID;
  if (obs && !n->last_raw_obs) {
    n->error = "fleet_norm_original_host: no raw observations (no reset / step yet, or the last one normalised in place)";
    return FLEET_ERR_STATE;
  }
  if (reward && !n->have_reward) {
    n->error = "fleet_norm_original_host: no raw rewards (no step yet)";
    return FLEET_ERR_STATE;
  }
  FLEET_HANDLE_TRY(n, hipSetDevice(n->device));
  FLEET_HANDLE_TRY(n, hipStreamSynchronize(n->last_stream));
  if (obs) FLEET_HANDLE_TRY(n, hipMemcpy(obs, n->last_raw_obs, (size_t)n->E * n->D * 4, hipMemcpyDeviceToHost));
  if (reward) FLEET_HANDLE_TRY(n, hipMemcpy(reward, n->raw_reward, (size_t)n->E * 8, hipMemcpyDeviceToHost));
  return FLEET_OK;
}

}  // extern "C"
