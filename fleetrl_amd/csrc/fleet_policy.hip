// fleet_policy.hip -- the deterministic forward pass of a trained MLP policy on the device (include/fleet_hip.h "MLP policy on the
// device"): what stable-baselines3's `predict(obs, deterministic=True)` computes for an MlpPolicy, in one launch whose output
// fleet_step_dev reads directly.
//
// One allocation holds the network's record (PolicyDesc, fleet_policy.h) and every layer's weights, re-laid at upload as
// Wt[in][out] with `out` padded to whole wavefronts: the lanes of a wavefront read consecutive addresses.  That image -- its layout,
// the upload, load_dev's re-lay kernel -- is fleet_mlp.hip's, shared with the target networks.  The kernels here:
//   policy_forward  grid (ceil(E / 16), heads).  A workgroup takes 16 env rows through every layer of one head; the activations
//                   ping-pong between two buffers in the LDS.  A lane owns ONE output column and keeps one accumulator per row in
//                   registers; an activation is read from the LDS by all lanes at the same address (a broadcast), four inputs per
//                   read.  acc = fmaf(x[k], w[k], acc) in ascending k, then + bias: a result depends on its own row and on nothing
//                   else, and for finite inputs it is that chain bit for bit (tests/policy_bits.py restates it; an infinite input
//                   turns a hidden layer's padded columns into inf * 0 = NaN, and with them its row).  The first layer's input is staged 128 columns at a time -- and normalised while it is staged, with
//                   fleet_norm_obs1 (fleet_norm.h), when a normaliser is given -- so D = 1438 needs no whole row in the LDS.
//                   A wavefront works on units of 64 columns x R rows, at most two, which share their LDS reads: R = 16 for layers
//                   of 4..8 column groups, 8 for 2..3, 4 for one (four wavefronts split the rows of a 64-wide layer).
//   policy_forward_sample  fleet_explore_act_dev (include/fleet_hip.h "exploration actions on the device"): the same forward, but
//                   head 0's last layer leaves its 16 rows of means in the LDS, behind the staged input, instead of storing the
//                   transformed output; after a barrier the workgroup runs the sampling epilogue as a phase of its own -- one
//                   thread per (row, 4 columns): one Philox block, two Box-Muller pairs, the action, the env's action and the
//                   log-probability terms, which a wavefront per 4 rows then sums in an order that depends on A alone.  The
//                   critic's workgroups (blockIdx.y = 1) are those of policy_forward.
//   explore_uniform the warm-up's uniform actions: no network.
// Launch boundaries are the only visibility mechanism.  float32 throughout (the normalisation in float64, as everywhere).
// The layer functions (stage, accumulate, run_layer, run_head) live in fleet_policy_dev.h: fleet_qtarget.hip runs them too.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "fleet_mlp.h"
#include "fleet_norm.h"
#include "fleet_philox.h"
#include "fleet_policy.h"
#include "fleet_policy_dev.h"

namespace {

// what the sampling epilogue needs beside the forward's arguments (include/fleet_hip.h FleetExploreArgs)
struct SampleArgs {
  const float *scale, *shift;
  float *noise, *actions, *env_actions, *log_prob, *mean;
  uint64_t seed, step;
  uint32_t env0;  // global id of row 0
  int mode, given;
  float lo, hi;  // ACTION_NOISE: the clip
};

// The epilogue of head 0: means[16][M] (the last layer's output before its transform) -> noise, actions, env_actions, mean; the
// log-probability terms replace the means in place and are summed per row after a barrier.
__device__ __forceinline__ void sample_epilogue(const ForwardArgs& a, const SampleArgs& x, const PolicyHeadDesc* H, float* means, int M,
                                                int A, int row0) {
  const int nb = (A + 3) / 4;  // Philox blocks per row
  const int output = H->output;
  const float hlo = H->lo, hhi = H->hi;
  const bool gauss = x.mode == FLEET_EXPLORE_GAUSSIAN;
  for (int item = threadIdx.x; item < kPolicyRows * nb; item += kPolicyThreads) {
    const int r = item / nb, b = item - r * nb;
    const int row = row0 + r;
    if (row >= a.E) continue;
    const size_t o = (size_t)row * A;
    float z[4];
    row_normals4(x.given, x.noise, o, b, A, x.env0 + (uint32_t)row, x.step, x.seed, z);
    const float4 m4 = *reinterpret_cast<const float4*>(means + r * M + 4 * b);  // (M is a multiple of 64: aligned, inside the row)
    const float mz[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = 4 * b + c;
      if (j >= A) break;
      const float eps = z[c], m = mz[c], sc = x.scale[j];
      if (!x.given && x.noise) x.noise[o + j] = eps;
      float act, env, mu = m;
      if (gauss) {
        const float sd = expf(sc);
        act = fmaf(sd, eps, m);
        env = output_of(act, output, hlo, hhi);
        const float dm = act - m;
        means[r * M + j] = -(dm * dm) / (2.0f * sd * sd) - sc - 0.9189385332f;  // torch's Normal.log_prob on the stored action
      } else {
        mu = output_of(m, output, hlo, hhi);
        const float n = (x.shift ? x.shift[j] : 0.0f) + sc * eps;
        const float v = mu + n;
        act = env = v < x.lo ? x.lo : (v > x.hi ? x.hi : v);
      }
      x.actions[o + j] = act;
      if (x.env_actions) x.env_actions[o + j] = env;
      if (x.mean) x.mean[o + j] = mu;
    }
  }
  if (!x.log_prob) return;  // (uniform over the launch)
  __syncthreads();
  // a wavefront sums 4 rows: every lane its columns lane, lane + 64, ... in ascending order, then a butterfly over the 64 lanes
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = w * (kPolicyRows / kPolicyWaves); r < (w + 1) * (kPolicyRows / kPolicyWaves); ++r) {
    float sum = 0.0f;
    for (int j = lane; j < A; j += 64) sum += means[r * M + j];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0 && row0 + r < a.E) x.log_prob[row0 + r] = sum;
  }
}

template <bool kNorm, bool kSample>
__device__ __forceinline__ void forward_tile(const ForwardArgs& a, const SampleArgs* x) {
  extern __shared__ float lds[];  // two activation buffers [16][S], then the staged input [16][kPolicyChunk]; kSample: then [16][M]
  const PolicyDesc* __restrict__ d = a.desc;
  const PolicyHeadDesc* __restrict__ H = &d->head[blockIdx.y];
  const int S = d->stride;
  float *cur = lds, *nxt = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* means = kSample && blockIdx.y == 0 ? xs + kPolicyRows * kPolicyChunk : nullptr;
  const int row0 = blockIdx.x * kPolicyRows;
  float* gout = blockIdx.y ? a.values : a.actions;
  const int n = H->n_layers;
  run_head<kNorm ? kStageNorm : kStagePlain, kSample>(a, H, cur, nxt, xs, S, row0, gout, means, StageTail{});
  if (kSample && means) sample_epilogue(a, *x, H, means, H->layer[n - 1].out64, H->layer[n - 1].out, row0);
}

template <bool kNorm>
__global__ __launch_bounds__(kPolicyThreads) void policy_forward(ForwardArgs a) {
  forward_tile<kNorm, false>(a, nullptr);
}

template <bool kNorm>
__global__ __launch_bounds__(kPolicyThreads) void policy_forward_sample(ForwardArgs a, SampleArgs x) {
  forward_tile<kNorm, true>(a, &x);
}

// ---- explore_uniform -------------------------------------------------------------------------------------------------------------
// a[e][j] = lo + (hi - lo) * u2 of the column's own word of the row's Philox block, kept below hi; one thread per (row, 4 columns)
__global__ __launch_bounds__(256) void explore_uniform(SampleArgs x, int E, int A) {
  const int nb = (A + 3) / 4;
  const size_t items = (size_t)E * nb;
  for (size_t item = (size_t)blockIdx.x * 256 + threadIdx.x; item < items; item += (size_t)gridDim.x * 256) {
    const size_t row = item / nb;
    const int b = (int)(item - row * nb);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (!x.given) philox_row_block(x.env0 + (uint32_t)row, b, x.step, x.seed, w);
    const float top = x.lo < x.hi ? nextafterf(x.hi, x.lo) : x.lo;  // the largest value of [lo, hi)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = 4 * b + c;
      if (j >= A) break;
      const size_t o = row * A + j;
      const float u = x.given ? x.noise[o] : (float)(w[c] >> 8) * 0x1p-24f;
      if (!x.given && x.noise) x.noise[o] = u;
      float v = x.lo + (x.hi - x.lo) * u;
      if (v > top) v = top;  // (the sum may round up to hi)
      x.actions[o] = v;
      if (x.env_actions) x.env_actions[o] = v;
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_policy_create_error;

std::string validate(const FleetPolicyParams* p) {
  if (!p) return "null FleetPolicyParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetPolicyParams)) return "FleetPolicyParams.struct_bytes does not match this library";
  if (p->obs_dim < 1 || p->obs_dim > FLEET_POLICY_MAX_OBS_DIM)
    return "obs_dim must be in 1.." + std::to_string(FLEET_POLICY_MAX_OBS_DIM) + ", got " + std::to_string(p->obs_dim);
  if (p->n_heads < 1 || p->n_heads > FLEET_POLICY_MAX_HEADS) return "n_heads must be 1 or 2, got " + std::to_string(p->n_heads);
  for (int h = 0; h < p->n_heads; ++h) {
    const std::string why = mlp_validate_head(p->head[h], "head " + std::to_string(h) + ": ");
    if (!why.empty()) return why;
  }
  return "";
}

const char* const kHeadName[FLEET_POLICY_MAX_HEADS] = {"head 0", "head 1"};
const MlpNames kPolicyNames = {kHeadName, "policy", "policy", ""};

}  // namespace

struct FleetPolicy : FleetMlpHandle {
  FleetPolicyParams p{};
  PolicyDesc desc{};
  size_t lds_bytes = 0;         // of one workgroup of policy_forward
  size_t sample_lds_bytes = 0;  // ... of policy_forward_sample: the means of head 0's last layer behind it
};
static_assert(mlp_image_is_first_base<FleetPolicy>, "mlp_borrow (fleet_mlp.hip) reads a fleet_policy_handle as the image's handle");

// the uniform draw's one launch site (fleet_policy.h)
hipError_t policy_launch_uniform(hipStream_t stream, int E, int A, const PolicyUniformArgs& u) {
  SampleArgs s{};
  s.noise = u.noise, s.actions = u.actions, s.env_actions = u.env_actions;
  s.seed = u.seed, s.step = u.step, s.env0 = u.env0;
  s.mode = FLEET_EXPLORE_UNIFORM, s.given = u.given, s.lo = u.lo, s.hi = u.hi;
  hipLaunchKernelGGL(explore_uniform, dim3(grid_for((size_t)E * ((A + 3) / 4), 256, 4096)), dim3(256), 0, stream, s, E, A);
  return hipGetLastError();
}

extern "C" {

int fleet_policy_create(int device, const FleetPolicyParams* p, const float* host_weights, fleet_policy_handle* out) {
  if (out) *out = nullptr;
  std::string why = validate(p);  // before the device is touched
  if (why.empty() && !host_weights) why = "null host_weights";
  if (why.empty() && !out) why = "null output handle";
  if (!why.empty()) {
    g_policy_create_error = why;
    return FLEET_ERR_INVALID;
  }
  FleetPolicy* h = new FleetPolicy();
  h->p = *p;
  h->p.tile_rows = kPolicyRows;
  h->desc.obs_dim = p->obs_dim, h->desc.n_heads = p->n_heads;
  const FleetPolicyHead* const heads[FLEET_POLICY_MAX_HEADS] = {&p->head[0], &p->head[1]};
  const int first_in[FLEET_POLICY_MAX_HEADS] = {p->obs_dim, p->obs_dim};
  h->record = &h->desc, h->record_bytes = sizeof(PolicyDesc), h->nets = h->desc.head, h->n_nets = p->n_heads, h->names = &kPolicyNames;
  h->floats = mlp_describe_layout(heads, first_in, p->n_heads, sizeof(PolicyDesc), h->desc.head, &h->desc.stride);
  h->lds_bytes = ((size_t)2 * kPolicyRows * h->desc.stride + (size_t)kPolicyRows * kPolicyChunk) * sizeof(float);
  h->sample_lds_bytes = h->lds_bytes + (size_t)kPolicyRows * h->desc.head[0].layer[p->head[0].n_layers - 1].out64 * sizeof(float);
  // (a hidden layer wider than 448 takes the forward past the 64 KiB a launch gets unasked)
  constexpr int kMaxLds = (2 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk) * (int)sizeof(float);
  constexpr int kMaxSampleLds = kMaxLds + kPolicyRows * FLEET_POLICY_MAX_WIDTH * (int)sizeof(float);
  const int rc = mlp_open(h, device, host_weights,
                          {{reinterpret_cast<const void*>(&policy_forward<false>), kMaxLds},
                           {reinterpret_cast<const void*>(&policy_forward<true>), kMaxLds},
                           {reinterpret_cast<const void*>(&policy_forward_sample<false>), kMaxSampleLds},
                           {reinterpret_cast<const void*>(&policy_forward_sample<true>), kMaxSampleLds}},
                          &g_policy_create_error);
  if (rc != FLEET_OK) {
    fleet_policy_destroy(h);
    return rc;
  }
  *out = h;
  return FLEET_OK;
}

int fleet_policy_destroy(fleet_policy_handle h) {
  if (!h) return FLEET_OK;
  handle_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_policy_last_error(fleet_policy_handle h) { return h ? h->error.c_str() : g_policy_create_error.c_str(); }

int fleet_policy_set_stream(fleet_policy_handle h, void* hip_stream) { return h ? handle_set_stream(h, hip_stream) : FLEET_ERR_INVALID; }

int fleet_policy_load_host(fleet_policy_handle h, const float* weights) {
  return h ? mlp_load_host(h, "fleet_policy_load_host", weights) : FLEET_ERR_INVALID;
}

int fleet_policy_load_dev(fleet_policy_handle h, const float* const* tensors, int count) {
  if (!h) return FLEET_ERR_INVALID;
  return mlp_launch_relay(h, kMlpLoad, "fleet_policy_load_dev", const_cast<float* const*>(tensors), count, 0.0f, 0.0f);  // (read only)
}

int fleet_policy_forward_dev(fleet_policy_handle h, const float* obs, int E, fleet_norm_handle norm, float* actions, float* values) {
  if (!h) return FLEET_ERR_INVALID;
  if (!obs || !actions) {
    h->error = "fleet_policy_forward_dev: null obs or actions";
    return FLEET_ERR_INVALID;
  }
  if (E < 1) {
    h->error = "fleet_policy_forward_dev: E must be >= 1, got " + std::to_string(E);
    return FLEET_ERR_INVALID;
  }
  if (values && h->p.n_heads < 2) {
    h->error = "fleet_policy_forward_dev: values asked of a policy without a critic head";
    return FLEET_ERR_INVALID;
  }
  ForwardArgs a{};
  a.desc = reinterpret_cast<const PolicyDesc*>(h->block);
  a.base = reinterpret_cast<const float*>(h->block);
  a.obs = obs, a.actions = actions, a.values = values, a.E = E;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  bool norm_obs;
  MlpNormStats ns{};
  if (const int rc = mlp_bind_norm(h, h->p.obs_dim, "policy", "fleet_policy_forward_dev", norm, &ns, &norm_obs); rc != FLEET_OK) return rc;
  a.mean = ns.mean, a.sd = ns.sd, a.clip = ns.clip;
  const dim3 grid((unsigned)(((size_t)E + kPolicyRows - 1) / kPolicyRows), values ? 2 : 1), block(kPolicyThreads);
  if (norm_obs) hipLaunchKernelGGL(policy_forward<true>, grid, block, h->lds_bytes, h->stream, a);
  else hipLaunchKernelGGL(policy_forward<false>, grid, block, h->lds_bytes, h->stream, a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  if (norm) FLEET_HANDLE_TRY(h, fleet_norm_end_read(norm, h->stream));
  return FLEET_OK;
}

int fleet_policy_describe(fleet_policy_handle h, FleetPolicyParams* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  *out = h->p;
  return FLEET_OK;
}

int fleet_explore_act_dev(fleet_policy_handle h, const float* obs, int E, fleet_norm_handle norm, const FleetExploreArgs* args) {
  if (!h) return FLEET_ERR_INVALID;
  const auto refuse = [h](const std::string& why) {
    h->error = "fleet_explore_act_dev: " + why;
    return FLEET_ERR_INVALID;
  };
  if (!args) return refuse("null FleetExploreArgs");
  const FleetExploreArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetExploreArgs)) return refuse("FleetExploreArgs.struct_bytes does not match this library");
  if (x.mode != FLEET_EXPLORE_GAUSSIAN && x.mode != FLEET_EXPLORE_ACTION_NOISE && x.mode != FLEET_EXPLORE_UNIFORM)
    return refuse("unknown mode " + std::to_string(x.mode));
  if (x.noise_mode != FLEET_EXPLORE_NOISE_DRAW && x.noise_mode != FLEET_EXPLORE_NOISE_GIVEN)
    return refuse("unknown noise_mode " + std::to_string(x.noise_mode));
  const bool uniform = x.mode == FLEET_EXPLORE_UNIFORM;
  if (E < 1) return refuse("E must be >= 1, got " + std::to_string(E));
  if (!x.actions) return refuse("null actions");
  if (!uniform && !obs) return refuse("null obs");
  if (!uniform && !x.scale) return refuse("null scale (log_std or sigma)");
  if (x.log_prob && x.mode != FLEET_EXPLORE_GAUSSIAN) return refuse("log_prob asked outside the GAUSSIAN mode");
  if (x.values && uniform) return refuse("values asked in the UNIFORM mode: no network runs");
  if (x.values && h->p.n_heads < 2) return refuse("values asked of a policy without a critic head");
  if (x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN && !x.noise) return refuse("noise_mode GIVEN with a null noise");
  // (GAUSSIAN does not read the bounds: the head's own clip is its transform)
  if (x.mode != FLEET_EXPLORE_GAUSSIAN && !(x.noise_lo <= x.noise_hi)) return refuse("the bounds need noise_lo <= noise_hi");
  if (x.env_id_offset < 0) return refuse("env_id_offset must be >= 0, got " + std::to_string(x.env_id_offset));
  SampleArgs s{};
  s.scale = x.scale, s.shift = x.shift, s.noise = x.noise, s.actions = x.actions, s.env_actions = x.env_actions;
  s.log_prob = x.log_prob, s.mean = x.mean, s.seed = x.seed, s.step = x.step, s.env0 = (uint32_t)x.env_id_offset;
  s.mode = x.mode, s.given = x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN, s.lo = x.noise_lo, s.hi = x.noise_hi;
  const int A = h->p.head[0].width[h->p.head[0].n_layers - 1];
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  if (uniform) {
    const PolicyUniformArgs u{s.noise, s.actions, s.env_actions, s.seed, s.step, s.env0, s.given, s.lo, s.hi};
    FLEET_HANDLE_TRY(h, policy_launch_uniform(h->stream, E, A, u));
    return FLEET_OK;
  }
  ForwardArgs a{};
  a.desc = reinterpret_cast<const PolicyDesc*>(h->block);
  a.base = reinterpret_cast<const float*>(h->block);
  a.obs = obs, a.actions = nullptr, a.values = x.values, a.E = E;
  bool norm_obs;
  MlpNormStats ns{};
  if (const int rc = mlp_bind_norm(h, h->p.obs_dim, "policy", "fleet_explore_act_dev", norm, &ns, &norm_obs); rc != FLEET_OK) return rc;
  a.mean = ns.mean, a.sd = ns.sd, a.clip = ns.clip;
  const dim3 grid((unsigned)(((size_t)E + kPolicyRows - 1) / kPolicyRows), x.values ? 2 : 1), block(kPolicyThreads);
  if (norm_obs) hipLaunchKernelGGL(policy_forward_sample<true>, grid, block, h->sample_lds_bytes, h->stream, a, s);
  else hipLaunchKernelGGL(policy_forward_sample<false>, grid, block, h->sample_lds_bytes, h->stream, a, s);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  if (norm) FLEET_HANDLE_TRY(h, fleet_norm_end_read(norm, h->stream));
  return FLEET_OK;
}

}  // extern "C"
