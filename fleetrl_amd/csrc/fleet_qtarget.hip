// fleet_qtarget.hip -- the target networks of a TD3 / DDPG agent on the device (include/fleet_hip.h "TD3 / DDPG learning targets on
// the device"): the bootstrap target of a minibatch in one launch, the Polyak update in one launch, loads and the export.
//
// One allocation holds the record (QTargetDesc) and every layer's weights of the actor, critic 0 and critic 1: the image of
// fleet_mlp.h, which the policy keeps too.  Its layout, the uploads and the kernel behind load_dev, polyak_dev and export_dev (mlp_relay:
// only real elements are visited, t' = fmaf(tau, p, t * omt)) are fleet_mlp.hip's.  The kernel here:
//   qtarget_target  grid ceil(B / 16).  A workgroup of 256 threads takes 16 rows through the ACTOR with the layer functions of
//                   fleet_policy_dev.h; its last layer leaves the rows untransformed in the LDS, act[16][A64], as
//                   policy_forward_sample's does.  An epilogue phase -- one thread per (row, 4 columns) -- turns them into the
//                   target action a' in place.  The SAME workgroup then runs critic 0 and critic 1, one after the other: their first
//                   layer stages its input 128 columns at a time, columns below D from next_obs in global memory, columns D .. D+A-1
//                   from act[][] in the LDS, zeros behind.  A critic's last layer (64 padded columns) goes to the activation buffer
//                   its layer before did not read; threads 0..15 pick column 0 of their row up into a register.  The final phase
//                   is those 16 threads: q, qmin, y.
//                   LDS: two activation buffers [16][S], S the widest hidden layer of all three networks, the staged chunk
//                   [16][128], act [16][A64]: 20 KiB .. 104 KiB.
// Launch boundaries are the only visibility mechanism; no atomics.  float32 throughout.
#include <hip/hip_runtime.h>

#include <string>

#include "fleet_mlp.h"
#include "fleet_philox.h"
#include "fleet_policy.h"
#include "fleet_policy_dev.h"
#include "fleet_qtarget.h"

namespace {

struct TargetArgs {
  const QTargetDesc* desc;
  const float* base;
  const float *next_obs, *rewards, *dones, *sigma;
  float *noise, *target_q, *next_actions, *q;
  uint64_t seed, step;
  uint32_t row_id0;  // global id of row 0
  int given, B;
  float gamma, noise_clip, lo, hi;
};

// act[16][M]: the actor's last layer before its transform -> a' in place; the optional noise and next_actions
__device__ __forceinline__ void action_epilogue(const TargetArgs& t, const PolicyHeadDesc* H, float* act, int M, int A, int row0) {
  const int nb = (A + 3) / 4;  // Philox blocks per row
  const int output = H->output;
  const float hlo = H->lo, hhi = H->hi;
  const float nlo = -t.noise_clip, nhi = t.noise_clip;
  for (int item = threadIdx.x; item < kPolicyRows * nb; item += kPolicyThreads) {
    const int r = item / nb, b = item - r * nb;
    const int row = row0 + r;
    if (row >= t.B) continue;  // (such a row keeps the untransformed numbers: the critics run on them and nobody reads the result)
    const size_t o = (size_t)row * A;
    float z[4];
    row_normals4(t.given, t.noise, o, b, A, t.row_id0 + (uint32_t)row, t.step, t.seed, z);
    const float4 m4 = *reinterpret_cast<const float4*>(act + r * M + 4 * b);  // (M is a multiple of 64: aligned, inside the row)
    const float mz[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = 4 * b + c;
      if (j >= A) break;
      const float eps = z[c];
      if (!t.given && t.noise) t.noise[o + j] = eps;
      const float d = output_of(mz[c], output, hlo, hhi);
      float n = t.sigma[j] * eps;
      n = n < nlo ? nlo : (n > nhi ? nhi : n);
      float v = d + n;
      v = v < t.lo ? t.lo : (v > t.hi ? t.hi : v);
      act[r * M + j] = v;
      if (t.next_actions) t.next_actions[o + j] = v;
    }
  }
}

__global__ __launch_bounds__(kPolicyThreads) void qtarget_target(TargetArgs t) {
  extern __shared__ float lds[];  // two activation buffers [16][S], the staged input [16][kPolicyChunk], act [16][M]
  const QTargetDesc* __restrict__ d = t.desc;
  const int S = d->stride, D = d->obs_dim, A = d->act_dim, M = d->act64, nc = d->n_critics;
  float *buf0 = lds, *buf1 = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* act = xs + kPolicyRows * kPolicyChunk;
  const int row0 = blockIdx.x * kPolicyRows;
  ForwardArgs a{};
  a.base = t.base, a.obs = t.next_obs, a.E = t.B;
  run_head<kStagePlain, true>(a, &d->net[0], buf0, buf1, xs, S, row0, nullptr, act, StageTail{});
  action_epilogue(t, &d->net[0], act, M, A, row0);
  __syncthreads();
  const StageTail tail{act, M, D};
  float q0 = 0.0f, q1 = 0.0f;
  {
    const PolicyHeadDesc* H = &d->net[1];
    float* qrows = (H->n_layers - 1) & 1 ? buf0 : buf1;  // the buffer the last layer does not read (run_head)
    run_head<kStageConcat, true>(a, H, buf0, buf1, xs, S, row0, nullptr, qrows, tail);
    if (threadIdx.x < kPolicyRows) q0 = qrows[threadIdx.x * 64];  // (before the next head's first barrier: nobody has written yet)
  }
  if (nc == 2) {
    const PolicyHeadDesc* H = &d->net[2];
    float* qrows = (H->n_layers - 1) & 1 ? buf0 : buf1;
    run_head<kStageConcat, true>(a, H, buf0, buf1, xs, S, row0, nullptr, qrows, tail);
    if (threadIdx.x < kPolicyRows) q1 = qrows[threadIdx.x * 64];
  }
  const int row = row0 + (int)threadIdx.x;
  if (threadIdx.x < kPolicyRows && row < t.B) {
    if (t.q) {
      t.q[(size_t)row * nc] = q0;
      if (nc == 2) t.q[(size_t)row * nc + 1] = q1;
    }
    const float qmin = nc == 2 ? (q1 < q0 ? q1 : q0) : q0;
    const float keep = (1.0f - t.dones[row]) * t.gamma;
    const float boot = keep * qmin;  // (its own rounding: -ffp-contract=off, and no fmaf here)
    t.target_q[row] = t.rewards[row] + boot;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_qtarget_error;  // of the last failed call without a handle

std::string validate(const FleetQTargetParams* p) {
  if (!p) return "null FleetQTargetParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetQTargetParams)) return "FleetQTargetParams.struct_bytes does not match this library";
  if (p->obs_dim < 1 || p->obs_dim > FLEET_POLICY_MAX_OBS_DIM)
    return "obs_dim must be in 1.." + std::to_string(FLEET_POLICY_MAX_OBS_DIM) + ", got " + std::to_string(p->obs_dim);
  if (p->n_critics < 1 || p->n_critics > 2) return "n_critics must be 1 or 2, got " + std::to_string(p->n_critics);
  std::string why = mlp_validate_head(p->actor, "actor: ");
  if (!why.empty()) return why;
  const int A = p->actor.width[p->actor.n_layers - 1];
  if (p->obs_dim + A > FLEET_POLICY_MAX_OBS_DIM)
    return "obs_dim + act_dim must be at most " + std::to_string(FLEET_POLICY_MAX_OBS_DIM) + " (a critic's input), got " +
           std::to_string(p->obs_dim) + " + " + std::to_string(A);
  for (int c = 0; c < p->n_critics; ++c) {
    const std::string who = "critic " + std::to_string(c) + ": ";
    why = mlp_validate_head(p->critic[c], who);
    if (!why.empty()) return why;
    if (p->critic[c].width[p->critic[c].n_layers - 1] != 1)
      return who + "the last width must be 1, got " + std::to_string(p->critic[c].width[p->critic[c].n_layers - 1]);
    if (p->critic[c].output != FLEET_POLICY_OUT_NONE) return who + "the output transform must be NONE";
  }
  return "";
}

const char* const kNetName[kQNets] = {"actor", "critic 0", "critic 1"};
const MlpNames kTargetNames = {kNetName, "target networks", "target", "fleet_qtarget_create: "};


// what fleet_qtarget_target_dev refuses, looked at without the handle; "" when the arguments pass
std::string check_target_args(const float* next_obs, const float* rewards, const float* dones, int B, const FleetQTargetArgs* args) {
  if (!args) return "null FleetQTargetArgs";
  const FleetQTargetArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetQTargetArgs)) return "FleetQTargetArgs.struct_bytes does not match this library";
  if (x.noise_mode != FLEET_EXPLORE_NOISE_DRAW && x.noise_mode != FLEET_EXPLORE_NOISE_GIVEN)
    return "unknown noise_mode " + std::to_string(x.noise_mode);
  if (B < 1) return "B must be >= 1, got " + std::to_string(B);
  if (!next_obs) return "null next_obs";
  if (!rewards) return "null rewards";
  if (!dones) return "null dones";
  if (!x.sigma) return "null sigma";
  if (!x.target_q) return "null target_q";
  if (!(x.act_lo <= x.act_hi)) return "the bounds need act_lo <= act_hi";
  if (!(x.noise_clip >= 0.0f)) return "noise_clip must be >= 0";
  if (x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN && !x.noise) return "noise_mode GIVEN with a null noise";
  if (x.row_offset < 0) return "row_offset must be >= 0, got " + std::to_string(x.row_offset);
  return "";
}

}  // namespace

extern "C" {

int fleet_qtarget_create(int device, const FleetQTargetParams* p, const float* host_weights, fleet_qtarget_handle* out) {
  if (out) *out = nullptr;
  std::string why = validate(p);  // before the device is touched
  if (why.empty() && !host_weights) why = "null host_weights";
  if (why.empty() && !out) why = "null output handle";
  if (!why.empty()) {
    g_qtarget_error = "fleet_qtarget_create: " + why;
    return FLEET_ERR_INVALID;
  }
  FleetQTarget* h = new FleetQTarget();
  h->p = *p;
  h->p.tile_rows = kPolicyRows;
  const int A = p->actor.width[p->actor.n_layers - 1];
  h->desc.obs_dim = p->obs_dim, h->desc.act_dim = A, h->desc.n_critics = p->n_critics, h->desc.act64 = mlp_round_up(A, 64);
  const FleetPolicyHead* const heads[kQNets] = {&p->actor, &p->critic[0], &p->critic[1]};
  const int first_in[kQNets] = {p->obs_dim, p->obs_dim + A, p->obs_dim + A};
  h->record = &h->desc, h->record_bytes = sizeof(QTargetDesc), h->nets = h->desc.net, h->n_nets = 1 + p->n_critics, h->names = &kTargetNames;
  h->floats = mlp_describe_layout(heads, first_in, h->n_nets, sizeof(QTargetDesc), h->desc.net, &h->desc.stride);
  h->lds_bytes = ((size_t)2 * kPolicyRows * h->desc.stride + (size_t)kPolicyRows * kPolicyChunk + (size_t)kPolicyRows * h->desc.act64) * sizeof(float);
  constexpr int kMaxLds = (3 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk) * (int)sizeof(float);
  const int rc = mlp_open(h, device, host_weights, {{reinterpret_cast<const void*>(&qtarget_target), kMaxLds}}, &g_qtarget_error);
  if (rc != FLEET_OK) {
    fleet_qtarget_destroy(h);
    return rc;
  }
  *out = h;
  return FLEET_OK;
}

int fleet_qtarget_destroy(fleet_qtarget_handle h) {
  if (!h) return FLEET_OK;
  handle_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_qtarget_last_error(fleet_qtarget_handle h) { return h ? h->error.c_str() : g_qtarget_error.c_str(); }

int fleet_qtarget_set_stream(fleet_qtarget_handle h, void* hip_stream) { return h ? handle_set_stream(h, hip_stream) : FLEET_ERR_INVALID; }

int fleet_qtarget_load_host(fleet_qtarget_handle h, const float* weights) {
  return h ? mlp_load_host(h, "fleet_qtarget_load_host", weights) : FLEET_ERR_INVALID;
}

int fleet_qtarget_load_dev(fleet_qtarget_handle h, const float* const* tensors, int count) {
  if (!h) return FLEET_ERR_INVALID;
  return mlp_launch_relay(h, kMlpLoad, "fleet_qtarget_load_dev", const_cast<float* const*>(tensors), count, 0.0f, 0.0f);  // (read only)
}

int fleet_qtarget_polyak_dev(fleet_qtarget_handle h, const float* const* tensors, int count, double tau) {
  if (!h) return FLEET_ERR_INVALID;
  if (!(tau >= 0.0 && tau <= 1.0)) {
    h->error = "fleet_qtarget_polyak_dev: tau must be in [0, 1], got " + std::to_string(tau);
    return FLEET_ERR_INVALID;
  }
  return mlp_launch_relay(h, kMlpPolyak, "fleet_qtarget_polyak_dev", const_cast<float* const*>(tensors), count, (float)tau, (float)(1.0 - tau));
}

int fleet_qtarget_export_dev(fleet_qtarget_handle h, float* const* tensors, int count) {
  if (!h) return FLEET_ERR_INVALID;
  return mlp_launch_relay(h, kMlpExport, "fleet_qtarget_export_dev", tensors, count, 0.0f, 0.0f);
}

int fleet_qtarget_target_dev(fleet_qtarget_handle h, const float* next_obs, const float* rewards, const float* dones, int B,
                             const FleetQTargetArgs* args) {
  const std::string why = check_target_args(next_obs, rewards, dones, B, args);
  if (const int rc = handle_enter("fleet_qtarget_target_dev", why, h, g_qtarget_error); rc != FLEET_OK) return rc;
  if (qtarget_squashed(h)) {  // (the actor's last layer is (mu, log_std): fleet_sac_target_dev is its target)
    h->error = "fleet_qtarget_target_dev: the handle's actor is a squashed Gaussian (fleet_sac_create): use fleet_sac_target_dev";
    return FLEET_ERR_INVALID;
  }
  const FleetQTargetArgs& x = *args;
  TargetArgs t{};
  t.desc = reinterpret_cast<const QTargetDesc*>(h->block);
  t.base = reinterpret_cast<const float*>(h->block);
  t.next_obs = next_obs, t.rewards = rewards, t.dones = dones, t.sigma = x.sigma;
  t.noise = x.noise, t.target_q = x.target_q, t.next_actions = x.next_actions, t.q = x.q;
  t.seed = x.seed, t.step = x.step, t.row_id0 = (uint32_t)x.row_offset;
  t.given = x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN, t.B = B;
  t.gamma = x.gamma, t.noise_clip = x.noise_clip, t.lo = x.act_lo, t.hi = x.act_hi;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  const dim3 grid((unsigned)(((size_t)B + kPolicyRows - 1) / kPolicyRows)), block(kPolicyThreads);
  hipLaunchKernelGGL(qtarget_target, grid, block, h->lds_bytes, h->stream, t);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

int fleet_qtarget_describe(fleet_qtarget_handle h, FleetQTargetParams* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  *out = h->p;
  return FLEET_OK;
}

}  // extern "C"
