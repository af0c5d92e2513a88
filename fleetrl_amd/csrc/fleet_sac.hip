// fleet_sac.hip -- the forward side of a SAC agent on the device (include/fleet_hip.h "SAC on the device"): the stochastic squashed-
// Gaussian actor's action with its log-probability in one launch, and the entropy-regularised bootstrap target of a minibatch in one
// launch.  The networks live in a fleet_qtarget handle (fleet_qtarget.h) that fleet_sac_create makes: the actor is ONE chain whose last
// layer is 2A wide -- rows 0..A-1 mu, rows A..2A-1 log_std -- so the weight image, its relay kernel, the critic gradient launches and
// Adam serve it as they are; QTargetDesc::reserved[kQSquashed] marks it.  The layer functions are fleet_policy_dev.h's.  The kernels:
//   sac_act     grid ceil(E / 16), 256 threads.  A workgroup takes 16 rows through the actor; the last layer leaves its 2A columns
//               untransformed in the LDS, hd[16][M2] (M2 = 2A rounded up to 64), as policy_forward_sample's does.  The epilogue -- one
//               (fleet_sac_dev.h) -- one thread per (row, 4 action columns): one Philox block, the draw of fleet_explore_act_dev -- forms ls, u, a and the two
//               log-probability terms, which replace mu (t) and log_std (c) in place; after a barrier a wavefront per 4 rows sums
//               each in the order fleet_explore_act_dev sums (a function of A alone) and lane 0 stores S(t) - S(c).
//   sac_target  grid ceil(B / 16).  The same actor phase and the SAME epilogue function on the ONLINE image, a' to act[16][A64] in the
//               LDS and the row's log-probability to 16 row scalars; then the workgroup runs critic 0 and critic 1 of the TARGETS
//               image from act[][] as qtarget_target does (kStageConcat); threads 0..15 form q, qmin and y.  Two image bases; the
//               LDS and its row stride are the larger of the two handles' needs.
//   LDS: two activation buffers [16][S], the staged chunk [16][128], hd [16][M2] (sac_target: act [16][A64] and 16 scalars behind it):
//        sac_act 20 KiB .. 104 KiB, sac_target 24.1 KiB .. 120.1 KiB.
// Launch boundaries are the only visibility mechanism; no atomics.  float32 throughout (the normalisation in float64, as everywhere).
#include <hip/hip_runtime.h>

#include <string>

#include "fleet_mlp.h"
#include "fleet_norm.h"
#include "fleet_philox.h"
#include "fleet_policy.h"
#include "fleet_policy_dev.h"
#include "fleet_qtarget.h"
#include "fleet_sac_dev.h"

namespace {

struct ActArgs {
  ForwardArgs f;  // desc is not read: the record is `desc` below
  const QTargetDesc* desc;
  SacEpilogue x;
};

template <bool kNorm>
__global__ __launch_bounds__(kPolicyThreads) void sac_act(ActArgs t) {
  extern __shared__ float lds[];  // two activation buffers [16][S], the staged input [16][kPolicyChunk], hd [16][M2]
  const QTargetDesc* __restrict__ d = t.desc;
  const PolicyHeadDesc* __restrict__ H = &d->net[0];
  const int S = d->stride, A = d->act_dim;
  float *cur = lds, *nxt = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* hd = xs + kPolicyRows * kPolicyChunk;
  const int row0 = blockIdx.x * kPolicyRows;
  run_head<kNorm ? kStageNorm : kStagePlain, true>(t.f, H, cur, nxt, xs, S, row0, nullptr, hd, StageTail{});
  sac_epilogue(t.x, hd, H->layer[H->n_layers - 1].out64, A, t.f.E, row0, nullptr, 0, nullptr, nullptr, 0);
}

struct SoftTargetArgs {
  const QTargetDesc *online, *targets;  // the two records, in their blocks
  const float *online_base, *targets_base;
  const float *next_obs, *rewards, *dones, *ent_coef;
  float *target_q, *q;
  SacEpilogue x;
  int B, S;  // S: the larger of the two records' strides
  float gamma;
};

__global__ __launch_bounds__(kPolicyThreads) void sac_target(SoftTargetArgs t) {
  extern __shared__ float lds[];  // two buffers [16][S], the staged input [16][kPolicyChunk], hd [16][M2], act [16][M], lp [16]
  const QTargetDesc* __restrict__ on = t.online;
  const QTargetDesc* __restrict__ tg = t.targets;
  const PolicyHeadDesc* __restrict__ H0 = &on->net[0];
  const int S = t.S, D = on->obs_dim, A = on->act_dim, M = on->act64, nc = tg->n_critics;
  const int M2 = H0->layer[H0->n_layers - 1].out64;
  float *buf0 = lds, *buf1 = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* hd = xs + kPolicyRows * kPolicyChunk;
  float* act = hd + kPolicyRows * M2;
  float* rowlp = act + kPolicyRows * M;
  const int row0 = blockIdx.x * kPolicyRows;
  ForwardArgs a{};
  a.base = t.online_base, a.obs = t.next_obs, a.E = t.B;
  run_head<kStagePlain, true>(a, H0, buf0, buf1, xs, S, row0, nullptr, hd, StageTail{});
  sac_epilogue(t.x, hd, M2, A, t.B, row0, act, M, rowlp, nullptr, 0);
  __syncthreads();
  a.base = t.targets_base;
  const StageTail tail{act, M, D};
  float q0 = 0.0f, q1 = 0.0f;
  {
    const PolicyHeadDesc* H = &tg->net[1];
    float* qrows = (H->n_layers - 1) & 1 ? buf0 : buf1;  // the buffer the last layer does not read (run_head)
    run_head<kStageConcat, true>(a, H, buf0, buf1, xs, S, row0, nullptr, qrows, tail);
    if (threadIdx.x < kPolicyRows) q0 = qrows[threadIdx.x * 64];  // (before the next head's first barrier: nobody has written yet)
  }
  if (nc == 2) {
    const PolicyHeadDesc* H = &tg->net[2];
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
    const float p = t.ent_coef[0] * rowlp[threadIdx.x];
    const float v = qmin - p;
    const float keep = (1.0f - t.dones[row]) * t.gamma;
    const float boot = keep * v;  // (its own rounding: -ffp-contract=off, and no fmaf here)
    t.target_q[row] = t.rewards[row] + boot;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_sac_error;  // of the last failed call without a handle

std::string validate(const FleetSacParams* p) {
  if (!p) return "null FleetSacParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetSacParams)) return "FleetSacParams.struct_bytes does not match this library";
  if (p->obs_dim < 1 || p->obs_dim > FLEET_POLICY_MAX_OBS_DIM)
    return "obs_dim must be in 1.." + std::to_string(FLEET_POLICY_MAX_OBS_DIM) + ", got " + std::to_string(p->obs_dim);
  if (p->n_critics < 1 || p->n_critics > 2) return "n_critics must be 1 or 2, got " + std::to_string(p->n_critics);
  std::string why = mlp_validate_head(p->actor, "actor: ");
  if (!why.empty()) return why;
  const int W = p->actor.width[p->actor.n_layers - 1];
  if (W % 2 != 0) return "actor: the last width must be even (mu rows, then as many log_std rows), got " + std::to_string(W);
  if (p->actor.output != FLEET_POLICY_OUT_NONE) return "actor: the output transform must be NONE (the squashing is the entry's)";
  const int A = W / 2;
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
const MlpNames kSacNames = {kNetName, "SAC networks", "SAC", ""};

std::string check_noise_mode(int mode) {
  if (mode != FLEET_EXPLORE_NOISE_DRAW && mode != FLEET_EXPLORE_NOISE_GIVEN) return "unknown noise_mode " + std::to_string(mode);
  return "";
}

// what fleet_sac_act_dev refuses, looked at without the handle; "" when the arguments pass
std::string check_act_args(const float* obs, int E, const FleetSacActArgs* args) {
  if (!args) return "null FleetSacActArgs";
  const FleetSacActArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetSacActArgs)) return "FleetSacActArgs.struct_bytes does not match this library";
  if (std::string why = check_noise_mode(x.noise_mode); !why.empty()) return why;
  if (E < 1) return "E must be >= 1, got " + std::to_string(E);
  if (!obs) return "null obs";
  if (!x.actions) return "null actions";
  if (x.deterministic != 0 && x.deterministic != 1) return "deterministic must be 0 or 1, got " + std::to_string(x.deterministic);
  if (x.deterministic) {
    if (x.noise) return "noise given with deterministic: no noise is read or written";
    if (x.log_prob) return "log_prob asked with deterministic";
    if (x.gaussian_actions) return "gaussian_actions asked with deterministic";
  } else if (x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN && !x.noise) {
    return "noise_mode GIVEN with a null noise";
  }
  if (x.env_id_offset < 0) return "env_id_offset must be >= 0, got " + std::to_string(x.env_id_offset);
  return "";
}

std::string check_target_args(const float* next_obs, const float* rewards, const float* dones, int B, const FleetSacTargetArgs* args) {
  if (!args) return "null FleetSacTargetArgs";
  const FleetSacTargetArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetSacTargetArgs)) return "FleetSacTargetArgs.struct_bytes does not match this library";
  if (std::string why = check_noise_mode(x.noise_mode); !why.empty()) return why;
  if (B < 1) return "B must be >= 1, got " + std::to_string(B);
  if (!next_obs) return "null next_obs";
  if (!rewards) return "null rewards";
  if (!dones) return "null dones";
  if (!x.ent_coef) return "null ent_coef";
  if (!x.target_q) return "null target_q";
  if (x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN && !x.noise) return "noise_mode GIVEN with a null noise";
  if (x.row_offset < 0) return "row_offset must be >= 0, got " + std::to_string(x.row_offset);
  return "";
}

// floats of the LDS in front of hd[][]: two activation buffers and the staged chunk
size_t front_floats(int S) { return (size_t)2 * kPolicyRows * S + (size_t)kPolicyRows * kPolicyChunk; }

int refuse(FleetQTarget* h, const char* entry, const std::string& why) {
  h->error = std::string(entry) + ": " + why;
  return FLEET_ERR_INVALID;
}

}  // namespace

extern "C" {

int fleet_sac_create(int device, const FleetSacParams* p, const float* host_weights, fleet_qtarget_handle* out) {
  if (out) *out = nullptr;
  std::string why = validate(p);  // before the device is touched
  if (why.empty() && !host_weights) why = "null host_weights";
  if (why.empty() && !out) why = "null output handle";
  if (!why.empty()) return handle_refuse(g_sac_error, "fleet_sac_create", why, FLEET_ERR_INVALID);
  FleetQTarget* h = new FleetQTarget();
  h->p.struct_bytes = (int32_t)sizeof(FleetQTargetParams);  // (what fleet_qtarget_describe reports: the actor's last width is 2A)
  h->p.obs_dim = p->obs_dim, h->p.n_critics = p->n_critics, h->p.tile_rows = kPolicyRows;
  h->p.actor = p->actor, h->p.critic[0] = p->critic[0], h->p.critic[1] = p->critic[1];
  const int A = p->actor.width[p->actor.n_layers - 1] / 2;
  h->desc.obs_dim = p->obs_dim, h->desc.act_dim = A, h->desc.n_critics = p->n_critics, h->desc.act64 = mlp_round_up(A, 64);
  h->desc.reserved[kQSquashed] = 1;
  const FleetPolicyHead* const heads[kQNets] = {&p->actor, &p->critic[0], &p->critic[1]};
  const int first_in[kQNets] = {p->obs_dim, p->obs_dim + A, p->obs_dim + A};
  h->record = &h->desc, h->record_bytes = sizeof(QTargetDesc), h->nets = h->desc.net, h->n_nets = 1 + p->n_critics, h->names = &kSacNames;
  h->floats = mlp_describe_layout(heads, first_in, h->n_nets, sizeof(QTargetDesc), h->desc.net, &h->desc.stride);
  const int M2 = h->desc.net[0].layer[p->actor.n_layers - 1].out64;
  h->lds_bytes = (front_floats(h->desc.stride) + (size_t)kPolicyRows * (M2 + h->desc.act64 + 1)) * sizeof(float);
  constexpr int kMaxActLds = (3 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk) * (int)sizeof(float);
  constexpr int kMaxTargetLds = kMaxActLds + kPolicyRows * (FLEET_POLICY_MAX_WIDTH / 2 + 1) * (int)sizeof(float);
  const int rc = mlp_open(h, device, host_weights,
                          {{reinterpret_cast<const void*>(&sac_act<false>), kMaxActLds},
                           {reinterpret_cast<const void*>(&sac_act<true>), kMaxActLds},
                           {reinterpret_cast<const void*>(&sac_target), kMaxTargetLds}},
                          &why);
  if (rc != FLEET_OK) {
    fleet_qtarget_destroy(h);
    return handle_refuse(g_sac_error, "fleet_sac_create", why, rc);
  }
  *out = h;
  return FLEET_OK;
}

const char* fleet_sac_last_error(fleet_qtarget_handle h) { return h ? h->error.c_str() : g_sac_error.c_str(); }

int fleet_sac_act_dev(fleet_qtarget_handle h, const float* obs, int E, fleet_norm_handle norm, const FleetSacActArgs* args) {
  const std::string why = check_act_args(obs, E, args);
  if (const int rc = handle_enter("fleet_sac_act_dev", why, h, g_sac_error); rc != FLEET_OK) return rc;
  if (h->record_bytes != sizeof(QTargetDesc) || !qtarget_squashed(h))
    return refuse(h, "fleet_sac_act_dev", "the handle's actor is not a squashed Gaussian: fleet_sac_create makes one");
  const FleetSacActArgs& x = *args;
  ActArgs t{};
  t.desc = reinterpret_cast<const QTargetDesc*>(h->block);
  t.f.base = reinterpret_cast<const float*>(h->block);
  t.f.obs = obs, t.f.E = E;
  t.x.noise = x.noise, t.x.actions = x.actions, t.x.gaussian = x.gaussian_actions, t.x.log_prob = x.log_prob;
  t.x.mean = x.mean, t.x.log_std = x.log_std;
  t.x.seed = x.seed, t.x.step = x.step, t.x.id0 = (uint32_t)x.env_id_offset;
  t.x.given = x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN, t.x.deterministic = x.deterministic;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  bool norm_obs;
  MlpNormStats ns{};
  if (const int rc = mlp_bind_norm(h, h->desc.obs_dim, "networks", "fleet_sac_act_dev", norm, &ns, &norm_obs); rc != FLEET_OK) return rc;
  t.f.mean = ns.mean, t.f.sd = ns.sd, t.f.clip = ns.clip;
  const int M2 = h->desc.net[0].layer[h->desc.net[0].n_layers - 1].out64;
  const size_t lds = (front_floats(h->desc.stride) + (size_t)kPolicyRows * M2) * sizeof(float);
  const dim3 grid((unsigned)(((size_t)E + kPolicyRows - 1) / kPolicyRows)), block(kPolicyThreads);
  if (norm_obs) hipLaunchKernelGGL(sac_act<true>, grid, block, lds, h->stream, t);
  else hipLaunchKernelGGL(sac_act<false>, grid, block, lds, h->stream, t);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  if (norm) FLEET_HANDLE_TRY(h, fleet_norm_end_read(norm, h->stream));
  return FLEET_OK;
}

int fleet_sac_target_dev(fleet_qtarget_handle h, fleet_qtarget_handle targets, const float* next_obs, const float* rewards,
                         const float* dones, int B, const FleetSacTargetArgs* args) {
  std::string why = check_target_args(next_obs, rewards, dones, B, args);
  if (const int rc = handle_enter("fleet_sac_target_dev", why, h, g_sac_error); rc != FLEET_OK) return rc;
  const char* entry = "fleet_sac_target_dev";
  if (!targets) return refuse(h, entry, "null target networks handle");
  if (h->record_bytes != sizeof(QTargetDesc) || !qtarget_squashed(h))
    return refuse(h, entry, "the online handle's actor is not a squashed Gaussian: fleet_sac_create makes one");
  if (targets->record_bytes != sizeof(QTargetDesc) || !qtarget_squashed(targets))
    return refuse(h, entry, "the target networks' handle is not one fleet_sac_create made");
  const QTargetDesc &on = h->desc, &tg = targets->desc;
  if (on.obs_dim != tg.obs_dim || on.act_dim != tg.act_dim || on.n_critics != tg.n_critics)
    return refuse(h, entry, "the online networks have (obs_dim, act_dim, n_critics) = (" + std::to_string(on.obs_dim) + ", " +
                                std::to_string(on.act_dim) + ", " + std::to_string(on.n_critics) + "), the target networks (" +
                                std::to_string(tg.obs_dim) + ", " + std::to_string(tg.act_dim) + ", " + std::to_string(tg.n_critics) + ")");
  if (h->device != targets->device)
    return refuse(h, entry, "the online networks lie on device " + std::to_string(h->device) + ", the target networks on device " +
                                std::to_string(targets->device));
  if (h->stream != targets->stream)
    return refuse(h, entry, "the online and the target networks are handles that do not launch on one stream: fleet_qtarget_set_stream both to one first");
  const FleetSacTargetArgs& x = *args;
  SoftTargetArgs t{};
  t.online = reinterpret_cast<const QTargetDesc*>(h->block), t.targets = reinterpret_cast<const QTargetDesc*>(targets->block);
  t.online_base = reinterpret_cast<const float*>(h->block), t.targets_base = reinterpret_cast<const float*>(targets->block);
  t.next_obs = next_obs, t.rewards = rewards, t.dones = dones, t.ent_coef = x.ent_coef;
  t.target_q = x.target_q, t.q = x.q;
  t.x.noise = x.noise, t.x.actions = x.next_actions, t.x.log_prob = x.next_log_prob;
  t.x.seed = x.seed, t.x.step = x.step, t.x.id0 = (uint32_t)x.row_offset;
  t.x.given = x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN, t.x.deterministic = 0;
  t.B = B, t.S = on.stride > tg.stride ? on.stride : tg.stride;
  t.gamma = x.gamma;
  const int M2 = on.net[0].layer[on.net[0].n_layers - 1].out64;
  const size_t lds = (front_floats(t.S) + (size_t)kPolicyRows * (M2 + on.act64 + 1)) * sizeof(float);
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  const dim3 grid((unsigned)(((size_t)B + kPolicyRows - 1) / kPolicyRows)), block(kPolicyThreads);
  hipLaunchKernelGGL(sac_target, grid, block, lds, h->stream, t);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // extern "C"
