// fleet_sactrain.hip -- SAC's whole update on the device (include/fleet_hip.h "SAC's whole update on the device"; fleet_offpolicy.h):
// stable-baselines3's SAC.train() as ONE enqueue-only call: per gradient step fleet_replay_sample_dev, the alpha launch (a learned
// coefficient), fleet_sac_target_dev, fleet_td3_critic_grad_dev, the scale launch, fleet_adam_step_dev on the critics,
// fleet_sac_actor_grad_dev, fleet_adam_step_dev on the actor and on log_ent_coef and -- iff g % target_update_interval == 0, g the index
// INSIDE the call -- offpolicy_polyak (fleet_offpolicy.hip: the kernel itself, through offpolicy_launch_polyak) on the two SAC images;
// one closing launch per call.  The handle borrows a replay buffer, the targets' handle, a gradient handle and two or three optimisers
// and owns one block.
//   sactrain_alpha   one thread: alpha = (float)exp((double)log_ent_coef[0])
//   sactrain_scale   grid (chunks), 256 threads: g[i] = g[i] * s over the critics' gradient tensors, 1024 consecutive elements of one
//                    tensor per workgroup, four per thread -- one 16-byte word where the tensor starts on one and the four lie inside
//                    it, four scalars otherwise; the chunk table is built at create from the image's shapes
//   sactrain_finish  one workgroup of 256 threads per call: the ordered float64 sums of the call's slots, the statistics block
// No atomics, no ordering between workgroups: launch boundaries only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fleet_adam.h"
#include "fleet_handle.h"
#include "fleet_mlp.h"
#include "fleet_norm.h"
#include "fleet_offpolicy.h"
#include "fleet_qtarget.h"

namespace {

// ---- sactrain_alpha --------------------------------------------------------------------------------------------------------------
// one thread: the double exponential rounded once, so that the host can restate it
__global__ __launch_bounds__(64) void sactrain_alpha(const float* __restrict__ log_ent_coef, float* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (float)exp((double)log_ent_coef[0]);
}

// ---- sactrain_scale --------------------------------------------------------------------------------------------------------------
struct ScaleArgs {
  float* g[kMlpMaxTensors];
  const SacTrainChunk* chunks;
  float s;
};

__global__ __launch_bounds__(kOffpolicyThreads) void sactrain_scale(ScaleArgs a) {
  const SacTrainChunk ch = a.chunks[blockIdx.x];
  const int t = __builtin_amdgcn_readfirstlane(ch.tensor);
  float* __restrict__ g = a.g[t];
  const uint32_t i0 = ch.start + 4u * threadIdx.x;  // (start < len <= 8192 * 512: no wrap; a multiple of four)
  if (i0 + 4u <= ch.len && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    float4* __restrict__ w = reinterpret_cast<float4*>(g + i0);
    float4 v = *w;
    v.x = v.x * a.s, v.y = v.y * a.s, v.z = v.z * a.s, v.w = v.w * a.s;
    *w = v;
    return;
  }
#pragma unroll
  for (uint32_t e = 0; e < 4; ++e)
    if (i0 + e < ch.len) g[i0 + e] = g[i0 + e] * a.s;
}

// ---- sactrain_finish -------------------------------------------------------------------------------------------------------------
struct SacFinishArgs {
  const float* slots;  // f32[G][kOffpolicySlot]
  double* out;         // the statistics block f64[FLEET_TRAIN_STATS]
  uint64_t first;
  uint32_t G, interval;
  float scale;         // (float)loss_scale
  int learned;
};

__global__ __launch_bounds__(kOffpolicyThreads) void sactrain_finish(SacFinishArgs a) {
  __shared__ double red[kOffpolicyThreads];
  const uint32_t tid = threadIdx.x, G = a.G;
  const float* __restrict__ slots = a.slots;
  double sc = 0.0, sa = 0.0, se = 0.0, sl = 0.0, sp = 0.0, sq = 0.0;
  for (uint32_t g = tid; g < G; g += kOffpolicyThreads) {
    const float* __restrict__ q = slots + (size_t)g * kOffpolicySlot;
    sc = sc + (double)q[0];
    sa = sa + (double)q[kOffpolicyActorAt];
    sl = sl + (double)q[kOffpolicyActorAt + 1];
    sp = sp + (double)q[kOffpolicyActorAt + 2];
    sq = sq + (double)q[kOffpolicyActorAt + 3];
    se = se + (double)q[kOffpolicyActorAt + 4];
  }
  const double tc = tree_total(sc, red), ta = tree_total(sa, red), te = tree_total(se, red), tl = tree_total(sl, red);
  const double tp = tree_total(sp, red), tq = tree_total(sq, red);
  if (tid == 0) {
    const float* __restrict__ last = slots + (size_t)(G - 1) * kOffpolicySlot;
    a.out[0] = (double)a.scale * tc / (double)G;
    a.out[1] = ta / (double)G;
    a.out[2] = te / (double)G;
    a.out[3] = a.learned ? tl / (double)G : (double)NAN;
    a.out[4] = (double)a.scale * (double)last[0];
    a.out[5] = (double)last[kOffpolicyActorAt];
    a.out[6] = (double)(a.first + G);
    a.out[7] = (double)sactrain_target_updates(G, a.interval);
    a.out[8] = tp / (double)G;
    a.out[9] = tq / (double)G;
    for (int k = 10; k < FLEET_TRAIN_STATS; ++k) a.out[k] = 0.0;
  }
}

thread_local std::string g_sactrain_error;  // of the last failed call without a handle

}  // namespace

struct FleetSacTrain : FleetMlpUser {  // img: the ONLINE networks'; block: the staging arrays, the alpha cell, the slots, the chunk table
  fleet_replay_handle replay = nullptr;  // borrowed, as are all below
  fleet_qtarget_handle targets = nullptr, online = nullptr;
  FleetMlpHandle* tgt = nullptr;  // the targets' image
  FleetTd3* grad = nullptr;
  fleet_adam_handle adam_actor = nullptr, adam_critic = nullptr, adam_ent = nullptr;
  int D = 0, A = 0, n_critics = 0, max_batch = 0, max_steps = 0, n_actor = 0, n_critic = 0, n_chunks = 0;
  uint64_t stage[kStageArrays] = {}, staging_bytes = 0, alpha_at = 0, slots_at = 0, chunks_at = 0;

  float* staged(int which) const { return reinterpret_cast<float*>(block + stage[which]); }
  float* alpha() const { return reinterpret_cast<float*>(block + alpha_at); }
  float* slots() const { return reinterpret_cast<float*>(block + slots_at); }
  const SacTrainChunk* chunks() const { return reinterpret_cast<const SacTrainChunk*>(block + chunks_at); }
};

namespace {

std::string check_sactrain_params(const FleetSacTrainParams* p) {
  if (!p) return "null FleetSacTrainParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetSacTrainParams)) return "FleetSacTrainParams.struct_bytes does not match this library";
  if (p->max_steps < 1 || p->max_steps > kOffpolicyMaxSteps)
    return "max_steps must be in 1.." + std::to_string(kOffpolicyMaxSteps) + ", got " + std::to_string(p->max_steps);
  return "";
}

// what fleet_sactrain_scale_dev refuses without its handle
std::string check_scale_args(float* const* grads, int count, double s) {
  if (!std::isfinite(s)) return "the scale must be finite";
  if (!grads) return "null grads";
  if (count < 1 || count > kMlpMaxTensors) return "count must be in 1.." + std::to_string(kMlpMaxTensors) + ", got " + std::to_string(count);
  for (int i = 0; i < count; ++i)
    if (!grads[i]) return "gradient tensor " + std::to_string(i) + " is null";
  return "";
}

// what fleet_sactrain_sac_dev refuses, looked at without the handle: its own checks, then those of the entries it calls, in their words
std::string check_sac_args(const FleetSacTrainArgs* x, float* const* actor_params, float* const* actor_grads, int n_actor,
                           float* const* critic_params, float* const* critic_grads, int n_critic) {
  if (!x) return "null FleetSacTrainArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetSacTrainArgs)) return "FleetSacTrainArgs.struct_bytes does not match this library";
  if (x->gradient_steps < 1) return "gradient_steps must be >= 1, got " + std::to_string(x->gradient_steps);
  if (x->batch_size < 1) return "batch_size must be >= 1, got " + std::to_string(x->batch_size);
  if (x->target_update_interval < 1) return "target_update_interval must be >= 1, got " + std::to_string(x->target_update_interval);
  if (!x->stats) return "null stats";
  if ((x->ent_coef == nullptr) == (x->log_ent_coef == nullptr)) return "give exactly one of ent_coef (a fixed alpha) and log_ent_coef (a learned one)";
  if ((x->log_ent_coef == nullptr) != (x->log_ent_coef_grad == nullptr)) return "log_ent_coef and log_ent_coef_grad must be given together or both be null";
  if (x->log_ent_coef && x->log_ent_coef == x->log_ent_coef_grad) return "parameter tensor 0 is its own gradient (the entropy coefficient optimiser's)";
  if (!std::isfinite(x->loss_scale)) return "loss_scale must be finite";
  if (std::string why = offpolicy_check_tau(x->tau); !why.empty()) return why;
  if (!std::isfinite(x->lr) || x->lr < 0.0) return "lr must be finite and >= 0";
  for (int o = 0; o < 3; ++o) {
    const char* whose = o == 0 ? " (the actor optimiser's)" : (o == 1 ? " (the critic optimiser's)" : " (the entropy coefficient optimiser's)");
    if (!std::isfinite(x->eps[o]) || x->eps[o] < 0.0) return std::string("eps must be finite and >= 0") + whose;
    if (!(x->beta1[o] >= 0.0 && x->beta1[o] < 1.0)) return std::string("beta1 must be in [0, 1)") + whose;
    if (!(x->beta2[o] >= 0.0 && x->beta2[o] < 1.0)) return std::string("beta2 must be in [0, 1)") + whose;
    if (std::isnan(x->max_grad_norm[o])) return std::string("max_grad_norm is NaN") + whose;
  }
  if (std::string why = offpolicy_check_tensors("actor", actor_params, actor_grads, n_actor); !why.empty()) return why;
  return offpolicy_check_tensors("critics", critic_params, critic_grads, n_critic);
}

int launch_scale(FleetSacTrain* h, float* const* grads, int count, float s) {
  ScaleArgs a{};
  for (int i = 0; i < count; ++i) a.g[i] = grads[i];
  a.chunks = h->chunks(), a.s = s;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->img->device));
  hipLaunchKernelGGL(sactrain_scale, dim3((unsigned)h->n_chunks), dim3(kOffpolicyThreads), 0, h->img->stream, a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

int launch_alpha(FleetSacTrain* h, const float* log_ent_coef, float* out) {
  FLEET_HANDLE_TRY(h, hipSetDevice(h->img->device));
  hipLaunchKernelGGL(sactrain_alpha, dim3(1), dim3(64), 0, h->img->stream, log_ent_coef, out);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_sactrain_create(fleet_replay_handle replay, fleet_qtarget_handle targets, fleet_td3_handle grad, fleet_adam_handle adam_actor,
                          fleet_adam_handle adam_critic, fleet_adam_handle adam_ent, const FleetSacTrainParams* p, fleet_sactrain_handle* out) {
  const char* entry = "fleet_sactrain_create";
  if (out) *out = nullptr;
  std::string why = check_sactrain_params(p);
  if (!why.empty()) {
  } else if (!out) why = "null output handle";
  else if (!replay) why = "null replay handle";
  else if (!targets) why = "null target networks handle";
  else if (!grad) why = "null gradient handle";
  else if (!adam_actor) why = "null actor optimiser handle";
  else if (!adam_critic) why = "null critic optimiser handle";
  if (!why.empty()) return handle_refuse(g_sactrain_error, entry, why, FLEET_ERR_INVALID);
  FleetMlpHandle* img = image_of(grad);
  FleetMlpHandle* tgt = mlp_borrow(targets, sizeof(QTargetDesc), "target networks", &why);
  if (!tgt) return handle_refuse(g_sactrain_error, entry, why, FLEET_ERR_INVALID);
  const ReplayBase* rb = replay_base(replay);
  const FleetReplayLayout& L = rb->L;
  const int D = (int)(L.row_bytes[FLEET_REPLAY_OBS] / L.row_bytes[FLEET_REPLAY_REWARDS]);
  const int A = (int)(L.row_bytes[FLEET_REPLAY_ACTIONS] / L.row_bytes[FLEET_REPLAY_REWARDS]);
  FleetTd3Params gp{};
  uint64_t scratch = 0;
  int32_t tile = 0;
  FleetAdamParams pa{}, pc{}, pe{};
  FleetAdamInfo ia{}, ic{}, ie{};
  const QTargetDesc* desc = static_cast<const QTargetDesc*>(img->record);
  if (img == tgt) why = "the online and the target networks are one handle: the gradient handle must lie on a second image";
  else if (img->record_bytes != sizeof(QTargetDesc)) why = "the gradient handle does not lie on a fleet_qtarget image";
  else if (!qtarget_squashed(img) || !qtarget_squashed(tgt))
    why = "the networks' actor is not a squashed Gaussian (fleet_sac_create makes one): TD3's update is fleet_offpolicy_create's";
  else if (img->device != tgt->device)
    why = "the online networks lie on device " + std::to_string(img->device) + ", the target networks on device " + std::to_string(tgt->device);
  else if (img->floats != tgt->floats || img->n_tensors != tgt->n_tensors || memcmp(img->record, tgt->record, sizeof(QTargetDesc)) != 0)
    why = "the online and the target networks differ in their records (shapes, activations, output transform or bounds)";
  else if (image_of(adam_actor) != img) why = "the actor optimiser lies on another image than the gradient handle";
  else if (image_of(adam_critic) != img) why = "the critic optimiser lies on another image than the gradient handle";
  else if (adam_ent && image_of(adam_ent) != img) why = "the entropy coefficient optimiser lies on another image than the gradient handle";
  else if (fleet_td3_describe(grad, &gp, &scratch, &tile) != FLEET_OK || fleet_adam_describe(adam_actor, &pa, &ia) != FLEET_OK ||
           fleet_adam_describe(adam_critic, &pc, &ic) != FLEET_OK || (adam_ent && fleet_adam_describe(adam_ent, &pe, &ie) != FLEET_OK))
    why = "the handles do not describe themselves";
  else if (pa.first_net != 0 || pa.n_nets != 1 || pa.n_extra != 0) why = "the actor optimiser's span must be (first_net 0, n_nets 1, no extras)";
  else if (pc.first_net != 1 || pc.n_nets != desc->n_critics || pc.n_extra != 0)
    why = "the critic optimiser's span must be (first_net 1, n_nets " + std::to_string(desc->n_critics) + ", no extras)";
  else if (adam_ent && (pe.first_net != 0 || pe.n_nets != 0 || pe.n_extra != 1 || pe.extra_len[0] != 1))
    why = "the entropy coefficient optimiser's span must be (first_net 0, n_nets 0, one extra of length 1)";
  else if (rb->device != img->device) why = "the replay buffer lies on another device than the networks";
  else if (D != desc->obs_dim) why = "the replay buffer's obs_dim is " + std::to_string(D) + ", the networks' " + std::to_string(desc->obs_dim);
  else if (A != desc->act_dim) why = "the replay buffer's act_dim is " + std::to_string(A) + ", the networks' " + std::to_string(desc->act_dim);
  if (!why.empty()) return handle_refuse(g_sactrain_error, entry, why, FLEET_ERR_INVALID);
  FleetSacTrain* h = new FleetSacTrain();
  h->replay = replay, h->targets = targets, h->online = static_cast<FleetQTarget*>(img), h->tgt = tgt, h->grad = grad;
  h->adam_actor = adam_actor, h->adam_critic = adam_critic, h->adam_ent = adam_ent;
  h->D = D, h->A = A, h->n_critics = desc->n_critics, h->max_batch = gp.max_batch, h->max_steps = p->max_steps;
  h->n_actor = ia.n_tensors, h->n_critic = ic.n_tensors;
  // the scale launch's table: the critics' tensors in the order of the pointers (W, b per layer, critic after critic)
  std::vector<SacTrainChunk> chunks;
  int t = 0;
  for (int nt = 1; nt < 1 + desc->n_critics; ++nt)
    for (int l = 0; l < img->nets[nt].n_layers; ++l) {
      const PolicyLayer& Y = img->nets[nt].layer[l];
      const uint32_t lens[2] = {(uint32_t)Y.out * (uint32_t)Y.in, (uint32_t)Y.out};
      for (int k = 0; k < 2; ++k, ++t)
        for (uint32_t s = 0; s < lens[k]; s += kSacTrainChunk) chunks.push_back(SacTrainChunk{t, s, lens[k], 0});
    }
  h->n_chunks = (int)chunks.size();
  const uint64_t mb = (uint64_t)gp.max_batch;
  const uint64_t bytes[kStageArrays] = {mb * D * 4, mb * A * 4, mb * D * 4, mb * 4, mb * 4, mb * 4};
  uint64_t off = 0;
  for (int i = 0; i < kStageArrays; ++i) h->stage[i] = off, off = (off + bytes[i] + 255) / 256 * 256;
  h->staging_bytes = off;
  h->alpha_at = off, off += 256;
  h->slots_at = off, off += (uint64_t)p->max_steps * kOffpolicySlot * sizeof(float);
  off = (off + 255) / 256 * 256;
  h->chunks_at = off, off += chunks.size() * sizeof(SacTrainChunk);
  int rc = t == h->n_critic ? mlp_user_open(h, img, off, "staging block", {}, "", &why) : FLEET_ERR_INVALID;
  if (t != h->n_critic) why = "the critic optimiser's tensors are not the image's critics'";
  if (rc == FLEET_OK && (hipMemset(h->block, 0, off) != hipSuccess ||
                         hipMemcpy(h->block + h->chunks_at, chunks.data(), chunks.size() * sizeof(SacTrainChunk), hipMemcpyHostToDevice) != hipSuccess ||
                         hipDeviceSynchronize() != hipSuccess)) {
    (void)hipGetLastError();
    why = "clearing the staging block failed", rc = FLEET_ERR_HIP;
  }
  if (rc != FLEET_OK) {
    fleet_sactrain_destroy(h);
    return handle_refuse(g_sactrain_error, entry, why, rc);
  }
  *out = h;
  return FLEET_OK;
}

int fleet_sactrain_destroy(fleet_sactrain_handle h) {
  if (!h) return FLEET_OK;
  mlp_user_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_sactrain_last_error(fleet_sactrain_handle h) { return h ? h->error.c_str() : g_sactrain_error.c_str(); }

int fleet_sactrain_describe(fleet_sactrain_handle h, FleetSacTrainInfo* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  out->obs_dim = h->D, out->act_dim = h->A, out->n_critics = h->n_critics;
  out->max_batch = h->max_batch, out->max_steps = h->max_steps;
  out->n_actor_tensors = h->n_actor, out->n_critic_tensors = h->n_critic;
  out->learned_alpha = h->adam_ent ? 1 : 0;
  out->scale_chunks = h->n_chunks;
  out->reserved = 0;
  out->staging_bytes = h->staging_bytes;
  out->staging = h->block;
  out->alpha = h->alpha();
  out->slots = h->slots();
  return FLEET_OK;
}

int fleet_sactrain_alpha_dev(fleet_sactrain_handle h, const float* log_ent_coef, float* out) {
  const std::string why = log_ent_coef ? "" : "null log_ent_coef";
  if (const int rc = handle_enter("fleet_sactrain_alpha_dev", why, h, g_sactrain_error); rc != FLEET_OK) return rc;
  return launch_alpha(h, log_ent_coef, out ? out : h->alpha());
}

int fleet_sactrain_scale_dev(fleet_sactrain_handle h, float* const* grads, int count, double s) {
  std::string why = check_scale_args(grads, count, s);
  if (h && why.empty() && count != h->n_critic)
    why = "expected " + std::to_string(h->n_critic) + " tensors (W, b per layer, critic after critic), got " + std::to_string(count);
  if (const int rc = handle_enter("fleet_sactrain_scale_dev", why, h, g_sactrain_error); rc != FLEET_OK) return rc;
  return launch_scale(h, grads, count, (float)s);
}

int fleet_sactrain_polyak_dev(fleet_sactrain_handle h, double tau) {
  std::string why = offpolicy_check_tau(tau);
  if (h && why.empty() && h->tgt->stream != h->img->stream)
    why = "the target networks launch on another stream than the online networks: fleet_qtarget_set_stream both to one first";
  if (const int rc = handle_enter("fleet_sactrain_polyak_dev", why, h, g_sactrain_error); rc != FLEET_OK) return rc;
  return offpolicy_launch_polyak(h, h->tgt, h->img, tau);
}

int fleet_sactrain_sac_dev(fleet_sactrain_handle h, const FleetSacTrainArgs* x, float* const* actor_params, float* const* actor_grads,
                           int n_actor, float* const* critic_params, float* const* critic_grads, int n_critic) {
  const char* entry = "fleet_sactrain_sac_dev";
  std::string why = check_sac_args(x, actor_params, actor_grads, n_actor, critic_params, critic_grads, n_critic);
  int refusal = FLEET_ERR_INVALID;
  if (h && why.empty()) {
    const ReplayBase* rb = replay_base(h->replay);
    int32_t pos = 0, full = 0;
    (void)fleet_replay_size(h->replay, &pos, &full, nullptr, nullptr);
    if (x->gradient_steps > h->max_steps)
      why = "gradient_steps must be at most max_steps = " + std::to_string(h->max_steps) + ", got " + std::to_string(x->gradient_steps);
    else if (x->batch_size > h->max_batch)
      why = "batch_size: B must be at most max_batch = " + std::to_string(h->max_batch) + ", got " + std::to_string(x->batch_size);
    else if (n_actor != h->n_actor)
      why = "expected " + std::to_string(h->n_actor) + " tensors (W, b per layer of the actor), got " + std::to_string(n_actor);
    else if (n_critic != h->n_critic)
      why = "expected " + std::to_string(h->n_critic) + " tensors (W, b per layer, critic after critic), got " + std::to_string(n_critic);
    else if ((x->log_ent_coef != nullptr) != (h->adam_ent != nullptr))
      why = h->adam_ent ? "the handle has an entropy coefficient optimiser: give log_ent_coef, not ent_coef"
                        : "the handle has no entropy coefficient optimiser: give ent_coef, not log_ent_coef";
    else if (rb->stream != h->img->stream || h->tgt->stream != h->img->stream)
      why = "the replay buffer, the target networks and the online networks do not launch on one stream: *_set_stream them to one first";
    else if (!full && pos == 0) why = "the buffer is empty", refusal = FLEET_ERR_STATE;
    else if (x->norm) {
      FleetNormView v{};
      FLEET_HANDLE_TRY(h, hipSetDevice(rb->device));
      FLEET_HANDLE_TRY(h, fleet_norm_begin_read(x->norm, rb->stream, &v));  // (what the first sample would do: it orders, it launches nothing)
      if (v.D != h->D || v.device != rb->device)
        why = "the normaliser has obs_dim " + std::to_string(v.D) + " on device " + std::to_string(v.device) + ", the buffer " +
              std::to_string(h->D) + " on device " + std::to_string(rb->device);
    }
  }
  if (const int rc = handle_enter(entry, why, h, g_sactrain_error); rc != FLEET_OK) return refusal;
  const int B = x->batch_size, G = x->gradient_steps;
  const bool learned = x->log_ent_coef != nullptr;
  const float* alpha = learned ? h->alpha() : x->ent_coef;
  const float s32 = (float)x->loss_scale;
  FleetSacTargetArgs q{};
  q.struct_bytes = (int32_t)sizeof q;
  q.noise_mode = FLEET_EXPLORE_NOISE_DRAW, q.seed = x->target_seed, q.row_offset = 0;
  q.gamma = x->gamma, q.ent_coef = alpha, q.target_q = h->staged(kStageTargetQ);
  FleetTd3CriticArgs c{};
  c.struct_bytes = (int32_t)sizeof c, c.B = B;
  c.obs = h->staged(kStageObs), c.actions = h->staged(kStageAct), c.target_q = h->staged(kStageTargetQ);
  FleetSacActorArgs a{};
  a.struct_bytes = (int32_t)sizeof a, a.B = B;
  a.noise_mode = FLEET_EXPLORE_NOISE_DRAW, a.row_offset = 0, a.seed = x->seed;
  a.obs = h->staged(kStageObs), a.ent_coef = alpha;
  a.log_ent_coef = x->log_ent_coef, a.log_ent_coef_grad = x->log_ent_coef_grad, a.target_entropy = x->target_entropy;
  FleetAdamStepArgs s[3] = {};
  for (int o = 0; o < 3; ++o) {
    s[o].struct_bytes = (int32_t)sizeof s[o];
    s[o].lr = x->lr, s[o].beta1 = x->beta1[o], s[o].beta2 = x->beta2[o], s[o].eps = x->eps[o], s[o].max_grad_norm = x->max_grad_norm[o];
  }
  float* const ent_param[1] = {x->log_ent_coef};
  float* const ent_grad[1] = {x->log_ent_coef_grad};
  const auto failed = [&](int rc, const char* said) {
    h->error = std::string(entry) + ": " + said;
    return rc;
  };
  for (int g = 0; g < G; ++g) {
    const uint64_t u = x->first_update + (uint64_t)g;
    float* slot = h->slots() + (size_t)g * kOffpolicySlot;
    if (const int rc = fleet_replay_sample_dev(h->replay, B, x->norm, h->staged(kStageObs), h->staged(kStageAct), h->staged(kStageNext),
                                               h->staged(kStageDones), h->staged(kStageRewards), nullptr, nullptr);
        rc != FLEET_OK)
      return failed(rc, fleet_replay_last_error(h->replay));
    if (learned)
      if (const int rc = launch_alpha(h, x->log_ent_coef, h->alpha()); rc != FLEET_OK) return rc;
    q.step = u;
    if (const int rc = fleet_sac_target_dev(h->online, h->targets, h->staged(kStageNext), h->staged(kStageRewards), h->staged(kStageDones), B, &q);
        rc != FLEET_OK)
      return failed(rc, fleet_sac_last_error(h->online));
    c.stats = slot;
    if (const int rc = fleet_td3_critic_grad_dev(h->grad, &c, critic_grads, n_critic); rc != FLEET_OK)
      return failed(rc, fleet_td3_last_error(h->grad));
    if (s32 != 1.0f)
      if (const int rc = launch_scale(h, critic_grads, n_critic, s32); rc != FLEET_OK) return rc;
    if (const int rc = fleet_adam_step_dev(h->adam_critic, &s[1], critic_params, critic_grads, n_critic); rc != FLEET_OK)
      return failed(rc, fleet_adam_last_error(h->adam_critic));
    a.step = u, a.stats = slot + kOffpolicyActorAt;
    if (const int rc = fleet_sac_actor_grad_dev(h->grad, &a, actor_grads, n_actor); rc != FLEET_OK)
      return failed(rc, fleet_td3_last_error(h->grad));
    if (const int rc = fleet_adam_step_dev(h->adam_actor, &s[0], actor_params, actor_grads, n_actor); rc != FLEET_OK)
      return failed(rc, fleet_adam_last_error(h->adam_actor));
    if (learned)
      if (const int rc = fleet_adam_step_dev(h->adam_ent, &s[2], ent_param, ent_grad, 1); rc != FLEET_OK)
        return failed(rc, fleet_adam_last_error(h->adam_ent));
    if (g % x->target_update_interval == 0)
      if (const int rc = offpolicy_launch_polyak(h, h->tgt, h->img, x->tau); rc != FLEET_OK) return rc;
  }
  SacFinishArgs f{};
  f.slots = h->slots(), f.out = x->stats, f.first = x->first_update, f.G = (uint32_t)G, f.interval = (uint32_t)x->target_update_interval;
  f.scale = s32, f.learned = learned ? 1 : 0;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->img->device));
  hipLaunchKernelGGL(sactrain_finish, dim3(1), dim3(kOffpolicyThreads), 0, h->img->stream, f);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // extern "C"
