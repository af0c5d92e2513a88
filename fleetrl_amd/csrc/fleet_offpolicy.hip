// fleet_offpolicy.hip -- stable-baselines3's TD3.train() / DDPG's as ONE enqueue-only call (include/fleet_hip.h "TD3 / DDPG's whole
// update on the device"; fleet_offpolicy.h): per gradient step fleet_replay_sample_dev, fleet_qtarget_target_dev on the targets,
// fleet_td3_critic_grad_dev and fleet_adam_step_dev on the online networks and -- on every policy_delay-th update --
// fleet_td3_actor_grad_dev, fleet_adam_step_dev and the image-to-image Polyak update, all through their own entries, as they are, on
// one stream; one closing launch per call.  The handle borrows a replay buffer, the targets' handle, a gradient handle and two
// optimisers and owns one block: the staging arrays of max_batch rows and max_steps slots of per-step statistics.
//   offpolicy_polyak  grid (min(ceil(words / 256), 2048)), 256 threads.  The targets' image <- the online image over every float behind
//              the two records, t' = fmaf(tau, p, t * omt): the images have one layout, so this is one contiguous stream, one
//              16-byte word per thread and pass (a scalar head and tail where the stream does not start or end on a word; every
//              layout fleet_mlp.hip makes starts and ends on one).  It WALKS the zero padding, which stays +0.
//   offpolicy_finish  one workgroup of 256 threads per call: the ordered float64 sums of the call's slots, the means, the statistics block.
// No LDS in the first, no atomics, no ordering between workgroups: launch boundaries only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "fleet_adam.h"
#include "fleet_handle.h"
#include "fleet_mlp.h"
#include "fleet_norm.h"
#include "fleet_offpolicy.h"
#include "fleet_qtarget.h"

namespace {

// ---- offpolicy_polyak ------------------------------------------------------------------------------------------------------------
struct PolyakArgs {
  float* t;        // the targets' image behind its record
  const float* p;  // the online image behind its record
  uint32_t head, words, tail;  // floats in front of the first 16-byte word, words, floats behind the last
  float tau, omt;
};

__device__ __forceinline__ float polyak1(float tau, float p, float t, float omt) { return fmaf(tau, p, t * omt); }

__global__ __launch_bounds__(kOffpolicyThreads) void offpolicy_polyak(PolyakArgs a) {
  const uint32_t gid = blockIdx.x * kOffpolicyThreads + threadIdx.x, stride = gridDim.x * kOffpolicyThreads;
  float4* __restrict__ t4 = reinterpret_cast<float4*>(a.t + a.head);
  const float4* __restrict__ p4 = reinterpret_cast<const float4*>(a.p + a.head);
  for (uint32_t i = gid; i < a.words; i += stride) {  // (words < 2^30, stride <= 2^19: no wrap)
    const float4 p = p4[i];
    float4 t = t4[i];
    t.x = polyak1(a.tau, p.x, t.x, a.omt);
    t.y = polyak1(a.tau, p.y, t.y, a.omt);
    t.z = polyak1(a.tau, p.z, t.z, a.omt);
    t.w = polyak1(a.tau, p.w, t.w, a.omt);
    t4[i] = t;
  }
  for (uint32_t i = gid; i < a.head; i += stride) a.t[i] = polyak1(a.tau, a.p[i], a.t[i], a.omt);
  if (gid < a.tail) {  // (fewer than four)
    const size_t i = (size_t)a.head + 4 * (size_t)a.words + gid;
    a.t[i] = polyak1(a.tau, a.p[i], a.t[i], a.omt);
  }
}

// ---- offpolicy_finish ------------------------------------------------------------------------------------------------------------
struct FinishArgs {
  const float* slots;  // f32[G][kOffpolicySlot]
  double* out;         // the statistics block f64[FLEET_TRAIN_STATS]
  uint64_t first;
  uint32_t G, delay;
};

__global__ __launch_bounds__(kOffpolicyThreads) void offpolicy_finish(FinishArgs a) {
  __shared__ double red[kOffpolicyThreads];
  const uint32_t tid = threadIdx.x, G = a.G;
  const float* __restrict__ slots = a.slots;
  uint32_t g0 = 0;
  const uint32_t n = offpolicy_actor_steps(a.first, G, a.delay, &g0);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, sa = 0.0;
  for (uint32_t g = tid; g < G; g += kOffpolicyThreads) {
    const float* __restrict__ q = slots + (size_t)g * kOffpolicySlot;
    s0 = s0 + (double)q[0];
    s1 = s1 + (double)q[1];
    s2 = s2 + (double)q[2];
  }
  for (uint32_t j = tid; j < n; j += kOffpolicyThreads)  // position j of the sum: the j-th actor step, slot g0 + j * delay < G
    sa = sa + (double)slots[((size_t)g0 + (size_t)j * a.delay) * kOffpolicySlot + kOffpolicyActorAt];
  const double t0 = tree_total(s0, red), t1 = tree_total(s1, red), t2 = tree_total(s2, red), ta = tree_total(sa, red);
  if (tid == 0) {
    a.out[0] = t0 / (double)G;
    a.out[1] = t1 / (double)G;
    a.out[2] = t2 / (double)G;
    a.out[3] = n ? ta / (double)n : (double)NAN;
    a.out[4] = (double)slots[(size_t)(G - 1) * kOffpolicySlot];
    a.out[5] = n ? (double)slots[((size_t)g0 + (size_t)(n - 1) * a.delay) * kOffpolicySlot + kOffpolicyActorAt] : (double)NAN;
    a.out[6] = (double)(a.first + G);
    a.out[7] = (double)n;
    for (int k = 8; k < FLEET_TRAIN_STATS; ++k) a.out[k] = 0.0;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_offpolicy_error;  // of the last failed call without a handle

std::string check_params(const FleetOffpolicyParams* p) {
  if (!p) return "null FleetOffpolicyParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetOffpolicyParams)) return "FleetOffpolicyParams.struct_bytes does not match this library";
  if (p->max_steps < 1 || p->max_steps > kOffpolicyMaxSteps)
    return "max_steps must be in 1.." + std::to_string(kOffpolicyMaxSteps) + ", got " + std::to_string(p->max_steps);
  return "";
}

// what fleet_offpolicy_td3_dev refuses, looked at without the handle: its own checks, then fleet_qtarget_target_dev's,
// fleet_qtarget_polyak_dev's and fleet_adam_step_dev's in their words; "" when the arguments pass
std::string check_td3_args(const FleetOffpolicyArgs* x, float* const* actor_params, float* const* actor_grads, int n_actor,
                           float* const* critic_params, float* const* critic_grads, int n_critic) {
  if (!x) return "null FleetOffpolicyArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetOffpolicyArgs)) return "FleetOffpolicyArgs.struct_bytes does not match this library";
  if (x->gradient_steps < 1) return "gradient_steps must be >= 1, got " + std::to_string(x->gradient_steps);
  if (x->batch_size < 1) return "batch_size must be >= 1, got " + std::to_string(x->batch_size);
  if (x->policy_delay < 1) return "policy_delay must be >= 1, got " + std::to_string(x->policy_delay);
  if (x->reserved != 0) return "reserved must be 0";
  if (!x->stats) return "null stats";
  if (!x->sigma) return "null sigma";
  if (!(x->act_lo <= x->act_hi)) return "the bounds need act_lo <= act_hi";
  if (!(x->noise_clip >= 0.0f)) return "noise_clip must be >= 0";
  if (std::string why = offpolicy_check_tau(x->tau); !why.empty()) return why;
  if (!std::isfinite(x->lr) || x->lr < 0.0) return "lr must be finite and >= 0";
  for (int o = 0; o < 2; ++o) {
    const char* whose = o ? " (the critic optimiser's)" : " (the actor optimiser's)";
    if (!std::isfinite(x->eps[o]) || x->eps[o] < 0.0) return std::string("eps must be finite and >= 0") + whose;
    if (!(x->beta1[o] >= 0.0 && x->beta1[o] < 1.0)) return std::string("beta1 must be in [0, 1)") + whose;
    if (!(x->beta2[o] >= 0.0 && x->beta2[o] < 1.0)) return std::string("beta2 must be in [0, 1)") + whose;
    if (std::isnan(x->max_grad_norm[o])) return std::string("max_grad_norm is NaN") + whose;
  }
  if (std::string why = offpolicy_check_tensors("actor", actor_params, actor_grads, n_actor); !why.empty()) return why;
  return offpolicy_check_tensors("critics", critic_params, critic_grads, n_critic);
}

// floats of an image's record, rounded up as fleet_mlp.hip lays the first layer behind it
size_t record_floats(const FleetMlpHandle* img) { return (size_t)mlp_round_up((int)img->record_bytes, 256) / 4; }

}  // namespace

struct FleetOffpolicy : FleetMlpUser {  // img: the ONLINE networks'; block: the staging arrays, then the slots
  fleet_replay_handle replay = nullptr;  // borrowed, as are the five below
  fleet_qtarget_handle targets = nullptr;
  FleetMlpHandle* tgt = nullptr;  // the targets' image
  FleetTd3* grad = nullptr;
  fleet_adam_handle adam_actor = nullptr, adam_critic = nullptr;
  int D = 0, A = 0, n_critics = 0, max_batch = 0, max_steps = 0, n_actor = 0, n_critic = 0;
  uint64_t stage[kStageArrays] = {}, staging_bytes = 0;

  float* staged(int which) const { return reinterpret_cast<float*>(block + stage[which]); }
  float* slots() const { return reinterpret_cast<float*>(block + staging_bytes); }
};

// the one launch of the image-to-image update `tgt` <- `img`, on the targets' stream (the caller has seen that the online image launches
// there too); h: the handle whose error a failure goes to.  fleet_sactrain.hip launches it on the two SAC images (fleet_offpolicy.h).
int offpolicy_launch_polyak(FleetMlpUser* h, FleetMlpHandle* tgt, const FleetMlpHandle* img, double tau) {
  const size_t off = record_floats(tgt), n = tgt->floats - off;  // (create has seen that both images have these)
  PolyakArgs a{};
  a.t = reinterpret_cast<float*>(tgt->block) + off;
  a.p = reinterpret_cast<const float*>(img->block) + off;
  // 16-byte words where both streams reach a word's start together (hipMalloc'ed blocks and fleet_mlp.hip's layout: at once, head 0);
  // otherwise every float goes through the scalar head
  const uintptr_t mt = reinterpret_cast<uintptr_t>(a.t) & 15, mp = reinterpret_cast<uintptr_t>(a.p) & 15;
  size_t head = mt == mp ? ((16 - mt) & 15) / 4 : n;
  if (head > n) head = n;
  a.head = (uint32_t)head, a.words = (uint32_t)((n - head) / 4), a.tail = (uint32_t)((n - head) % 4);
  a.tau = (float)tau, a.omt = (float)(1.0 - tau);
  FLEET_HANDLE_TRY(h, hipSetDevice(tgt->device));
  const size_t most = a.words > a.head ? a.words : a.head;
  hipLaunchKernelGGL(offpolicy_polyak, dim3(grid_for(most, kOffpolicyThreads, kOffpolicyMaxBlocks)), dim3(kOffpolicyThreads), 0,
                     tgt->stream, a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

extern "C" {

int fleet_offpolicy_create(fleet_replay_handle replay, fleet_qtarget_handle targets, struct FleetTd3* grad, struct FleetAdam* adam_actor,
                           struct FleetAdam* adam_critic, const FleetOffpolicyParams* p, fleet_offpolicy_handle* out) {
  if (out) *out = nullptr;
  std::string why = check_params(p);
  if (!why.empty()) {
  } else if (!out) why = "null output handle";
  else if (!replay) why = "null replay handle";
  else if (!targets) why = "null target networks handle";
  else if (!grad) why = "null gradient handle";
  else if (!adam_actor) why = "null actor optimiser handle";
  else if (!adam_critic) why = "null critic optimiser handle";
  if (!why.empty()) return handle_refuse(g_offpolicy_error, "fleet_offpolicy_create", why, FLEET_ERR_INVALID);
  FleetMlpHandle* img = image_of(grad);
  FleetMlpHandle* tgt = mlp_borrow(targets, sizeof(QTargetDesc), "target networks", &why);
  if (!tgt) return handle_refuse(g_offpolicy_error, "fleet_offpolicy_create", why, FLEET_ERR_INVALID);
  const ReplayBase* rb = replay_base(replay);
  const FleetReplayLayout& L = rb->L;
  const int D = (int)(L.row_bytes[FLEET_REPLAY_OBS] / L.row_bytes[FLEET_REPLAY_REWARDS]);
  const int A = (int)(L.row_bytes[FLEET_REPLAY_ACTIONS] / L.row_bytes[FLEET_REPLAY_REWARDS]);
  FleetTd3Params gp{};
  uint64_t scratch = 0;
  int32_t tile = 0;
  FleetAdamParams pa{}, pc{};
  FleetAdamInfo ia{}, ic{};
  const QTargetDesc* desc = static_cast<const QTargetDesc*>(img->record);
  if (img == tgt) why = "the online and the target networks are one handle: the gradient handle must lie on a second image";
  else if (img->record_bytes != sizeof(QTargetDesc)) why = "the gradient handle does not lie on a fleet_qtarget image";
  else if (qtarget_squashed(img) || qtarget_squashed(tgt))
    why = "the networks' actor is a squashed Gaussian (fleet_sac_create): TD3's update does not train it";
  else if (img->device != tgt->device)
    why = "the online networks lie on device " + std::to_string(img->device) + ", the target networks on device " + std::to_string(tgt->device);
  else if (img->floats != tgt->floats || img->n_tensors != tgt->n_tensors || memcmp(img->record, tgt->record, sizeof(QTargetDesc)) != 0)
    why = "the online and the target networks differ in their records (shapes, activations, output transform or bounds)";
  else if (image_of(adam_actor) != img) why = "the actor optimiser lies on another image than the gradient handle";
  else if (image_of(adam_critic) != img) why = "the critic optimiser lies on another image than the gradient handle";
  else if (fleet_td3_describe(grad, &gp, &scratch, &tile) != FLEET_OK || fleet_adam_describe(adam_actor, &pa, &ia) != FLEET_OK ||
           fleet_adam_describe(adam_critic, &pc, &ic) != FLEET_OK)
    why = "the handles do not describe themselves";
  else if (pa.first_net != 0 || pa.n_nets != 1 || pa.n_extra != 0) why = "the actor optimiser's span must be (first_net 0, n_nets 1, no extras)";
  else if (pc.first_net != 1 || pc.n_nets != desc->n_critics || pc.n_extra != 0)
    why = "the critic optimiser's span must be (first_net 1, n_nets " + std::to_string(desc->n_critics) + ", no extras)";
  else if (rb->device != img->device) why = "the replay buffer lies on another device than the networks";
  else if (D != desc->obs_dim) why = "the replay buffer's obs_dim is " + std::to_string(D) + ", the networks' " + std::to_string(desc->obs_dim);
  else if (A != desc->act_dim) why = "the replay buffer's act_dim is " + std::to_string(A) + ", the networks' " + std::to_string(desc->act_dim);
  if (!why.empty()) return handle_refuse(g_offpolicy_error, "fleet_offpolicy_create", why, FLEET_ERR_INVALID);
  FleetOffpolicy* h = new FleetOffpolicy();
  h->replay = replay, h->targets = targets, h->tgt = tgt, h->grad = grad, h->adam_actor = adam_actor, h->adam_critic = adam_critic;
  h->D = D, h->A = A, h->n_critics = desc->n_critics, h->max_batch = gp.max_batch, h->max_steps = p->max_steps;
  h->n_actor = ia.n_tensors, h->n_critic = ic.n_tensors;
  const uint64_t mb = (uint64_t)gp.max_batch;
  const uint64_t bytes[kStageArrays] = {mb * D * 4, mb * A * 4, mb * D * 4, mb * 4, mb * 4, mb * 4};
  uint64_t off = 0;
  for (int i = 0; i < kStageArrays; ++i) h->stage[i] = off, off = (off + bytes[i] + 255) / 256 * 256;
  h->staging_bytes = off;
  off += (uint64_t)p->max_steps * kOffpolicySlot * sizeof(float);
  int rc = mlp_user_open(h, img, off, "staging block", {}, "", &why);
  if (rc == FLEET_OK && (hipMemset(h->block, 0, off) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
    (void)hipGetLastError();
    why = "clearing the staging block failed", rc = FLEET_ERR_HIP;
  }
  if (rc != FLEET_OK) {
    fleet_offpolicy_destroy(h);
    return handle_refuse(g_offpolicy_error, "fleet_offpolicy_create", why, rc);
  }
  *out = h;
  return FLEET_OK;
}

int fleet_offpolicy_destroy(fleet_offpolicy_handle h) {
  if (!h) return FLEET_OK;
  mlp_user_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_offpolicy_last_error(fleet_offpolicy_handle h) { return h ? h->error.c_str() : g_offpolicy_error.c_str(); }

int fleet_offpolicy_describe(fleet_offpolicy_handle h, FleetOffpolicyInfo* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  out->obs_dim = h->D, out->act_dim = h->A, out->n_critics = h->n_critics;
  out->max_batch = h->max_batch, out->max_steps = h->max_steps;
  out->n_actor_tensors = h->n_actor, out->n_critic_tensors = h->n_critic;
  out->reserved = 0;
  out->staging_bytes = h->staging_bytes;
  out->staging = h->block;
  out->slots = h->slots();
  return FLEET_OK;
}

int fleet_offpolicy_polyak_dev(fleet_offpolicy_handle h, double tau) {
  std::string why = offpolicy_check_tau(tau);
  if (h && why.empty() && h->tgt->stream != h->img->stream)
    why = "the target networks launch on another stream than the online networks: fleet_qtarget_set_stream both to one first";
  if (const int rc = handle_enter("fleet_offpolicy_polyak_dev", why, h, g_offpolicy_error); rc != FLEET_OK) return rc;
  return offpolicy_launch_polyak(h, h->tgt, h->img, tau);
}

int fleet_offpolicy_td3_dev(fleet_offpolicy_handle h, const FleetOffpolicyArgs* x, float* const* actor_params, float* const* actor_grads,
                            int n_actor, float* const* critic_params, float* const* critic_grads, int n_critic) {
  std::string why = check_td3_args(x, actor_params, actor_grads, n_actor, critic_params, critic_grads, n_critic);
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
  if (const int rc = handle_enter("fleet_offpolicy_td3_dev", why, h, g_offpolicy_error); rc != FLEET_OK) return refusal;
  const int B = x->batch_size, G = x->gradient_steps;
  FleetQTargetArgs q{};
  q.struct_bytes = (int32_t)sizeof q;
  q.noise_mode = FLEET_EXPLORE_NOISE_DRAW, q.seed = x->seed, q.row_offset = 0;
  q.gamma = x->gamma, q.noise_clip = x->noise_clip, q.act_lo = x->act_lo, q.act_hi = x->act_hi;
  q.sigma = x->sigma, q.target_q = h->staged(kStageTargetQ);
  FleetTd3CriticArgs c{};
  c.struct_bytes = (int32_t)sizeof c, c.B = B;
  c.obs = h->staged(kStageObs), c.actions = h->staged(kStageAct), c.target_q = h->staged(kStageTargetQ);
  FleetTd3ActorArgs a{};
  a.struct_bytes = (int32_t)sizeof a, a.B = B;
  a.obs = h->staged(kStageObs);
  FleetAdamStepArgs s[2] = {};
  for (int o = 0; o < 2; ++o) {
    s[o].struct_bytes = (int32_t)sizeof s[o];
    s[o].lr = x->lr, s[o].beta1 = x->beta1[o], s[o].beta2 = x->beta2[o], s[o].eps = x->eps[o], s[o].max_grad_norm = x->max_grad_norm[o];
  }
  const auto failed = [&](int rc, const char* said) {
    h->error = std::string("fleet_offpolicy_td3_dev: ") + said;
    return rc;
  };
  for (int g = 0; g < G; ++g) {
    const uint64_t u = x->first_update + (uint64_t)g;
    float* slot = h->slots() + (size_t)g * kOffpolicySlot;
    if (const int rc = fleet_replay_sample_dev(h->replay, B, x->norm, h->staged(kStageObs), h->staged(kStageAct), h->staged(kStageNext),
                                               h->staged(kStageDones), h->staged(kStageRewards), nullptr, nullptr);
        rc != FLEET_OK)
      return failed(rc, fleet_replay_last_error(h->replay));
    q.step = u;
    if (const int rc = fleet_qtarget_target_dev(h->targets, h->staged(kStageNext), h->staged(kStageRewards), h->staged(kStageDones), B, &q);
        rc != FLEET_OK)
      return failed(rc, fleet_qtarget_last_error(h->targets));
    c.stats = slot;
    if (const int rc = fleet_td3_critic_grad_dev(h->grad, &c, critic_grads, n_critic); rc != FLEET_OK)
      return failed(rc, fleet_td3_last_error(h->grad));
    if (const int rc = fleet_adam_step_dev(h->adam_critic, &s[1], critic_params, critic_grads, n_critic); rc != FLEET_OK)
      return failed(rc, fleet_adam_last_error(h->adam_critic));
    if ((u + 1) % (uint64_t)x->policy_delay != 0) continue;
    a.stats = slot + kOffpolicyActorAt;
    if (const int rc = fleet_td3_actor_grad_dev(h->grad, &a, actor_grads, n_actor); rc != FLEET_OK)
      return failed(rc, fleet_td3_last_error(h->grad));
    if (const int rc = fleet_adam_step_dev(h->adam_actor, &s[0], actor_params, actor_grads, n_actor); rc != FLEET_OK)
      return failed(rc, fleet_adam_last_error(h->adam_actor));
    if (const int rc = offpolicy_launch_polyak(h, h->tgt, h->img, x->tau); rc != FLEET_OK) return rc;
  }
  FinishArgs f{};
  f.slots = h->slots(), f.out = x->stats, f.first = x->first_update, f.G = (uint32_t)G, f.delay = (uint32_t)x->policy_delay;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->img->device));
  hipLaunchKernelGGL(offpolicy_finish, dim3(1), dim3(kOffpolicyThreads), 0, h->img->stream, f);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // extern "C"
