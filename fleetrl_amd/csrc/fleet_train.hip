// fleet_train.hip -- stable-baselines3's PPO.train() as ONE enqueue-only call (include/fleet_hip.h "PPO's whole update on the device";
// fleet_train.h): n_epochs passes over a finished rollout buffer in freshly shuffled minibatches, each minibatch five launches on the
// policy's stream -- train_minibatch here, then fleet_ppo_grad_dev's two and fleet_adam_step_dev's two through their own entries, as
// they are -- and one closing launch per call.  The handle borrows a rollout buffer, a gradient handle and an optimiser that lie on one
// policy and owns one block: the staging arrays of max_batch rows, the gradient launches' stats and the running sums.
//   train_minibatch  grid (min(ceil(B / 4), 256)), 256 threads.  Every workgroup evaluates the shuffle at the minibatch's positions
//              (the buffer rows of the first 2048 into the LDS) and, when the advantages are normalised, forms their mean and standard
//              deviation itself: float64, lane t adds positions t, t + 256, ... in ascending order, then a halving tree over the 256
//              lane sums -- every workgroup holds the same bits with no ordering between them.  Then it strides over tiles of 4
//              rows: a wavefront moves one row, lanes along the row (16-byte words when D or A is a multiple of 4), lane 0
//              the row's scalars (the buffer's value too in the second instance, train_minibatch<true>, which
//              fleet_train_ppo_vclip_dev launches) and its normalised advantage.  Thread 0 of workgroup 0 first folds the PREVIOUS minibatch's
//              statistics into the running float64 sums (or clears them: the call's first launch).
//   train_finish     one workgroup of 256 threads per call: the last minibatch's statistics into the sums, the means,
//              explained_variance over the whole buffer and mean(exp(log_std)) with the same ordered sum, the statistics block.
//   train_indices    the shuffle on its own: one position per thread.
// No atomics, no ordering between workgroups: launch boundaries only.
// Early stopping on approx_kl (target_kl; fleet_train_ppo_kl_dev) runs GATED instances of train_minibatch and train_finish, of
// fleet_ppo.hip's ppo_rows and ppo_weights and of fleet_adam.hip's adam_norm and adam_step; the ungated ones keep their text and their
// code.  The handle's block carries a control record (TrainCtl) behind everything else.  The property that makes the device's own
// decision safe without atomics: NO launch reads a word that a workgroup of the SAME launch may write.
//   `decided`  written by the statistics workgroup of minibatch i's ppo_weights: (double)approx_kl > 1.5 * target_kl.  Read by LATER
//              launches only: minibatch i's two Adam launches (set: they return at their top, nothing is written) and every
//              workgroup of minibatch i + 1's train_minibatch (set: no gather).
//   `stopped`  read and written by thread 0 of workgroup 0 of train_minibatch alone: clear -> it folds minibatch i's statistics into
//              the running sums and bumps the counters (minibatches run; optimiser steps taken, only when `decided` is clear; epochs
//              entered; the last epoch's approx_kl sum), then stopped = decided.  Read by LATER launches: ppo_rows and ppo_weights
//              return at their top when it is set.
//   The call's first train_minibatch clears the record and does not read `decided`.  train_finish<true> (one workgroup) folds the
//   last minibatch that ran unless `stopped` says it was folded already, divides by the DEVICE's count and writes slots [9..13].
// After a stop every remaining launch of the call loads one word and returns.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <type_traits>

#include "fleet_handle.h"
#include "fleet_mlp.h"
#include "fleet_philox.h"
#include "fleet_policy.h"
#include "fleet_train.h"

namespace {

// ---- the shuffle -------------------------------------------------------------------------------------------------------------
struct PermKey {
  uint64_t seed, epoch;
  uint32_t n;
  int h;  // half the Feistel block's bits
};

// perm(n, seed, epoch, p), p < n: the header's lines
__device__ inline uint32_t train_perm(const PermKey& k, uint32_t p) {
  const uint32_t mask = (1u << k.h) - 1u;
  uint32_t x = p;
  do {
    uint32_t L = x >> k.h, R = x & mask;
#pragma unroll 1
    for (int r = 0; r < kTrainRounds; ++r) {
      uint32_t w[4];
      philox4x32_10(R, (uint32_t)r, (uint32_t)k.epoch, (uint32_t)(k.epoch >> 32), (uint32_t)k.seed, (uint32_t)(k.seed >> 32), w);
      const uint32_t t = L ^ (w[0] & mask);
      L = R, R = t;
    }
    x = (L << k.h) | R;
  } while (x >= k.n);  // (a bijection of [0, 2^(2h)) walked from a point below n returns below n)
  return x;
}

__global__ __launch_bounds__(kTrainThreads) void train_indices(PermKey k, uint32_t start, uint32_t count, int32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kTrainThreads + threadIdx.x;
  if (i < count) out[i] = (int32_t)train_perm(k, start + i);
}

// the ordered sum's tree: every thread's `v` in, the total out to every thread
__device__ inline double tree_total(double v, double* red) {
  __syncthreads();  // (the previous total has been read)
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kTrainThreads / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// ---- train_minibatch ---------------------------------------------------------------------------------------------------------
struct MiniArgs {
  const float *obs, *act, *logp, *adv, *ret;            // the buffer's arrays, [K, E, ...]
  float *o_obs, *o_act, *o_logp, *o_adv, *o_advn, *o_ret;  // the staging arrays, [max_batch, ...]
  const float* prev_stats;  // the gradient launches' stats f32[8] of the previous minibatch
  double* acc;              // the running sums f64[5]
  PermKey key;
  uint32_t E, K, start, B;
  uint32_t obs_words, act_words;  // per row: floats, or 16-byte words when *_vec
  int obs_vec, act_vec, normalise, fold;
};

struct MiniArgsVclip : MiniArgs {
  const float* val;  // the buffer's values, [K, E]
  float* o_val;      // their staging array, [max_batch]
};

// the control record of a gated call (the head comment states who reads and who writes which word)
struct TrainCtl {
  uint32_t decided, stopped;
  uint32_t minibatches, steps, epochs;  // run; optimiser steps taken; epochs entered
  uint32_t epoch_n;                     // minibatches of the last epoch entered
  double epoch_kl;                      // their approx_kl, the ordered float64 sum
};
static_assert(sizeof(TrainCtl) <= 256, "the record's place in the block");

struct MiniArgsGated : MiniArgsVclip {  // (val and o_val are not read without the value clip; fold is not read)
  TrainCtl* ctl;
  int first;             // the call's first launch: clears the record and the sums
  int prev_epoch_start;  // the previous minibatch was the first of its epoch
};

// minibatch statistics `st` (the gradient launches' f32[8]) into the running sums and the counters
__device__ inline void ctl_fold(TrainCtl* c, double* acc, const float* st, uint32_t decided, int epoch_start) {
#pragma unroll
  for (int k = 0; k < 5; ++k) acc[k] = acc[k] + (double)st[k < 3 ? k : k + 1];
  c->minibatches = c->minibatches + 1u;
  if (!decided) c->steps = c->steps + 1u;
  if (epoch_start) c->epochs = c->epochs + 1u, c->epoch_n = 0u, c->epoch_kl = 0.0;
  c->epoch_n = c->epoch_n + 1u;
  c->epoch_kl = c->epoch_kl + (double)st[4];
}

// the buffer row t * E + e of position start + b of the epoch: the shuffle gives i = e * K + t
__device__ inline uint32_t buffer_row(const MiniArgs& a, uint32_t b) {
  const uint32_t i = train_perm(a.key, a.start + b);
  const uint32_t e = i / a.K, t = i - e * a.K;
  return t * a.E + e;
}

// one row: words `lane`, lane + 64, ... of it, four loads in flight per lane before the first of them is stored; a load past the row's
// end reads the row's last word instead (a valid address: no branch around any load) and is not stored
template <typename T>
__device__ inline void move_row(const float* src, float* dst, size_t from, size_t to, uint32_t words, uint32_t lane) {
  const T* __restrict__ s = reinterpret_cast<const T*>(src) + from * words;
  T* __restrict__ d = reinterpret_cast<T*>(dst) + to * words;
  const uint32_t last = words - 1;
  for (uint32_t c0 = lane; c0 < words; c0 += 4 * 64) {
    const uint32_t c1 = c0 + 64, c2 = c0 + 128, c3 = c0 + 192;
    const T v0 = s[c0], v1 = s[c1 < last ? c1 : last], v2 = s[c2 < last ? c2 : last], v3 = s[c3 < last ? c3 : last];
    d[c0] = v0;
    if (c1 < words) d[c1] = v1;
    if (c2 < words) d[c2] = v2;
    if (c3 < words) d[c3] = v3;
  }
}

// kVclip: the instance that stages the old values too (a second instance, so that the first one stays the code it was)
// kGated: the instances of a call that may stop itself (further instances, for the same reason)
template <bool kVclip, bool kGated = false>
__global__ __launch_bounds__(kTrainThreads) void train_minibatch(
    std::conditional_t<kGated, MiniArgsGated, std::conditional_t<kVclip, MiniArgsVclip, MiniArgs>> a) {
  __shared__ double red[kTrainThreads];
  __shared__ uint32_t rows[kTrainCache];
  const uint32_t tid = threadIdx.x, B = a.B;
  if constexpr (kGated) {
    // (the previous minibatch's ppo_weights wrote `decided`; the first launch clears it and does not read it)
    const uint32_t decided = a.first ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane(a.ctl->decided);
    if (blockIdx.x == 0 && tid == 0) {
      TrainCtl* c = a.ctl;
      if (a.first) {
#pragma unroll
        for (int k = 0; k < 5; ++k) a.acc[k] = 0.0;
        c->decided = 0u, c->stopped = 0u, c->minibatches = 0u, c->steps = 0u, c->epochs = 0u, c->epoch_n = 0u, c->epoch_kl = 0.0;
      } else {
        const uint32_t stopped = c->stopped;
        if (!stopped) ctl_fold(c, a.acc, a.prev_stats, decided, a.prev_epoch_start);
        c->stopped = stopped | decided;
      }
    }
    if (decided) return;  // (uniform over the launch)
  } else if (blockIdx.x == 0 && tid == 0) {
    // [0] policy_loss [1] value_loss [2] entropy_loss [3] approx_kl [4] clip_fraction <- stats[0], [1], [2], [4], [5]
    if (!a.fold) {
#pragma unroll
      for (int k = 0; k < 5; ++k) a.acc[k] = 0.0;
    } else {
#pragma unroll
      for (int k = 0; k < 5; ++k) a.acc[k] = a.acc[k] + (double)a.prev_stats[k < 3 ? k : k + 1];
    }
  }
  for (uint32_t b = tid; b < B && b < (uint32_t)kTrainCache; b += kTrainThreads) rows[b] = buffer_row(a, b);
  __syncthreads();
  const auto row_of = [&](uint32_t b) { return b < (uint32_t)kTrainCache ? rows[b] : buffer_row(a, b); };
  float mean = 0.0f, den = 1.0f;
  const bool normalise = a.normalise && B > 1;
  if (normalise) {
    double s = 0.0;
    for (uint32_t b = tid; b < B; b += kTrainThreads) s = s + (double)a.adv[row_of(b)];
    const double mean64 = tree_total(s, red) / (double)B;
    double q = 0.0;
    for (uint32_t b = tid; b < B; b += kTrainThreads) {
      const double d = (double)a.adv[row_of(b)] - mean64;
      q = q + d * d;
    }
    const double std64 = sqrt(tree_total(q, red) / (double)(B - 1));
    mean = (float)mean64;
    den = (float)std64 + 1e-8f;
  }
  const uint32_t lane = tid & 63, w = tid >> 6;
  constexpr uint32_t kWaves = kTrainThreads / 64;
  for (uint32_t tile = blockIdx.x; tile * kTrainRows < B; tile += gridDim.x) {
    for (uint32_t r = w; r < (uint32_t)kTrainRows; r += kWaves) {
      const uint32_t b = tile * kTrainRows + r;  // (uniform over the wavefront)
      if (b >= B) break;
      const uint32_t row = __builtin_amdgcn_readfirstlane(row_of(b));
      float x = 0.0f, lp = 0.0f, rt = 0.0f, ov = 0.0f;
      if (lane == 0) {  // (issued ahead of the row's words)
        x = a.adv[row], lp = a.logp[row], rt = a.ret[row];
        if constexpr (kVclip) ov = a.val[row];
      }
      if (a.obs_vec) move_row<float4>(a.obs, a.o_obs, row, b, a.obs_words, lane);
      else move_row<float>(a.obs, a.o_obs, row, b, a.obs_words, lane);
      if (a.act_vec) move_row<float4>(a.act, a.o_act, row, b, a.act_words, lane);
      else move_row<float>(a.act, a.o_act, row, b, a.act_words, lane);
      if (lane == 0) {
        a.o_logp[b] = lp;
        a.o_ret[b] = rt;
        a.o_adv[b] = x;
        if (normalise) a.o_advn[b] = (x - mean) / den;
        if constexpr (kVclip) a.o_val[b] = ov;
      }
    }
  }
}

// ---- train_finish ------------------------------------------------------------------------------------------------------------
struct FinishArgs {
  const float *ret, *val;  // the buffer's returns and values, n = K * E floats each, time-major
  const float* log_std;
  const float* last_stats;  // the gradient launches' stats f32[8] of the last minibatch
  double* acc;
  double* out;              // the statistics block f64[FLEET_TRAIN_STATS]
  uint32_t n;
  int A;
  double count;             // minibatches of the call
};

struct FinishArgsGated : FinishArgs {  // (count is not read: the device counted)
  TrainCtl* ctl;
  int last_epoch_start;  // the call's last scheduled minibatch is the first of its epoch
};

template <bool kGated>
__global__ __launch_bounds__(kTrainThreads) void train_finish(std::conditional_t<kGated, FinishArgsGated, FinishArgs> a) {
  __shared__ double red[kTrainThreads];
  const uint32_t tid = threadIdx.x, n = a.n;
  const float* __restrict__ ret = a.ret;
  const float* __restrict__ val = a.val;
  double sy = 0.0, sd = 0.0;
  for (uint32_t i = tid; i < n; i += kTrainThreads) {
    const double y = (double)ret[i];
    sy = sy + y;
    sd = sd + (y - (double)val[i]);
  }
  const double my = tree_total(sy, red) / (double)n;
  const double md = tree_total(sd, red) / (double)n;
  double qy = 0.0, qd = 0.0;
  for (uint32_t i = tid; i < n; i += kTrainThreads) {
    const double y = (double)ret[i];
    const double d = y - (double)val[i];
    qy = qy + (y - my) * (y - my);
    qd = qd + (d - md) * (d - md);
  }
  const double vy = tree_total(qy, red) / (double)n;
  const double vd = tree_total(qd, red) / (double)n;
  double se = 0.0;
  for (int j = (int)tid; j < a.A; j += kTrainThreads) se = se + exp((double)a.log_std[j]);
  const double sdev = tree_total(se, red) / (double)a.A;
  if constexpr (kGated) {
    if (tid == 0) {
      TrainCtl* c = a.ctl;
      const uint32_t decided = c->decided;
      // stopped clear: the last scheduled minibatch ran and no train_minibatch came behind it to fold it
      if (!c->stopped) ctl_fold(c, a.acc, a.last_stats, decided, a.last_epoch_start);
      const double count = (double)c->minibatches;
#pragma unroll
      for (int k = 0; k < 5; ++k) a.out[k] = a.acc[k] / count;
      a.out[5] = (double)a.last_stats[3];  // (the gradient launches after a stop wrote nothing: the last minibatch that ran)
      a.out[6] = count;
      a.out[7] = vy == 0.0 ? (double)NAN : 1.0 - vd / vy;
      a.out[8] = sdev;
      a.out[9] = (double)c->steps;
      a.out[10] = (double)c->epochs;
      a.out[11] = decided ? 1.0 : 0.0;
      a.out[12] = (double)a.last_stats[4];
      a.out[13] = c->epoch_kl / (double)c->epoch_n;
      for (int k = 14; k < FLEET_TRAIN_STATS; ++k) a.out[k] = 0.0;
    }
  } else if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) a.out[k] = (a.acc[k] + (double)a.last_stats[k < 3 ? k : k + 1]) / a.count;
    a.out[5] = (double)a.last_stats[3];
    a.out[6] = a.count;
    a.out[7] = vy == 0.0 ? (double)NAN : 1.0 - vd / vy;
    a.out[8] = sdev;
    for (int k = 9; k < FLEET_TRAIN_STATS; ++k) a.out[k] = 0.0;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_train_error;  // of the last failed call without a handle

constexpr int kMaxCount = kMlpMaxTensors + FLEET_ADAM_MAX_EXTRA;  // what fleet_adam_step_dev takes at most

// what fleet_train_ppo_dev refuses, looked at without the handle, fleet_ppo_grad_dev's and fleet_adam_step_dev's refusals in their
// words; "" when the arguments pass
std::string check_ppo_args(const FleetTrainPpoArgs* x, float* const* params, float* const* grads, int count) {
  if (!x) return "null FleetTrainPpoArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetTrainPpoArgs)) return "FleetTrainPpoArgs.struct_bytes does not match this library";
  if (x->n_epochs < 1) return "n_epochs must be >= 1, got " + std::to_string(x->n_epochs);
  if (x->batch_size < 1) return "batch_size must be >= 1, got " + std::to_string(x->batch_size);
  if (x->reserved != 0) return "reserved must be 0";
  if (!x->stats) return "null stats";
  if (!(x->clip_range > 0.0f && x->clip_range < 1.0f)) return "clip_range must be in (0, 1)";
  if (std::isnan(x->vf_coef)) return "vf_coef is NaN";
  if (std::isnan(x->ent_coef)) return "ent_coef is NaN";
  if (!std::isfinite(x->lr) || x->lr < 0.0) return "lr must be finite and >= 0";
  if (!std::isfinite(x->eps) || x->eps < 0.0) return "eps must be finite and >= 0";
  if (!(x->beta1 >= 0.0 && x->beta1 < 1.0)) return "beta1 must be in [0, 1)";
  if (!(x->beta2 >= 0.0 && x->beta2 < 1.0)) return "beta2 must be in [0, 1)";
  if (std::isnan(x->max_grad_norm)) return "max_grad_norm is NaN";
  if (!params) return "null params";
  if (!grads) return "null grads";
  if (count < 1 || count > kMaxCount) return "count must be the policy's tensors plus one (log_std), got " + std::to_string(count);
  for (int i = 0; i < count; ++i) {
    if (!params[i]) return "parameter tensor " + std::to_string(i) + " is null";
    if (!grads[i]) return "gradient tensor " + std::to_string(i) + " is null";
    if (params[i] == grads[i]) return "parameter tensor " + std::to_string(i) + " is its own gradient";
  }
  return "";
}

std::string check_indices_args(int32_t n, int32_t start, int32_t count, const int32_t* out) {
  if (n < 1) return "n must be >= 1, got " + std::to_string(n);
  if (start < 0 || count < 0 || (int64_t)start + count > n)
    return "positions " + std::to_string(start) + " .. +" + std::to_string(count) + " lie outside [0, " + std::to_string(n) + ")";
  if (!out) return "null out";
  return "";
}

PermKey perm_key(uint32_t n, uint64_t seed, uint64_t epoch) {
  int h = kTrainMinHalfBits;
  while (((uint64_t)1 << (2 * h)) < n) ++h;  // (n < 2^31: h <= 16)
  return PermKey{seed, epoch, n, h};
}

// The handles this family is created on keep their definitions in their own files; what it needs of them is what their scaffolds
// share: a rollout buffer's first base is FleetBufferBase<FleetRolloutLayout> (fleet_handle.h), a gradient handle's and an optimiser's
// is FleetMlpUser (fleet_mlp.h), as mlp_borrow relies on the image's handle being its family's first base.
using RolloutBase = FleetBufferBase<FleetRolloutLayout>;
const RolloutBase* rollout_base(fleet_rollout_handle r) { return reinterpret_cast<const RolloutBase*>(r); }
FleetMlpHandle* image_of(void* user) { return reinterpret_cast<FleetMlpUser*>(user)->img; }

}  // namespace

enum { kStageObs, kStageAct, kStageLogp, kStageAdv, kStageAdvn, kStageRet, kStageArrays };

struct FleetTrain : FleetMlpUser {  // img: the policy's; block: the staging arrays, the gradient launches' stats, the running sums
  fleet_rollout_handle buffer = nullptr;  // borrowed, as are the two below
  fleet_ppo_handle grad = nullptr;
  fleet_adam_handle adam = nullptr;
  FleetRolloutArrays arr{};
  int E = 0, K = 0, D = 0, A = 0, max_batch = 0, n_tensors = 0;
  uint64_t stage[kStageArrays] = {}, stats_at = 0, acc_at = 0, staging_bytes = 0;
  uint64_t val_at = 0;  // the staged old values, behind everything that was there before them
  uint64_t ctl_at = 0;  // a gated call's control record (TrainCtl), behind those

  float* staged(int which) const { return reinterpret_cast<float*>(block + stage[which]); }
};

extern "C" {

int fleet_train_create(fleet_rollout_handle buffer, struct FleetPpo* grad, struct FleetAdam* adam, fleet_train_handle* out) {
  if (out) *out = nullptr;
  std::string why;
  if (!out) why = "null output handle";
  else if (!buffer) why = "null rollout handle";
  else if (!grad) why = "null gradient handle";
  else if (!adam) why = "null optimiser handle";
  if (!why.empty()) return handle_refuse(g_train_error, "fleet_train_create", why, FLEET_ERR_INVALID);
  FleetMlpHandle* img = image_of(grad);
  const RolloutBase* rb = rollout_base(buffer);
  const FleetRolloutLayout& L = rb->L;
  const int E = (int)(L.row_bytes[FLEET_ROLLOUT_REWARDS] / 4), K = (int)(L.bytes[FLEET_ROLLOUT_REWARDS] / L.row_bytes[FLEET_ROLLOUT_REWARDS]);
  const int D = (int)(L.row_bytes[FLEET_ROLLOUT_OBS] / L.row_bytes[FLEET_ROLLOUT_REWARDS]);
  const int A = (int)(L.row_bytes[FLEET_ROLLOUT_ACTIONS] / L.row_bytes[FLEET_ROLLOUT_REWARDS]);
  FleetPpoParams pp{};
  uint64_t scratch = 0;
  int32_t tile = 0;
  FleetAdamParams ap{};
  FleetAdamInfo ai{};
  if (image_of(adam) != img) why = "the gradient handle and the optimiser lie on different policies";
  else if (img->record_bytes != sizeof(PolicyDesc)) why = "the handles do not lie on a policy";
  else if (rb->device != img->device) why = "the rollout buffer lies on another device than the policy";
  else if (fleet_ppo_describe(grad, &pp, &scratch, &tile) != FLEET_OK || fleet_adam_describe(adam, &ap, &ai) != FLEET_OK)
    why = "the handles do not describe themselves";
  else {
    const PolicyHeadDesc& actor = img->nets[0];
    const int pd = actor.layer[0].in, pa = actor.layer[actor.n_layers - 1].out;
    if (D != pd) why = "the rollout buffer's obs_dim is " + std::to_string(D) + ", the policy's " + std::to_string(pd);
    else if (A != pa) why = "the rollout buffer's act_dim is " + std::to_string(A) + ", the policy's " + std::to_string(pa);
    else if (ap.first_net != 0 || ap.n_nets != 2 || ap.n_extra != 1 || ap.extra_len[0] != A)
      why = "the optimiser's span must be both heads of the policy and one extra of length " + std::to_string(A) + " (log_std)";
  }
  if (!why.empty()) return handle_refuse(g_train_error, "fleet_train_create", why, FLEET_ERR_INVALID);
  FleetTrain* h = new FleetTrain();
  h->buffer = buffer, h->grad = grad, h->adam = adam;
  h->E = E, h->K = K, h->D = D, h->A = A, h->max_batch = pp.max_batch, h->n_tensors = img->n_tensors + 1;
  fleet_rollout_arrays(buffer, &h->arr);
  const uint64_t mb = (uint64_t)pp.max_batch;
  const uint64_t bytes[kStageArrays] = {mb * D * 4, mb * A * 4, mb * 4, mb * 4, mb * 4, mb * 4};
  uint64_t off = 0;
  for (int i = 0; i < kStageArrays; ++i) h->stage[i] = off, off = (off + bytes[i] + 255) / 256 * 256;
  h->staging_bytes = off;
  h->stats_at = off, off += 256;
  h->acc_at = off, off += 256;
  h->val_at = off, off += (mb * 4 + 255) / 256 * 256;
  h->ctl_at = off, off += 256;
  int rc = mlp_user_open(h, img, off, "staging block", {}, "", &why);
  if (rc == FLEET_OK && (hipMemset(h->block, 0, off) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
    (void)hipGetLastError();
    why = "clearing the staging block failed", rc = FLEET_ERR_HIP;
  }
  if (rc != FLEET_OK) {
    fleet_train_destroy(h);
    return handle_refuse(g_train_error, "fleet_train_create", why, rc);
  }
  *out = h;
  return FLEET_OK;
}

int fleet_train_destroy(fleet_train_handle h) {
  if (!h) return FLEET_OK;
  mlp_user_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_train_last_error(fleet_train_handle h) { return h ? h->error.c_str() : g_train_error.c_str(); }

int fleet_train_describe(fleet_train_handle h, FleetTrainInfo* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  out->num_envs = h->E, out->n_steps = h->K, out->obs_dim = h->D, out->act_dim = h->A;
  out->max_batch = h->max_batch, out->n_tensors = h->n_tensors;
  out->rounds = kTrainRounds, out->min_half_bits = kTrainMinHalfBits;
  out->tile_rows = kTrainRows, out->cache_rows = kTrainCache;
  out->staging_bytes = h->staging_bytes;
  out->staging = h->block;
  return FLEET_OK;
}

int fleet_train_indices_dev(fleet_train_handle h, int32_t n, uint64_t seed, uint64_t epoch, int32_t start, int32_t count, int32_t* out) {
  const std::string why = check_indices_args(n, start, count, out);
  if (const int rc = handle_enter("fleet_train_indices_dev", why, h, g_train_error); rc != FLEET_OK) return rc;
  if (count == 0) return FLEET_OK;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->img->device));
  hipLaunchKernelGGL(train_indices, dim3(((unsigned)count + kTrainThreads - 1) / kTrainThreads), dim3(kTrainThreads), 0, h->img->stream,
                     perm_key((uint32_t)n, seed, epoch), (uint32_t)start, (uint32_t)count, out);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // extern "C"

namespace {

// every update; clip_range_vf 0: no value clip; target_kl 0: no early stop, the ungated launches (`why`: what the entry's own checks
// found)
int train_ppo(const char* entry, fleet_train_handle h, std::string why, const FleetTrainPpoArgs* x, float clip_range_vf, float* const* params,
              float* const* grads, int count, double target_kl = 0.0) {
  const uint32_t n = h ? (uint32_t)h->E * (uint32_t)h->K : 0;
  const uint32_t bs = h && why.empty() ? ((uint32_t)x->batch_size < n ? (uint32_t)x->batch_size : n) : 0;
  if (h && why.empty()) {
    if (count != h->n_tensors)
      why = "expected " + std::to_string(h->n_tensors) + " gradient tensors (W, b per layer, then log_std), got " + std::to_string(count);
    else if (bs > (uint32_t)h->max_batch)
      why = "a minibatch of " + std::to_string(bs) + " rows: B must be at most max_batch = " + std::to_string(h->max_batch) + ", got " +
            std::to_string(bs);
    else if (rollout_base(h->buffer)->stream != h->img->stream)
      why = "the rollout buffer launches on another stream than the policy: fleet_rollout_set_stream it to the policy's first";
  }
  if (const int rc = handle_enter(entry, why, h, g_train_error); rc != FLEET_OK) return rc;
  const bool vclip = clip_range_vf > 0.0f, gated = target_kl > 0.0;
  FleetMlpHandle* pol = h->img;
  TrainCtl* ctl = reinterpret_cast<TrainCtl*>(h->block + h->ctl_at);
  int64_t base_step = 0;
  if (gated) {
    FLEET_HANDLE_TRY(h, hipSetDevice(pol->device));
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    FLEET_HANDLE_TRY(h, hipStreamIsCapturing(pol->stream, &capture));
    if (capture != hipStreamCaptureStatusNone) {
      h->error = std::string(entry) + ": the policy's stream is capturing a graph; an update that may stop itself settles the optimiser's "
                 "step count through an event and cannot be captured";
      return FLEET_ERR_STATE;
    }
    FleetAdamParams ap{};
    FleetAdamInfo ai{};
    if (const int rc = fleet_adam_describe(h->adam, &ap, &ai); rc != FLEET_OK) {  // (settles what an earlier call left pending)
      h->error = std::string(entry) + ": " + fleet_adam_last_error(h->adam);
      return rc;
    }
    base_step = ai.step;
  }
  float* gstats = reinterpret_cast<float*>(h->block + h->stats_at);
  double* acc = reinterpret_cast<double*>(h->block + h->acc_at);
  MiniArgsGated m{};
  m.ctl = ctl;
  m.obs = h->arr.obs, m.act = h->arr.actions, m.logp = h->arr.log_probs, m.adv = h->arr.advantages, m.ret = h->arr.returns;
  m.o_obs = h->staged(kStageObs), m.o_act = h->staged(kStageAct), m.o_logp = h->staged(kStageLogp), m.o_adv = h->staged(kStageAdv);
  m.o_advn = h->staged(kStageAdvn), m.o_ret = h->staged(kStageRet);
  m.val = h->arr.values, m.o_val = vclip ? reinterpret_cast<float*>(h->block + h->val_at) : nullptr;
  FleetPpoGradGatedArgs gg{};  // (the gated call's; its base is filled from `g` per minibatch)
  gg.struct_bytes = (int32_t)sizeof gg, gg.clip_range_vf = vclip ? clip_range_vf : 0.0f, gg.old_values = m.o_val;
  gg.gate.skip = &ctl->stopped, gg.gate.decided = &ctl->decided, gg.gate.threshold = 1.5 * target_kl;
  m.prev_stats = gstats, m.acc = acc;
  m.E = (uint32_t)h->E, m.K = (uint32_t)h->K;
  // (the buffer's arrays and the staging arrays start at multiples of 256 bytes: a row of 4k floats starts at a multiple of 16)
  m.obs_vec = h->D % 4 == 0, m.act_vec = h->A % 4 == 0;
  m.obs_words = (uint32_t)(m.obs_vec ? h->D / 4 : h->D), m.act_words = (uint32_t)(m.act_vec ? h->A / 4 : h->A);
  m.normalise = x->normalize_advantage != 0;
  FleetPpoGradVclipArgs gv{};
  gv.struct_bytes = (int32_t)sizeof gv, gv.clip_range_vf = clip_range_vf, gv.old_values = m.o_val;
  FleetPpoGradArgs& g = gv.base;
  g.struct_bytes = (int32_t)sizeof g;
  g.obs = m.o_obs, g.actions = m.o_act, g.old_log_prob = m.o_logp, g.returns = m.o_ret, g.log_std = params[count - 1];
  g.clip_range = x->clip_range, g.vf_coef = x->vf_coef, g.ent_coef = x->ent_coef, g.stats = gstats;
  FleetAdamStepArgs s{};
  s.struct_bytes = (int32_t)sizeof s;
  s.lr = x->lr, s.beta1 = x->beta1, s.beta2 = x->beta2, s.eps = x->eps, s.max_grad_norm = x->max_grad_norm;
  FLEET_HANDLE_TRY(h, hipSetDevice(pol->device));
  uint64_t done = 0;
  bool prev_epoch_start = false;
  for (int e = 0; e < x->n_epochs; ++e) {
    m.key = perm_key(n, x->seed, x->first_epoch + (uint64_t)e);
    for (uint32_t start = 0; start < n; start += bs, ++done) {
      const uint32_t B = n - start < bs ? n - start : bs;
      m.start = start, m.B = B, m.fold = done != 0;
      const unsigned tiles = (B + kTrainRows - 1) / kTrainRows;
      const dim3 grid(tiles < (unsigned)kTrainMaxBlocks ? tiles : (unsigned)kTrainMaxBlocks);
      m.first = done == 0, m.prev_epoch_start = prev_epoch_start, prev_epoch_start = start == 0;
      if (gated && vclip) hipLaunchKernelGGL((train_minibatch<true, true>), grid, dim3(kTrainThreads), 0, pol->stream, m);
      else if (gated) hipLaunchKernelGGL((train_minibatch<false, true>), grid, dim3(kTrainThreads), 0, pol->stream, m);
      else if (vclip) hipLaunchKernelGGL(train_minibatch<true>, grid, dim3(kTrainThreads), 0, pol->stream, static_cast<const MiniArgsVclip&>(m));
      else hipLaunchKernelGGL(train_minibatch<false>, grid, dim3(kTrainThreads), 0, pol->stream, static_cast<const MiniArgs&>(m));
      FLEET_HANDLE_TRY(h, hipGetLastError());
      g.B = (int32_t)B;
      g.advantages = m.normalise && B > 1 ? m.o_advn : m.o_adv;
      if (gated) {
        gg.base = g;
        if (const int rc = fleet_ppo_grad_gated_dev(h->grad, &gg, grads, count); rc != FLEET_OK) {
          h->error = std::string(entry) + ": " + fleet_ppo_last_error(h->grad);
          return rc;
        }
        if (const int rc = fleet_adam_step_gated_dev(h->adam, &s, params, grads, count, &ctl->decided); rc != FLEET_OK) {
          h->error = std::string(entry) + ": " + fleet_adam_last_error(h->adam);
          return rc;
        }
        continue;
      }
      if (const int rc = vclip ? fleet_ppo_grad_vclip_dev(h->grad, &gv, grads, count) : fleet_ppo_grad_dev(h->grad, &g, grads, count);
          rc != FLEET_OK) {
        h->error = std::string(entry) + ": " + fleet_ppo_last_error(h->grad);
        return rc;
      }
      if (const int rc = fleet_adam_step_dev(h->adam, &s, params, grads, count); rc != FLEET_OK) {
        h->error = std::string(entry) + ": " + fleet_adam_last_error(h->adam);
        return rc;
      }
    }
  }
  FinishArgsGated f{};
  f.ctl = ctl, f.last_epoch_start = prev_epoch_start;
  f.ret = h->arr.returns, f.val = h->arr.values, f.log_std = params[count - 1], f.last_stats = gstats, f.acc = acc, f.out = x->stats;
  f.n = n, f.A = h->A, f.count = (double)done;
  if (gated) hipLaunchKernelGGL(train_finish<true>, dim3(1), dim3(kTrainThreads), 0, pol->stream, f);
  else hipLaunchKernelGGL(train_finish<false>, dim3(1), dim3(kTrainThreads), 0, pol->stream, static_cast<const FinishArgs&>(f));
  FLEET_HANDLE_TRY(h, hipGetLastError());
  if (gated) {
    // the steps that ran are the device's to say: base_step + ctl->steps, once everything enqueued here has run
    if (const int rc = fleet_adam_settle_dev(h->adam, base_step, &ctl->steps); rc != FLEET_OK) {
      h->error = std::string(entry) + ": " + fleet_adam_last_error(h->adam);
      return rc;
    }
  }
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_train_ppo_dev(fleet_train_handle h, const FleetTrainPpoArgs* x, float* const* params, float* const* grads, int count) {
  return train_ppo("fleet_train_ppo_dev", h, check_ppo_args(x, params, grads, count), x, 0.0f, params, grads, count);
}

int fleet_train_ppo_vclip_dev(fleet_train_handle h, const FleetTrainPpoVclipArgs* a, float* const* params, float* const* grads, int count) {
  std::string why;
  if (!a) why = "null FleetTrainPpoVclipArgs";
  else if (a->struct_bytes != (int32_t)sizeof(FleetTrainPpoVclipArgs)) why = "FleetTrainPpoVclipArgs.struct_bytes does not match this library";
  else why = check_ppo_args(&a->base, params, grads, count);
  if (why.empty() && !(std::isfinite(a->clip_range_vf) && a->clip_range_vf > 0.0f)) why = "clip_range_vf must be finite and > 0";
  return train_ppo("fleet_train_ppo_vclip_dev", h, why, a ? &a->base : nullptr, a ? a->clip_range_vf : 0.0f, params, grads, count);
}

int fleet_train_ppo_kl_dev(fleet_train_handle h, const FleetTrainPpoKlArgs* a, float* const* params, float* const* grads, int count) {
  std::string why;
  if (!a) why = "null FleetTrainPpoKlArgs";
  else if (a->struct_bytes != (int32_t)sizeof(FleetTrainPpoKlArgs)) why = "FleetTrainPpoKlArgs.struct_bytes does not match this library";
  else why = check_ppo_args(&a->base, params, grads, count);
  if (why.empty() && !(std::isfinite(a->target_kl) && a->target_kl > 0.0)) why = "target_kl must be finite and > 0";
  if (why.empty() && !(std::isfinite(a->clip_range_vf) && a->clip_range_vf >= 0.0f)) why = "clip_range_vf must be finite and >= 0 (0: no value clip)";
  return train_ppo("fleet_train_ppo_kl_dev", h, why, a ? &a->base : nullptr, a ? a->clip_range_vf : 0.0f, params, grads, count,
                   a ? a->target_kl : 0.0);
}

int fleet_train_describe_vclip(fleet_train_handle h, uint64_t* old_values_offset) {
  if (!h || !old_values_offset) return FLEET_ERR_INVALID;
  *old_values_offset = h->val_at;
  return FLEET_OK;
}

}  // extern "C"
