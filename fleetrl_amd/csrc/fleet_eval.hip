// fleet_eval.hip -- stable-baselines3's EvalCallback as ONE enqueue-only call (include/fleet_hip.h "evaluation of the agent on the
// device"; fleet_eval.h): the normaliser sync, the reset, per env step the deterministic forward, the env step and the normaliser step
// through their own entries, as they are, on one stream, and what nothing else keeps on the device -- evaluate_policy's episode
// quotas and lists, their mean and std, SB3's "new best" test and the copy of the best weights.  The handle borrows an env, an
// optional normaliser and a policy and owns one block: the step's buffers, the per-env bookkeeping, the lists, the scalars and the
// snapshot.  The actor may also be the squashed-Gaussian networks of fleet_sac_create (include/fleet_hip_sac_loop.h, fleet_saceval_*):
// the action is then fleet_sac_act_dev's deterministic one and the snapshot the whole image, critics included.
//   eval_episodes  ONE workgroup of 1024 threads per env step: sums and lengths move on, the envs below their quota that finished
//              take list slots in env order (ballot and popcount per wavefront, chunks of 1024 envs).  Behind one of two loaders:
//              the env's records, or the caller's arrays.
//   eval_clear     the reset's zero sums, lengths, counts and list count.
//   eval_finish    one workgroup of 256 threads per call: the ordered float64 sums over the lists, mean and std, the gate, the best.
//   eval_copy      the policy image's weights into the snapshot iff the gate is set; the snapshot into a policy (no gate).
// No atomics, no ordering between workgroups: launch boundaries only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <string>

#include "../../include/fleet_hip_sac_loop.h"
#include "fleet_batch.h"
#include "fleet_eval.h"
#include "fleet_handle.h"
#include "fleet_mlp.h"
#include "fleet_norm.h"
#include "fleet_qtarget.h"

namespace {

// ---- eval_episodes ---------------------------------------------------------------------------------------------------------------
struct EpisodeArgs {
  const uint8_t* done;    // u8[E]: the step's done flags
  const double* reward;   // f64[E]: what the stack hands SB3 for the step
  const EnvRec* env;      // reward_source 1: the env's records and ...
  const FleetCold* cold;  // ... its cold block (last_len[E]), or
  const double* ep_ret;   // the caller's arrays f64[E] and ...
  const int32_t* ep_len;  // ... i32[E]
  double* sums;           // f64[E]
  int32_t* lengths;       // i32[E]
  int32_t* counts;        // i32[E]
  double* ep_reward;      // f64[max_episodes]
  int32_t* ep_length;     // i32[max_episodes]
  uint64_t* listed;
  int E, n_eval, max_episodes;
  int round32;            // the reward is a raw one: SB3 sees it as float32
  int source;
};

template <bool kFromEnv>
__global__ __launch_bounds__(kEvalScanThreads) void eval_episodes(EpisodeArgs a) {
  __shared__ int s_wave[kEvalScanWaves];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int E = a.E;
  const uint64_t listed = *a.listed;  // (thread 0 writes it behind the last barrier)
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int e0 = 0; e0 < E; e0 += kEvalScanThreads) {
    const int e = e0 + (int)threadIdx.x;
    bool f = false;
    double ep_r = 0.0;
    int32_t ep_n = 0;
    if (e < E) {
      const double r = a.round32 ? (double)(float)a.reward[e] : a.reward[e];
      const double s = a.sums[e] + r;
      const int32_t n = a.lengths[e] + 1;
      const int32_t cnt = a.counts[e];
      const int32_t target = (int32_t)(((int64_t)a.n_eval + e) / E);
      f = cnt < target && a.done[e] != 0;
      if (f) {
        if (a.source) {
          ep_r = kFromEnv ? a.env[e].last_ep_return : a.ep_ret[e];
          ep_n = kFromEnv ? a.cold->last_len[e] : a.ep_len[e];
        } else {
          ep_r = s, ep_n = n;
        }
        a.counts[e] = cnt + 1;
      }
      a.sums[e] = f ? 0.0 : s;
      a.lengths[e] = f ? 0 : n;
    }
    const unsigned long long m = __ballot(f);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (f) {
      const uint64_t slot = listed + (uint64_t)(off + before);
      if (slot < (uint64_t)a.max_episodes) {
        a.ep_reward[slot] = ep_r;
        a.ep_length[slot] = ep_n;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int w = 0; w < kEvalScanWaves; ++w) tot += s_wave[w];
      s_base += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *a.listed = listed + (uint64_t)s_base;
}

// ---- eval_clear ------------------------------------------------------------------------------------------------------------------
__global__ void eval_clear(double* __restrict__ sums, int32_t* __restrict__ lengths, int32_t* __restrict__ counts, uint64_t* __restrict__ listed,
                           int E) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < E) sums[i] = 0.0, lengths[i] = 0, counts[i] = 0;
  if (i == 0) *listed = 0;
}

// ---- eval_finish -----------------------------------------------------------------------------------------------------------------
struct FinishArgs {
  const double* ep_reward;
  const int32_t* ep_length;
  const uint64_t* listed;
  double* best;
  uint64_t* evals;
  uint32_t* gate;
  double* out;  // the statistics block f64[FLEET_EVAL_STATS]
  uint64_t num_timesteps;
  uint32_t max_episodes;
};

// the ordered sum's tree: every thread's `v` in, the total out to every thread
__device__ inline double tree_total(double v, double* red) {
  __syncthreads();  // (the previous total has been read)
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kEvalThreads / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kEvalThreads) void eval_finish(FinishArgs a) {
  __shared__ double red[kEvalThreads];
  const uint32_t tid = threadIdx.x;
  const uint64_t listed = *a.listed;
  const uint32_t n = listed < (uint64_t)a.max_episodes ? (uint32_t)listed : a.max_episodes;
  double sr = 0.0, sl = 0.0;
  for (uint32_t s = tid; s < n; s += kEvalThreads) {
    sr = sr + a.ep_reward[s];
    sl = sl + (double)a.ep_length[s];
  }
  const double mr = tree_total(sr, red) / (double)n, ml = tree_total(sl, red) / (double)n;  // (n == 0: not used)
  double vr = 0.0, vl = 0.0;
  for (uint32_t s = tid; s < n; s += kEvalThreads) {
    const double dr = a.ep_reward[s] - mr, dl = (double)a.ep_length[s] - ml;
    vr = vr + dr * dr;
    vl = vl + dl * dl;
  }
  const double tr = tree_total(vr, red), tl = tree_total(vl, red);
  if (tid == 0) {
    const double mean = n ? mr : (double)NAN;
    const double best = *a.best;
    const bool better = mean > best;  // (SB3's test: false for NaN)
    const uint64_t evals = *a.evals + 1;
    a.out[0] = mean;
    a.out[1] = n ? sqrt(tr / (double)n) : (double)NAN;
    a.out[2] = n ? ml : (double)NAN;
    a.out[3] = n ? sqrt(tl / (double)n) : (double)NAN;
    a.out[4] = (double)n;
    a.out[5] = better ? mean : best;
    a.out[6] = better ? 1.0 : 0.0;
    a.out[7] = (double)a.num_timesteps;
    a.out[8] = (double)evals;
    for (int k = 9; k < kEvalStats; ++k) a.out[k] = 0.0;
    if (better) *a.best = mean;
    *a.evals = evals;
    *a.gate = better ? 1u : 0u;
  }
}

// ---- eval_copy -------------------------------------------------------------------------------------------------------------------
// n4 float4 from src to dst; with a gate, only when its word is set (uniform over the grid: every thread reads the same word)
__global__ __launch_bounds__(256) void eval_copy(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4, const uint32_t* gate) {
  if (gate && *gate == 0) return;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) dst[i] = src[i];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_eval_error;  // of the last failed call without a handle

std::string check_params(const FleetEvalParams* p) {
  if (!p) return "null FleetEvalParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetEvalParams)) return "FleetEvalParams.struct_bytes does not match this library";
  if (p->max_episodes < 1 || p->max_episodes > kEvalMaxEpisodes)
    return "max_episodes must be in 1.." + std::to_string(kEvalMaxEpisodes) + ", got " + std::to_string(p->max_episodes);
  return "";
}

// what fleet_eval_run_dev refuses, looked at without the handle; "" when the arguments pass
std::string check_run_args(const FleetEvalArgs* x) {
  if (!x) return "null FleetEvalArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetEvalArgs)) return "FleetEvalArgs.struct_bytes does not match this library";
  if (x->n_eval_episodes < 1) return "n_eval_episodes must be >= 1, got " + std::to_string(x->n_eval_episodes);
  if (x->n_steps < 1) return "n_steps must be >= 1, got " + std::to_string(x->n_steps);
  if (x->reward_source != 0 && x->reward_source != 1) return "reward_source must be 0 or 1, got " + std::to_string(x->reward_source);
  if (x->reserved != 0) return "reserved must be 0";
  if (!x->stats) return "null stats";
  return "";
}

std::string check_episode_args(const uint8_t* done, const double* reward, const double* ep_return, const int32_t* ep_len, int E, int n_eval,
                               int source) {
  if (E < 1) return "E must be >= 1, got " + std::to_string(E);
  if (n_eval < 1) return "n_eval_episodes must be >= 1, got " + std::to_string(n_eval);
  if (source != 0 && source != 1) return "reward_source must be 0 or 1, got " + std::to_string(source);
  if (!done) return "null done";
  if (!reward) return "null reward";
  if (source == 1 && !ep_return) return "null ep_return";
  if (source == 1 && !ep_len) return "null ep_len";
  return "";
}

const FleetHandleBase* base_of(const void* h) { return reinterpret_cast<const FleetHandleBase*>(h); }

enum { kObs, kRaw, kAct, kRawReward, kReward, kDone, kSums, kLengths, kCounts, kEpReward, kEpLength, kScalars, kSnapshot, kArrays };

}  // namespace

struct FleetEval {
  fleet_handle env = nullptr;  // borrowed, as are the two below
  fleet_norm_handle norm = nullptr;
  fleet_policy_handle policy = nullptr;  // the actor is a policy's image (fleet_eval_create), or ...
  fleet_qtarget_handle nets = nullptr;   // ... a squashed SAC image (fleet_saceval_create): exactly one of the two
  FleetMlpHandle* pol = nullptr;  // the actor's image: its device and stream
  std::string error;              // fleet_eval_last_error(handle)
  char* block = nullptr;          // owned
  int E = 0, D = 0, A = 0, M = 0, launches = 0;
  bool ran = false;               // a run call was enqueued: the snapshot may hold something
  size_t weights_at = 0;          // the image's first weight, in floats (its record lies in front)
  uint64_t at[kArrays] = {}, bytes = 0;

  template <typename T>
  T* arr(int which) const { return reinterpret_cast<T*>(block + at[which]); }
  // the scalars: {listed u64, best_mean_reward f64, evaluations u64, gate u32}
  uint64_t* listed() const { return arr<uint64_t>(kScalars); }
  double* best() const { return arr<double>(kScalars) + 1; }
  uint64_t* evals() const { return arr<uint64_t>(kScalars) + 2; }
  uint32_t* gate() const { return arr<uint32_t>(kScalars) + 6; }
  hipStream_t stream() const { return env->stream; }
};

namespace {

// what the refusals call the actor of either kind of handle, and the entry that moves it to another stream
struct ActorWords {
  const char *noun, *set_stream;
};
const ActorWords kPolicyWords = {"policy", "fleet_policy_set_stream"}, kSacWords = {"networks handle", "fleet_qtarget_set_stream"};

// env, normaliser and actor launch on one stream; `more`: another image of the actor's kind
std::string check_streams(const FleetEval* h, const FleetHandleBase* more = nullptr) {
  if (h->norm && base_of(h->norm)->stream != h->env->stream)
    return "the normaliser launches on another stream than the env: fleet_norm_set_stream it to the env's first";
  if (h->pol->stream != h->env->stream)
    return h->nets ? "the networks launch on another stream than the env: fleet_qtarget_set_stream them to the env's first"
                   : "the policy launches on another stream than the env: fleet_policy_set_stream it to the env's first";
  if (more && more->stream != h->env->stream) {
    const ActorWords& w = h->nets ? kSacWords : kPolicyWords;
    return std::string("the destination ") + w.noun + " launches on another stream than the env: " + w.set_stream + " it to the env's first";
  }
  return "";
}

EpisodeArgs episode_args(const FleetEval* h) {
  EpisodeArgs a{};
  a.sums = h->arr<double>(kSums), a.lengths = h->arr<int32_t>(kLengths), a.counts = h->arr<int32_t>(kCounts);
  a.ep_reward = h->arr<double>(kEpReward), a.ep_length = h->arr<int32_t>(kEpLength), a.listed = h->listed();
  a.max_episodes = h->M;
  return a;
}

int launch_clear(FleetEval* h) {
  hipLaunchKernelGGL(eval_clear, dim3(((unsigned)h->E + 255) / 256), dim3(256), 0, h->stream(), h->arr<double>(kSums), h->arr<int32_t>(kLengths),
                     h->arr<int32_t>(kCounts), h->listed(), h->E);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

int launch_copy(FleetEval* h, const float* src, float* dst, const uint32_t* gate) {
  const size_t n4 = (h->pol->floats - h->weights_at) / 4;
  hipLaunchKernelGGL(eval_copy, dim3(grid_for(n4, 256, kEvalCopyMaxBlocks)), dim3(256), 0, h->stream(),
                     reinterpret_cast<const float4*>(src + h->weights_at), reinterpret_cast<float4*>(dst + h->weights_at), n4, gate);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

bool same_layout(const FleetMlpHandle* a, const FleetMlpHandle* b) {
  if (a->floats != b->floats || a->n_nets != b->n_nets || a->record_bytes != b->record_bytes) return false;
  for (int n = 0; n < a->n_nets; ++n) {
    if (a->nets[n].n_layers != b->nets[n].n_layers) return false;
    for (int l = 0; l < a->nets[n].n_layers; ++l) {
      const PolicyLayer &x = a->nets[n].layer[l], &y = b->nets[n].layer[l];
      if (x.in != y.in || x.out != y.out || x.w_off != y.w_off || x.b_off != y.b_off) return false;
    }
  }
  return true;
}

// Both create entries: `actor` is a fleet_policy_handle, or with `sac` the fleet_qtarget_handle of fleet_sac_create; the refusals
// name it "the policy" or "the networks".
int create_on(const char* entry, fleet_handle env, fleet_norm_handle norm, void* actor, bool sac, const FleetEvalParams* p, fleet_eval_handle* out) {
  const char* const noun = sac ? "networks" : "policy";
  if (out) *out = nullptr;
  std::string why = check_params(p);
  if (!why.empty()) {
  } else if (!out) why = "null output handle";
  else if (!env) why = "null env handle";
  else if (!actor) why = std::string("null ") + noun + " handle";
  if (!why.empty()) return handle_refuse(g_eval_error, entry, why, FLEET_ERR_INVALID);
  FleetMlpHandle* pol = mlp_borrow(actor, sac ? sizeof(QTargetDesc) : sizeof(PolicyDesc), noun, &why);
  if (!pol) return handle_refuse(g_eval_error, entry, why, FLEET_ERR_INVALID);
  const int E = env->d.E, D = env->d.obs_dim, A = env->d.N;
  const PolicyHeadDesc& head = pol->nets[0];
  const int pd = head.layer[0].in;
  const int pa = sac ? static_cast<const QTargetDesc*>(pol->record)->act_dim : head.layer[head.n_layers - 1].out;
  const size_t weights_at = (size_t)mlp_round_up((int)pol->record_bytes, 256) / 4;
  const std::string the = std::string("the ") + noun, whose = sac ? "the networks'" : "the policy's";
  if (!env->d.auto_reset) why = "the env needs auto_reset = 1: an evaluation runs across episode ends";
  else if (sac && !qtarget_squashed(pol)) why = "the networks' actor is not a squashed Gaussian: fleet_sac_create makes one";
  else if (pol->device != env->device)
    why = the + (sac ? " lie" : " lies") + " on device " + std::to_string(pol->device) + ", the env on device " + std::to_string(env->device);
  else if (pd != D) why = whose + " obs_dim is " + std::to_string(pd) + ", the env's " + std::to_string(D);
  else if (pa != A) why = whose + " act_dim is " + std::to_string(pa) + ", the env's " + std::to_string(A);
  else if (pol->floats < weights_at || (pol->floats - weights_at) % 4 != 0) why = the + " image's weights are no multiple of four floats";
  else if (norm) (void)fleet_norm_check_fit(norm, E, D, env->device, &why);
  if (!why.empty()) return handle_refuse(g_eval_error, entry, why, FLEET_ERR_INVALID);
  FleetEval* h = new FleetEval();
  h->env = env, h->norm = norm, h->pol = pol;
  if (sac) h->nets = static_cast<fleet_qtarget_handle>(actor);
  else h->policy = static_cast<fleet_policy_handle>(actor);
  h->E = E, h->D = D, h->A = A, h->M = p->max_episodes, h->weights_at = weights_at;
  const uint64_t e = (uint64_t)E, od = e * D * 4, m = (uint64_t)h->M;
  const uint64_t bytes[kArrays] = {od, norm ? od : 0, e * A * 4, e * 8, e * 8, e, e * 8, e * 4, e * 4, m * 8, m * 4, 32, (uint64_t)pol->floats * 4};
  uint64_t off = 0;
  for (int i = 0; i < kArrays; ++i) h->at[i] = off, off = (off + bytes[i] + 255) / 256 * 256;
  if (!norm) h->at[kRaw] = h->at[kObs];
  h->bytes = off;
  int rc = FLEET_OK;
  void* q = nullptr;
  const double ninf = -std::numeric_limits<double>::infinity();
  if (hipSetDevice(env->device) != hipSuccess) why = "hipSetDevice failed", rc = FLEET_ERR_HIP;
  else if (hipMalloc(&q, off) != hipSuccess) why = "hipMalloc of the evaluation block's " + std::to_string(off) + " bytes failed", rc = FLEET_ERR_HIP;
  else if (hipMemset(q, 0, off) != hipSuccess || hipMemcpy(static_cast<char*>(q) + h->at[kScalars] + 8, &ninf, 8, hipMemcpyHostToDevice) != hipSuccess ||
           hipDeviceSynchronize() != hipSuccess)
    why = "clearing the evaluation block failed", rc = FLEET_ERR_HIP;
  h->block = static_cast<char*>(q);
  if (rc != FLEET_OK) {
    (void)hipGetLastError();
    fleet_eval_destroy(h);
    return handle_refuse(g_eval_error, entry, why, rc);
  }
  *out = h;
  return FLEET_OK;
}

// fleet_eval_best_load_dev and fleet_saceval_best_load_dev: the snapshot into another image of the handle's kind, one launch
int best_load(FleetEval* h, const char* entry, void* dst, bool sac) {
  std::string why;
  FleetMlpHandle* to = nullptr;
  if (h && sac != (h->nets != nullptr)) {
    why = sac ? "the handle evaluates a policy (fleet_eval_create): fleet_eval_best_load_dev loads its snapshot"
              : "the handle evaluates SAC networks (fleet_saceval_create): fleet_saceval_best_load_dev loads its snapshot";
  } else if (h) {
    const ActorWords& w = sac ? kSacWords : kPolicyWords;
    const std::string the = std::string("the destination ") + w.noun;
    to = mlp_borrow(dst, sac ? sizeof(QTargetDesc) : sizeof(PolicyDesc), sac ? "networks" : "policy", &why);
    if (to && sac && !qtarget_squashed(to)) why = the + "'s actor is not a squashed Gaussian: fleet_sac_create makes one";
    else if (to && to->device != h->env->device) why = the + " lies on another device than the env";
    else if (to && !same_layout(to, h->pol)) why = the + "'s layout differs from the evaluated " + (sac ? "networks'" : "policy's");
    else if (to) why = check_streams(h, to);
  }
  if (const int rc = handle_enter(entry, why, h, g_eval_error); rc != FLEET_OK) return rc;
  if (!h->ran) {
    h->error = std::string(entry) + ": no evaluation has run on this handle: the snapshot is empty";
    return FLEET_ERR_STATE;
  }
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  return launch_copy(h, h->arr<float>(kSnapshot), reinterpret_cast<float*>(to->block), nullptr);
}

}  // namespace

extern "C" {

int fleet_eval_create(fleet_handle env, fleet_norm_handle norm, fleet_policy_handle policy, const FleetEvalParams* p, fleet_eval_handle* out) {
  return create_on("fleet_eval_create", env, norm, policy, false, p, out);
}

int fleet_saceval_create(fleet_handle env, fleet_norm_handle norm, fleet_qtarget_handle nets, const FleetEvalParams* p, fleet_eval_handle* out) {
  return create_on("fleet_saceval_create", env, norm, nets, true, p, out);
}

int fleet_eval_destroy(fleet_eval_handle h) {
  if (!h) return FLEET_OK;
  if (h->block) {  // (hipFree waits for the device: whatever still reads the block is done)
    (void)hipSetDevice(h->env->device);
    (void)hipFree(h->block);
  }
  delete h;
  return FLEET_OK;
}

const char* fleet_eval_last_error(fleet_eval_handle h) { return h ? h->error.c_str() : g_eval_error.c_str(); }

int fleet_eval_describe(fleet_eval_handle h, FleetEvalInfo* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  out->num_envs = h->E, out->obs_dim = h->D, out->act_dim = h->A, out->max_episodes = h->M;
  out->has_norm = h->norm != nullptr, out->launches = h->launches;
  out->block_bytes = h->bytes, out->snapshot_floats = h->pol->floats;
  out->obs = h->arr<float>(kObs), out->raw_obs = h->arr<float>(kRaw), out->actions = h->arr<float>(kAct);
  out->raw_reward = h->arr<double>(kRawReward), out->reward = h->arr<double>(kReward), out->done = h->arr<uint8_t>(kDone);
  out->sums = h->arr<double>(kSums), out->lengths = h->arr<int32_t>(kLengths), out->counts = h->arr<int32_t>(kCounts);
  out->ep_reward = h->arr<double>(kEpReward), out->ep_length = h->arr<int32_t>(kEpLength);
  out->listed = h->listed(), out->best_mean_reward = h->best(), out->evaluations = h->evals(), out->gate = h->gate();
  out->snapshot = h->arr<float>(kSnapshot);
  return FLEET_OK;
}

int fleet_eval_sync_norm_dev(fleet_norm_handle dst, fleet_norm_handle src) {
  std::string why;
  if (fleet_norm_check_sync(dst, src, &why) != FLEET_OK) return handle_refuse(g_eval_error, "fleet_eval_sync_norm_dev", why, FLEET_ERR_INVALID);
  hipError_t e = hipSetDevice(base_of(dst)->device);
  if (e == hipSuccess) e = fleet_norm_enqueue_sync(dst, src);
  if (e != hipSuccess) return handle_refuse(g_eval_error, "fleet_eval_sync_norm_dev", hipGetErrorString(e), FLEET_ERR_HIP);
  return FLEET_OK;
}

int fleet_eval_run_dev(fleet_eval_handle h, const FleetEvalArgs* x) {
  std::string why = check_run_args(x);
  if (h && why.empty()) {
    if (x->n_eval_episodes > h->M)
      why = "n_eval_episodes must be <= the handle's max_episodes " + std::to_string(h->M) + ", got " + std::to_string(x->n_eval_episodes);
    else why = check_streams(h);
    if (why.empty() && x->sync_from) {
      if (!h->norm) why = "sync_from given to a handle without a normaliser";
      else (void)fleet_norm_check_sync(h->norm, x->sync_from, &why);
    }
  }
  if (const int rc = handle_enter("fleet_eval_run_dev", why, h, g_eval_error); rc != FLEET_OK) return rc;
  const auto failed = [&](int rc, const char* said) {
    h->error = std::string("fleet_eval_run_dev: ") + said;
    return rc;
  };
  h->launches = 0;
  h->ran = true;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  if (x->sync_from) {
    FLEET_HANDLE_TRY(h, fleet_norm_enqueue_sync(h->norm, x->sync_from));
    h->launches += 1;
  }
  float *obs = h->arr<float>(kObs), *raw = h->arr<float>(kRaw), *act = h->arr<float>(kAct);
  double* raw_reward = h->arr<double>(kRawReward);
  double* reward = h->norm ? h->arr<double>(kReward) : raw_reward;
  uint8_t* done = h->arr<uint8_t>(kDone);
  if (const int rc = fleet_reset_dev(h->env, nullptr, raw); rc != FLEET_OK) return failed(rc, fleet_last_error(h->env));
  h->launches += 1;
  if (h->norm) {
    if (const int rc = fleet_norm_reset_dev(h->norm, raw, obs); rc != FLEET_OK) return failed(rc, fleet_norm_last_error(h->norm));
    h->launches += 1;
  }
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  if (const int rc = launch_clear(h); rc != FLEET_OK) return rc;
  h->launches += 1;
  EpisodeArgs a = episode_args(h);
  a.done = done, a.reward = reward, a.env = h->env->d.env, a.cold = h->env->d.cold;
  a.E = h->E, a.n_eval = x->n_eval_episodes, a.round32 = h->norm == nullptr, a.source = x->reward_source;
  FleetSacActArgs det{};  // a SAC handle's action: tanhf(mu), no noise, the observation already normalised
  det.struct_bytes = (int32_t)sizeof det;
  det.noise_mode = FLEET_EXPLORE_NOISE_DRAW, det.deterministic = 1, det.actions = act;
  for (int t = 0; t < x->n_steps; ++t) {
    if (h->nets) {
      if (const int rc = fleet_sac_act_dev(h->nets, obs, h->E, nullptr, &det); rc != FLEET_OK) return failed(rc, fleet_sac_last_error(h->nets));
    } else if (const int rc = fleet_policy_forward_dev(h->policy, obs, h->E, nullptr, act, nullptr); rc != FLEET_OK) {
      return failed(rc, fleet_policy_last_error(h->policy));
    }
    if (const int rc = fleet_step_dev(h->env, act, FLEET_ACT_F32, raw, raw_reward, done, nullptr); rc != FLEET_OK) return failed(rc, fleet_last_error(h->env));
    h->launches += 2;
    if (h->norm) {
      if (const int rc = fleet_norm_step_dev(h->norm, raw, raw_reward, done, nullptr, obs, reward, nullptr); rc != FLEET_OK)
        return failed(rc, fleet_norm_last_error(h->norm));
      h->launches += 1;
    }
    hipLaunchKernelGGL(eval_episodes<true>, dim3(1), dim3(kEvalScanThreads), 0, h->stream(), a);
    FLEET_HANDLE_TRY(h, hipGetLastError());
    h->launches += 1;
  }
  FinishArgs f{};
  f.ep_reward = h->arr<double>(kEpReward), f.ep_length = h->arr<int32_t>(kEpLength), f.listed = h->listed();
  f.best = h->best(), f.evals = h->evals(), f.gate = h->gate(), f.out = x->stats;
  f.num_timesteps = x->num_timesteps, f.max_episodes = (uint32_t)h->M;
  hipLaunchKernelGGL(eval_finish, dim3(1), dim3(kEvalThreads), 0, h->stream(), f);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  h->launches += 1;
  if (const int rc = launch_copy(h, reinterpret_cast<const float*>(h->pol->block), h->arr<float>(kSnapshot), h->gate()); rc != FLEET_OK) return rc;
  h->launches += 1;
  return FLEET_OK;
}

int fleet_eval_episodes_dev(fleet_eval_handle h, const uint8_t* done, const double* reward, const double* ep_return, const int32_t* ep_len, int E,
                            int n_eval_episodes, int reward_source) {
  std::string why = check_episode_args(done, reward, ep_return, ep_len, E, n_eval_episodes, reward_source);
  if (h && why.empty() && E > h->E) why = "E must be <= the handle's num_envs " + std::to_string(h->E) + ", got " + std::to_string(E);
  if (const int rc = handle_enter("fleet_eval_episodes_dev", why, h, g_eval_error); rc != FLEET_OK) return rc;
  EpisodeArgs a = episode_args(h);
  a.done = done, a.reward = reward, a.ep_ret = ep_return, a.ep_len = ep_len;
  a.E = E, a.n_eval = n_eval_episodes, a.round32 = 0, a.source = reward_source;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  hipLaunchKernelGGL(eval_episodes<false>, dim3(1), dim3(kEvalScanThreads), 0, h->stream(), a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

int fleet_eval_clear_dev(fleet_eval_handle h) {
  if (const int rc = handle_enter("fleet_eval_clear_dev", "", h, g_eval_error); rc != FLEET_OK) return rc;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  return launch_clear(h);
}

int fleet_eval_best_load_dev(fleet_eval_handle h, fleet_policy_handle dst) { return best_load(h, "fleet_eval_best_load_dev", dst, false); }

int fleet_saceval_best_load_dev(fleet_eval_handle h, fleet_qtarget_handle dst) { return best_load(h, "fleet_saceval_best_load_dev", dst, true); }

int fleet_eval_best_export_dev(fleet_eval_handle h, float* const* tensors, int count) {
  const std::string why = h ? check_streams(h) : "";
  if (const int rc = handle_enter("fleet_eval_best_export_dev", why, h, g_eval_error); rc != FLEET_OK) return rc;
  if (!h->ran) {
    h->error = "fleet_eval_best_export_dev: no evaluation has run on this handle: the snapshot is empty";
    return FLEET_ERR_STATE;
  }
  const int rc = mlp_launch_relay_at(h->pol, h->arr<float>(kSnapshot), kMlpExport, "fleet_eval_best_export_dev", tensors, count, 0.0f, 0.0f);
  if (rc != FLEET_OK) h->error = h->pol->error;
  return rc;
}

int fleet_eval_episodes_read(fleet_eval_handle h, double* ep_reward, int32_t* ep_length, uint64_t* count) {
  if (const int rc = handle_enter("fleet_eval_episodes_read", "", h, g_eval_error); rc != FLEET_OK) return rc;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  const size_t m = (size_t)h->M;
  if (ep_reward) FLEET_HANDLE_TRY(h, hipMemcpyAsync(ep_reward, h->arr<double>(kEpReward), m * 8, hipMemcpyDeviceToHost, h->stream()));
  if (ep_length) FLEET_HANDLE_TRY(h, hipMemcpyAsync(ep_length, h->arr<int32_t>(kEpLength), m * 4, hipMemcpyDeviceToHost, h->stream()));
  if (count) FLEET_HANDLE_TRY(h, hipMemcpyAsync(count, h->listed(), 8, hipMemcpyDeviceToHost, h->stream()));
  FLEET_HANDLE_TRY(h, hipStreamSynchronize(h->stream()));
  return FLEET_OK;
}

}  // extern "C"
