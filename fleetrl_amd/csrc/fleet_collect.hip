// fleet_collect.hip -- stable-baselines3's collect_rollouts as ONE enqueue-only call (include/fleet_hip.h "collect_rollouts on the
// device"; fleet_collect.h): per env step the exploration launch, the env step, the normaliser step and the buffer's add through
// their own entries, as they are, on one stream, and the one thing of SB3's rollout log nothing else keeps on the device -- the ring
// of the last W finished episodes.  The handle borrows an env, an optional normaliser and a policy and owns one block: the carry
// buffers (two sides that ping-pong), the raw buffers, the step's small arrays and the ring.  The actor may also be the squashed-
// Gaussian networks of fleet_sac_create (include/fleet_hip_sac_loop.h, fleet_saccollect_*): the off-policy loop with another action.
//   collect_episodes  ONE workgroup of 1024 threads per env step: the step's finished envs in env order (ballot and popcount per
//              wavefront, chunks of 1024 envs), the k-th of c to slot (count + k) % W iff c - k <= W; then count += c.  Behind one of
//              two loaders: the env's records, or the caller's arrays.
//   collect_finish    one workgroup of 256 threads per call: the ordered float64 sums over the ring, the means, the statistics block.
//   collect_fill      the reset's episode_start = 1.
// No atomics, no ordering between workgroups: launch boundaries only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/fleet_hip_sac_loop.h"
#include "fleet_batch.h"
#include "fleet_collect.h"
#include "fleet_handle.h"
#include "fleet_mlp.h"
#include "fleet_norm.h"
#include "fleet_policy.h"
#include "fleet_qtarget.h"

namespace {

// ---- collect_episodes ------------------------------------------------------------------------------------------------------------
struct EpisodeArgs {
  const uint8_t* done;    // u8[E]: the step's done flags
  const EnvRec* env;      // the env's records and ...
  const FleetCold* cold;  // ... its cold block (last_len[E]), or
  const double* ep_ret;   // the caller's arrays f64[E] and ...
  const int32_t* ep_len;  // ... i32[E]
  double* ring_return;    // f64[W]
  int32_t* ring_length;   // i32[W]
  uint64_t* counts;       // {appended so far, appended since the last closing launch}
  int E;
  uint32_t W;
};

template <bool kFromEnv>
__global__ __launch_bounds__(kCollectScanThreads) void collect_episodes(EpisodeArgs a) {
  __shared__ int s_wave[kCollectScanWaves];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int E = a.E;
  const uint8_t* __restrict__ done = a.done;
  const uint64_t count = a.counts[0], since = a.counts[1];  // (thread 0 writes them behind the last barrier)
  // c, the step's finished envs: the rule needs it before the first of them is placed
  int mine = 0;
  for (int e0 = 0; e0 < E; e0 += kCollectScanThreads) {
    const int e = e0 + (int)threadIdx.x;
    mine += __popcll(__ballot((e < E) && done[e] != 0));  // (every lane of a wavefront holds its wavefront's total)
  }
  if (lane == 0) s_wave[wave] = mine;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  int c = 0;
#pragma unroll
  for (int w = 0; w < kCollectScanWaves; ++w) c += s_wave[w];
  if (c == 0) return;  // (uniform over the workgroup: no episode ended, the ring and its counts stay)
  __syncthreads();     // (s_wave is rewritten below)
  for (int e0 = 0; e0 < E; e0 += kCollectScanThreads) {
    const int e = e0 + (int)threadIdx.x;
    const bool f = (e < E) && done[e] != 0;
    const unsigned long long m = __ballot(f);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < wave; ++w) off += s_wave[w];
    if (f) {
      uint32_t slot;
      if (collect_slot(count, (uint32_t)c, (uint32_t)(off + before), a.W, &slot)) {  // (slot < W)
        a.ring_return[slot] = kFromEnv ? a.env[e].last_ep_return : a.ep_ret[e];
        a.ring_length[slot] = kFromEnv ? a.cold->last_len[e] : a.ep_len[e];
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int w = 0; w < kCollectScanWaves; ++w) tot += s_wave[w];
      s_base += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    a.counts[0] = count + (uint64_t)c;
    a.counts[1] = since + (uint64_t)c;
  }
}

// ---- collect_finish --------------------------------------------------------------------------------------------------------------
struct FinishArgs {
  const double* ring_return;
  const int32_t* ring_length;
  uint64_t* counts;
  double* out;  // the statistics block f64[FLEET_COLLECT_STATS]
  uint64_t steps_after;  // first_step + steps
  uint32_t W;
};

// the ordered sum's tree: every thread's `v` in, the total out to every thread
__device__ inline double tree_total(double v, double* red) {
  __syncthreads();  // (the previous total has been read)
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = kCollectThreads / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kCollectThreads) void collect_finish(FinishArgs a) {
  __shared__ double red[kCollectThreads];
  const uint32_t tid = threadIdx.x;
  const uint64_t count = a.counts[0], since = a.counts[1];
  const uint32_t n = count < (uint64_t)a.W ? (uint32_t)count : a.W;
  double sr = 0.0, sl = 0.0;
  for (uint32_t s = tid; s < n; s += kCollectThreads) {
    sr = sr + a.ring_return[s];
    sl = sl + (double)a.ring_length[s];
  }
  const double tr = tree_total(sr, red), tl = tree_total(sl, red);
  if (tid == 0) {
    a.out[0] = n ? tr / (double)n : (double)NAN;
    a.out[1] = n ? tl / (double)n : (double)NAN;
    a.out[2] = (double)since;
    a.out[3] = (double)count;
    a.out[4] = (double)a.steps_after;
    for (int k = 5; k < kCollectStats; ++k) a.out[k] = 0.0;
    a.counts[1] = 0;
  }
}

// ---- collect_fill ----------------------------------------------------------------------------------------------------------------
__global__ void collect_fill(uint8_t* __restrict__ p, int n, uint8_t v) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) p[i] = v;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_collect_error;  // of the last failed call without a handle

std::string check_params(const FleetCollectParams* p) {
  if (!p) return "null FleetCollectParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetCollectParams)) return "FleetCollectParams.struct_bytes does not match this library";
  if (p->stats_window < 1 || p->stats_window > kCollectMaxWindow)
    return "stats_window must be in 1.." + std::to_string(kCollectMaxWindow) + ", got " + std::to_string(p->stats_window);
  return "";
}

// what fleet_collect_ppo_dev refuses, looked at without the handle; "" when the arguments pass
std::string check_ppo_args(const FleetCollectPpoArgs* x) {
  if (!x) return "null FleetCollectPpoArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetCollectPpoArgs)) return "FleetCollectPpoArgs.struct_bytes does not match this library";
  if (x->n_steps < 1) return "n_steps must be >= 1, got " + std::to_string(x->n_steps);
  if (x->reserved != 0) return "reserved must be 0";
  if (x->env_id_offset < 0) return "env_id_offset must be >= 0, got " + std::to_string(x->env_id_offset);
  if (!x->buffer) return "null rollout handle";
  if (!x->log_std) return "null scale (log_std or sigma)";
  if (!x->stats) return "null stats";
  return "";
}

std::string check_offpolicy_args(const FleetCollectOffpolicyArgs* x) {
  if (!x) return "null FleetCollectOffpolicyArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetCollectOffpolicyArgs)) return "FleetCollectOffpolicyArgs.struct_bytes does not match this library";
  if (x->n_steps < 1) return "n_steps must be >= 1, got " + std::to_string(x->n_steps);
  if (x->reserved != 0) return "reserved must be 0";
  if (x->env_id_offset < 0) return "env_id_offset must be >= 0, got " + std::to_string(x->env_id_offset);
  if (!x->replay) return "null replay handle";
  if (!x->sigma) return "null scale (log_std or sigma)";
  if (!(x->noise_lo <= x->noise_hi)) return "the bounds need noise_lo <= noise_hi";
  if (!x->stats) return "null stats";
  return "";
}

// what fleet_saccollect_uniform_dev and fleet_saccollect_sac_dev refuse, looked at without their handles
std::string check_uniform_args(int E, const FleetSacUniformArgs* x) {
  if (!x) return "null FleetSacUniformArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetSacUniformArgs)) return "FleetSacUniformArgs.struct_bytes does not match this library";
  if (E < 1) return "E must be >= 1, got " + std::to_string(E);
  if (!x->actions) return "null actions";
  if (x->env_id_offset < 0) return "env_id_offset must be >= 0, got " + std::to_string(x->env_id_offset);
  if (!(x->lo <= x->hi)) return "the bounds need lo <= hi";
  return "";
}

std::string check_sac_args(const FleetSacCollectArgs* x) {
  if (!x) return "null FleetSacCollectArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetSacCollectArgs)) return "FleetSacCollectArgs.struct_bytes does not match this library";
  if (x->n_steps < 1) return "n_steps must be >= 1, got " + std::to_string(x->n_steps);
  if (x->reserved != 0) return "reserved must be 0";
  if (x->env_id_offset < 0) return "env_id_offset must be >= 0, got " + std::to_string(x->env_id_offset);
  if (!x->replay) return "null replay handle";
  if (!(x->noise_lo <= x->noise_hi)) return "the bounds need noise_lo <= noise_hi";
  if (!x->stats) return "null stats";
  return "";
}

std::string check_episode_args(const uint8_t* done, const double* ep_return, const int32_t* ep_len, int E) {
  if (E < 1) return "E must be >= 1, got " + std::to_string(E);
  if (!done) return "null done";
  if (!ep_return) return "null ep_return";
  if (!ep_len) return "null ep_len";
  return "";
}

std::string check_finish_args(int32_t steps, const double* stats) {
  if (steps < 0) return "steps must be >= 0, got " + std::to_string(steps);
  if (!stats) return "null stats";
  return "";
}

// The handles this family is created on keep their definitions in their own files; what it needs of them is what their scaffolds
// share: a normaliser's and a noise process's first base is FleetHandleBase, a rollout buffer's and a replay buffer's is
// FleetBufferBase<their layout> (fleet_handle.h), and mlp_borrow relies on the image's handle being a policy's first base.
using RolloutBase = FleetBufferBase<FleetRolloutLayout>;
using ReplayBase = FleetBufferBase<FleetReplayLayout>;
const FleetHandleBase* base_of(const void* h) { return reinterpret_cast<const FleetHandleBase*>(h); }

enum { kObs0, kObs1, kRaw0, kRaw1, kTerm, kRawReward, kReward, kStart0, kStart1, kEnvAct, kEps, kLastValues, kRingReturn, kRingLength,
       kCounts, kArrays };

}  // namespace

struct FleetCollect {
  fleet_handle env = nullptr;  // borrowed, as are the two below
  fleet_norm_handle norm = nullptr;
  fleet_policy_handle policy = nullptr;  // the actor is a policy's image (fleet_collect_create), or ...
  fleet_qtarget_handle nets = nullptr;   // ... a squashed SAC image (fleet_saccollect_create): exactly one of the two
  FleetMlpHandle* pol = nullptr;  // the actor's image: its device and stream
  std::string error;              // fleet_collect_last_error(handle)
  char* block = nullptr;          // owned
  int E = 0, D = 0, A = 0, W = 0, n_heads = 0, cur = 0, launches = 0;
  uint64_t at[kArrays] = {}, bytes = 0;

  template <typename T>
  T* arr(int which) const { return reinterpret_cast<T*>(block + at[which]); }
  float* obs(int side) const { return arr<float>(kObs0 + side); }
  float* raw(int side) const { return arr<float>(kRaw0 + side); }  // (the carry buffers themselves without a normaliser)
  uint8_t* start(int side) const { return arr<uint8_t>(kStart0 + side); }
  hipStream_t stream() const { return env->stream; }
};

namespace {

// env, normaliser and policy launch on one stream; `more`: a buffer's or a noise handle's stream, with its noun
std::string check_streams(const FleetCollect* h, const FleetHandleBase* more = nullptr, const char* noun = nullptr) {
  if (h->norm && base_of(h->norm)->stream != h->env->stream)
    return "the normaliser launches on another stream than the env: fleet_norm_set_stream it to the env's first";
  if (h->pol->stream != h->env->stream)
    return h->nets ? "the networks launch on another stream than the env: fleet_qtarget_set_stream them to the env's first"
                   : "the policy launches on another stream than the env: fleet_policy_set_stream it to the env's first";
  if (more && more->stream != h->env->stream)
    return std::string("the ") + noun + " launches on another stream than the env: set its stream to the env's first";
  return "";
}

// which run call serves the other kind of handle
const char* const kServedBySac = "the handle borrows SAC networks (fleet_saccollect_create): fleet_saccollect_sac_dev runs it";
const char* const kServedByPolicy = "the handle borrows a policy (fleet_collect_create): fleet_collect_ppo_dev and fleet_collect_offpolicy_dev run it";

// what the off-policy run calls refuse about their replay buffer; "" when it fits and launches on the env's stream
std::string check_replay(const FleetCollect* h, fleet_replay_handle replay) {
  const ReplayBase* rb = reinterpret_cast<const ReplayBase*>(replay);
  const FleetReplayLayout& L = rb->L;
  const int E = (int)(L.row_bytes[FLEET_REPLAY_REWARDS] / 4);
  const int D = (int)(L.row_bytes[FLEET_REPLAY_OBS] / L.row_bytes[FLEET_REPLAY_REWARDS]);
  const int A = (int)(L.row_bytes[FLEET_REPLAY_ACTIONS] / L.row_bytes[FLEET_REPLAY_REWARDS]);
  if (rb->device != h->env->device) return "the replay buffer lies on another device than the env";
  if (E != h->E) return "the replay buffer's num_envs is " + std::to_string(E) + ", the env's " + std::to_string(h->E);
  if (D != h->D) return "the replay buffer's obs_dim is " + std::to_string(D) + ", the env's " + std::to_string(h->D);
  if (A != h->A) return "the replay buffer's act_dim is " + std::to_string(A) + ", the env's " + std::to_string(h->A);
  return check_streams(h, rb, "replay buffer");
}

int launch_episodes(FleetCollect* h, const uint8_t* done) {
  EpisodeArgs a{};
  a.done = done, a.env = h->env->d.env, a.cold = h->env->d.cold;
  a.ring_return = h->arr<double>(kRingReturn), a.ring_length = h->arr<int32_t>(kRingLength), a.counts = h->arr<uint64_t>(kCounts);
  a.E = h->E, a.W = (uint32_t)h->W;
  hipLaunchKernelGGL(collect_episodes<true>, dim3(1), dim3(kCollectScanThreads), 0, h->stream(), a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  h->launches += 1;
  return FLEET_OK;
}

int launch_finish(FleetCollect* h, uint64_t steps_after, double* stats) {
  FinishArgs f{};
  f.ring_return = h->arr<double>(kRingReturn), f.ring_length = h->arr<int32_t>(kRingLength), f.counts = h->arr<uint64_t>(kCounts);
  f.out = stats, f.steps_after = steps_after, f.W = (uint32_t)h->W;
  hipLaunchKernelGGL(collect_finish, dim3(1), dim3(kCollectThreads), 0, h->stream(), f);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  h->launches += 1;
  return FLEET_OK;
}

// The off-policy run calls' loop, once: per env step `action(s, cur, failed)` enqueues what writes the handle's env_actions from the
// carry observation of side `cur` (and counts its launches beyond the one counted here), then the env's step, the normaliser's step,
// the buffer's add and the episode launch; the sides swap; the closing launch ends the call.  failed(rc, said) puts "<entry>: <said>"
// into the handle's error and returns rc.
template <typename Action>
int offpolicy_loop(FleetCollect* h, const char* entry, fleet_replay_handle replay, int n_steps, uint64_t first_step, double* stats,
                   const Action& action) {
  const auto failed = [&](int rc, const char* said) {
    h->error = std::string(entry) + ": " + said;
    return rc;
  };
  h->launches = 0;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  float* act = h->arr<float>(kEnvAct);
  float* term = h->arr<float>(kTerm);
  double* raw_reward = h->arr<double>(kRawReward);
  double* reward = h->arr<double>(kReward);
  for (int t = 0; t < n_steps; ++t) {
    const int cur = h->cur, nxt = cur ^ 1;
    if (const int rc = action(first_step + (uint64_t)t, cur, failed); rc != FLEET_OK) return rc;
    if (const int rc = fleet_step_dev(h->env, act, FLEET_ACT_F32, h->raw(nxt), raw_reward, h->start(nxt), term); rc != FLEET_OK)
      return failed(rc, fleet_last_error(h->env));
    h->launches += 2;
    if (h->norm) {
      if (const int rc = fleet_norm_step_dev(h->norm, h->raw(nxt), raw_reward, h->start(nxt), nullptr, h->obs(nxt), reward, nullptr); rc != FLEET_OK)
        return failed(rc, fleet_norm_last_error(h->norm));
      h->launches += 1;
    }
    if (const int rc = fleet_replay_add_dev(replay, h->raw(cur), h->raw(nxt), act, raw_reward, FLEET_ACT_F64, h->start(nxt), term, nullptr); rc != FLEET_OK)
      return failed(rc, fleet_replay_last_error(replay));
    h->launches += 1;
    if (const int rc = launch_episodes(h, h->start(nxt)); rc != FLEET_OK) return rc;
    h->cur = nxt;
  }
  return launch_finish(h, first_step + (uint64_t)n_steps, stats);
}

// Both create entries: `actor` is a fleet_policy_handle, or with `sac` the fleet_qtarget_handle of fleet_sac_create; the refusals
// name it "the policy" or "the networks".
int create_on(const char* entry, fleet_handle env, fleet_norm_handle norm, void* actor, bool sac, const FleetCollectParams* p,
              fleet_collect_handle* out) {
  const char* const noun = sac ? "networks" : "policy";
  if (out) *out = nullptr;
  std::string why = check_params(p);
  if (!why.empty()) {
  } else if (!out) why = "null output handle";
  else if (!env) why = "null env handle";
  else if (!actor) why = std::string("null ") + noun + " handle";
  if (!why.empty()) return handle_refuse(g_collect_error, entry, why, FLEET_ERR_INVALID);
  FleetMlpHandle* pol = mlp_borrow(actor, sac ? sizeof(QTargetDesc) : sizeof(PolicyDesc), noun, &why);
  if (!pol) return handle_refuse(g_collect_error, entry, why, FLEET_ERR_INVALID);
  const int E = env->d.E, D = env->d.obs_dim, A = env->d.N;
  const PolicyHeadDesc& head = pol->nets[0];
  const int pd = head.layer[0].in;
  const int pa = sac ? static_cast<const QTargetDesc*>(pol->record)->act_dim : head.layer[head.n_layers - 1].out;
  const std::string the = std::string("the ") + noun, whose = sac ? "the networks'" : "the policy's";
  if (!env->d.auto_reset) why = "the env needs auto_reset = 1: a rollout runs across episode ends";
  else if (sac && !qtarget_squashed(pol)) why = "the networks' actor is not a squashed Gaussian: fleet_sac_create makes one";
  else if (pol->device != env->device)
    why = the + (sac ? " lie" : " lies") + " on device " + std::to_string(pol->device) + ", the env on device " + std::to_string(env->device);
  else if (pd != D) why = whose + " obs_dim is " + std::to_string(pd) + ", the env's " + std::to_string(D);
  else if (pa != A) why = whose + " act_dim is " + std::to_string(pa) + ", the env's " + std::to_string(A);
  else if (!sac && pol->n_nets > 1 && pol->nets[1].layer[pol->nets[1].n_layers - 1].out != 1)
    why = "the critic head's output width must be 1, got " + std::to_string(pol->nets[1].layer[pol->nets[1].n_layers - 1].out);
  else if (norm) (void)fleet_norm_check_fit(norm, E, D, env->device, &why);
  if (!why.empty()) return handle_refuse(g_collect_error, entry, why, FLEET_ERR_INVALID);
  FleetCollect* h = new FleetCollect();
  h->env = env, h->norm = norm, h->pol = pol;
  if (sac) h->nets = static_cast<fleet_qtarget_handle>(actor);
  else h->policy = static_cast<fleet_policy_handle>(actor);
  h->E = E, h->D = D, h->A = A, h->W = p->stats_window, h->n_heads = sac ? 0 : pol->n_nets;
  const uint64_t e = (uint64_t)E, od = e * D * 4, w = (uint64_t)h->W;
  const uint64_t bytes[kArrays] = {od, od, norm ? od : 0, norm ? od : 0, od, e * 8, e * 8, e, e, e * A * 4, e * A * 4, e * 4, w * 8, w * 4, 16};
  uint64_t off = 0;
  for (int i = 0; i < kArrays; ++i) h->at[i] = off, off = (off + bytes[i] + 255) / 256 * 256;
  if (!norm) h->at[kRaw0] = h->at[kObs0], h->at[kRaw1] = h->at[kObs1];
  h->bytes = off;
  int rc = FLEET_OK;
  void* q = nullptr;
  if (hipSetDevice(env->device) != hipSuccess) why = "hipSetDevice failed", rc = FLEET_ERR_HIP;
  else if (hipMalloc(&q, off) != hipSuccess) why = "hipMalloc of the collect block's " + std::to_string(off) + " bytes failed", rc = FLEET_ERR_HIP;
  else if (hipMemset(q, 0, off) != hipSuccess || hipDeviceSynchronize() != hipSuccess) why = "clearing the collect block failed", rc = FLEET_ERR_HIP;
  h->block = static_cast<char*>(q);
  if (rc != FLEET_OK) {
    (void)hipGetLastError();
    fleet_collect_destroy(h);
    return handle_refuse(g_collect_error, entry, why, rc);
  }
  *out = h;
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_collect_create(fleet_handle env, fleet_norm_handle norm, fleet_policy_handle policy, const FleetCollectParams* p,
                         fleet_collect_handle* out) {
  return create_on("fleet_collect_create", env, norm, policy, false, p, out);
}

int fleet_saccollect_create(fleet_handle env, fleet_norm_handle norm, fleet_qtarget_handle nets, const FleetCollectParams* p,
                            fleet_collect_handle* out) {
  return create_on("fleet_saccollect_create", env, norm, nets, true, p, out);
}

const char* fleet_saccollect_last_error(fleet_collect_handle h) { return fleet_collect_last_error(h); }

int fleet_saccollect_uniform_dev(fleet_qtarget_handle nets, int E, const FleetSacUniformArgs* x) {
  const std::string why = check_uniform_args(E, x);
  if (const int rc = handle_enter("fleet_saccollect_uniform_dev", why, nets, g_collect_error); rc != FLEET_OK) return rc;
  if (nets->record_bytes != sizeof(QTargetDesc) || !qtarget_squashed(nets)) {
    nets->error = "fleet_saccollect_uniform_dev: the handle's actor is not a squashed Gaussian: fleet_sac_create makes one";
    return FLEET_ERR_INVALID;
  }
  FLEET_HANDLE_TRY(nets, hipSetDevice(nets->device));
  const PolicyUniformArgs u{nullptr, x->actions, nullptr, x->seed, x->step, (uint32_t)x->env_id_offset, 0, x->lo, x->hi};
  FLEET_HANDLE_TRY(nets, policy_launch_uniform(nets->stream, E, nets->desc.act_dim, u));
  return FLEET_OK;
}

int fleet_collect_destroy(fleet_collect_handle h) {
  if (!h) return FLEET_OK;
  if (h->block) {  // (hipFree waits for the device: whatever still reads the block is done)
    (void)hipSetDevice(h->env->device);
    (void)hipFree(h->block);
  }
  delete h;
  return FLEET_OK;
}

const char* fleet_collect_last_error(fleet_collect_handle h) { return h ? h->error.c_str() : g_collect_error.c_str(); }

int fleet_collect_describe(fleet_collect_handle h, FleetCollectInfo* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  out->num_envs = h->E, out->obs_dim = h->D, out->act_dim = h->A, out->stats_window = h->W;
  out->has_norm = h->norm != nullptr, out->cur = h->cur, out->launches = h->launches, out->reserved = 0;
  out->block_bytes = h->bytes;
  for (int s = 0; s < 2; ++s) out->carry_obs[s] = h->obs(s), out->raw_obs[s] = h->raw(s), out->carry_start[s] = h->start(s);
  out->raw_terminal = h->arr<float>(kTerm), out->raw_reward = h->arr<double>(kRawReward), out->reward = h->arr<double>(kReward);
  out->env_actions = h->arr<float>(kEnvAct), out->last_values = h->arr<float>(kLastValues);
  out->ring_return = h->arr<double>(kRingReturn), out->ring_length = h->arr<int32_t>(kRingLength), out->ring_count = h->arr<uint64_t>(kCounts);
  return FLEET_OK;
}

int fleet_collect_reset_dev(fleet_collect_handle h, int clear_episodes) {
  const std::string why = h ? check_streams(h) : "";
  if (const int rc = handle_enter("fleet_collect_reset_dev", why, h, g_collect_error); rc != FLEET_OK) return rc;
  const auto failed = [&](int rc, const char* said) {
    h->error = std::string("fleet_collect_reset_dev: ") + said;
    return rc;
  };
  h->launches = 0;
  if (const int rc = fleet_reset_dev(h->env, nullptr, h->raw(0)); rc != FLEET_OK) return failed(rc, fleet_last_error(h->env));
  h->launches += 1;
  if (h->norm) {
    if (const int rc = fleet_norm_reset_dev(h->norm, h->raw(0), h->obs(0)); rc != FLEET_OK) return failed(rc, fleet_norm_last_error(h->norm));
    h->launches += 1;
  }
  h->cur = 0;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  hipLaunchKernelGGL(collect_fill, dim3(((unsigned)h->E + 255) / 256), dim3(256), 0, h->stream(), h->start(0), h->E, (uint8_t)1);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  h->launches += 1;
  if (clear_episodes) {  // (the ring, its lengths and the counts lie behind one another)
    FLEET_HANDLE_TRY(h, hipMemsetAsync(h->block + h->at[kRingReturn], 0, h->bytes - h->at[kRingReturn], h->stream()));
  }
  return FLEET_OK;
}

int fleet_collect_ppo_dev(fleet_collect_handle h, const FleetCollectPpoArgs* x) {
  std::string why = check_ppo_args(x);
  int K = 0;
  if (h && why.empty() && h->nets) why = kServedBySac;
  else if (h && why.empty()) {
    const RolloutBase* rb = reinterpret_cast<const RolloutBase*>(x->buffer);
    const FleetRolloutLayout& L = rb->L;
    const int E = (int)(L.row_bytes[FLEET_ROLLOUT_REWARDS] / 4);
    K = (int)(L.bytes[FLEET_ROLLOUT_REWARDS] / L.row_bytes[FLEET_ROLLOUT_REWARDS]);
    const int D = (int)(L.row_bytes[FLEET_ROLLOUT_OBS] / L.row_bytes[FLEET_ROLLOUT_REWARDS]);
    const int A = (int)(L.row_bytes[FLEET_ROLLOUT_ACTIONS] / L.row_bytes[FLEET_ROLLOUT_REWARDS]);
    if (h->n_heads < 2) why = "values asked of a policy without a critic head";
    else if (rb->device != h->env->device) why = "the rollout buffer lies on another device than the env";
    else if (E != h->E) why = "the rollout buffer's num_envs is " + std::to_string(E) + ", the env's " + std::to_string(h->E);
    else if (D != h->D) why = "the rollout buffer's obs_dim is " + std::to_string(D) + ", the env's " + std::to_string(h->D);
    else if (A != h->A) why = "the rollout buffer's act_dim is " + std::to_string(A) + ", the env's " + std::to_string(h->A);
    else if (x->n_steps != K) why = "n_steps must be the rollout buffer's " + std::to_string(K) + ", got " + std::to_string(x->n_steps);
    else why = check_streams(h, rb, "rollout buffer");
  }
  if (const int rc = handle_enter("fleet_collect_ppo_dev", why, h, g_collect_error); rc != FLEET_OK) return rc;
  const auto failed = [&](int rc, const char* said) {
    h->error = std::string("fleet_collect_ppo_dev: ") + said;
    return rc;
  };
  h->launches = 0;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  const int cur = h->cur, nxt = cur ^ 1;
  float* env_act = h->arr<float>(kEnvAct);
  double* raw_reward = h->arr<double>(kRawReward);
  double* reward = h->norm ? h->arr<double>(kReward) : raw_reward;
  FleetExploreArgs g{};
  g.struct_bytes = (int32_t)sizeof g;
  g.mode = FLEET_EXPLORE_GAUSSIAN, g.noise_mode = FLEET_EXPLORE_NOISE_DRAW;
  g.seed = x->seed, g.env_id_offset = x->env_id_offset, g.scale = x->log_std, g.env_actions = env_act;
  FleetRolloutSlot row{}, next_row{};
  if (const int rc = fleet_rollout_slot(x->buffer, 0, &row); rc != FLEET_OK) return failed(rc, fleet_rollout_last_error(x->buffer));
  for (int t = 0; t < K; ++t) {
    const float* cur_obs = t ? row.obs : h->obs(cur);
    const uint8_t* cur_start = t ? row.episode_start : h->start(cur);
    if (t + 1 < K) {
      if (const int rc = fleet_rollout_slot(x->buffer, t + 1, &next_row); rc != FLEET_OK) return failed(rc, fleet_rollout_last_error(x->buffer));
    }
    float* next_obs = t + 1 < K ? next_row.obs : h->obs(nxt);
    uint8_t* next_start = t + 1 < K ? next_row.episode_start : h->start(nxt);
    g.step = x->first_step + (uint64_t)t;
    g.actions = row.actions, g.log_prob = row.log_prob, g.values = row.value;
    if (const int rc = fleet_explore_act_dev(h->policy, cur_obs, h->E, nullptr, &g); rc != FLEET_OK) return failed(rc, fleet_policy_last_error(h->policy));
    if (const int rc = fleet_step_dev(h->env, env_act, FLEET_ACT_F32, h->norm ? h->raw(nxt) : next_obs, raw_reward, next_start, nullptr); rc != FLEET_OK)
      return failed(rc, fleet_last_error(h->env));
    h->launches += 2;
    if (h->norm) {
      if (const int rc = fleet_norm_step_dev(h->norm, h->raw(nxt), raw_reward, next_start, nullptr, next_obs, reward, nullptr); rc != FLEET_OK)
        return failed(rc, fleet_norm_last_error(h->norm));
      h->launches += 1;
    }
    if (const int rc = fleet_rollout_add_dev(x->buffer, t, cur_obs, row.actions, reward, FLEET_ACT_F64, cur_start, row.value, row.log_prob, nullptr, nullptr);
        rc != FLEET_OK)
      return failed(rc, fleet_rollout_last_error(x->buffer));
    h->launches += 1;
    if (const int rc = launch_episodes(h, next_start); rc != FLEET_OK) return rc;
    row = next_row;
  }
  h->cur = nxt;
  float* last_values = h->arr<float>(kLastValues);
  if (const int rc = fleet_policy_forward_dev(h->policy, h->obs(nxt), h->E, nullptr, env_act, last_values); rc != FLEET_OK)
    return failed(rc, fleet_policy_last_error(h->policy));
  if (const int rc = fleet_rollout_finish_dev(x->buffer, last_values, h->start(nxt)); rc != FLEET_OK) return failed(rc, fleet_rollout_last_error(x->buffer));
  h->launches += 2;
  return launch_finish(h, x->first_step + (uint64_t)K, x->stats);
}

int fleet_collect_offpolicy_dev(fleet_collect_handle h, const FleetCollectOffpolicyArgs* x) {
  std::string why = check_offpolicy_args(x);
  if (h && why.empty() && h->nets) why = kServedBySac;
  else if (h && why.empty()) {
    FleetNoiseParams np{};
    why = check_replay(h, x->replay);
    if (why.empty() && x->noise) {
      if (fleet_noise_describe(x->noise, &np) != FLEET_OK) why = "the noise handle does not describe itself";
      else if (base_of(x->noise)->device != h->env->device) why = "the noise handle lies on another device than the env";
      else if (np.num_envs != h->E || np.act_dim != h->A)
        why = "the noise handle was made for " + std::to_string(np.num_envs) + " envs x " + std::to_string(np.act_dim) + " actions, the env has " +
              std::to_string(h->E) + " x " + std::to_string(h->A);
      else why = check_streams(h, base_of(x->noise), "noise handle");
    }
  }
  if (const int rc = handle_enter("fleet_collect_offpolicy_dev", why, h, g_collect_error); rc != FLEET_OK) return rc;
  float* act = h->arr<float>(kEnvAct);
  float* eps = h->arr<float>(kEps);
  FleetExploreArgs g{};
  g.struct_bytes = (int32_t)sizeof g;
  g.seed = x->seed, g.env_id_offset = x->env_id_offset, g.scale = x->sigma, g.shift = x->shift;
  g.noise_lo = x->noise_lo, g.noise_hi = x->noise_hi, g.actions = act, g.env_actions = act;
  const auto action = [&](uint64_t s, int cur, const auto& failed) {
    g.step = s;
    if (s < x->learning_starts) {
      g.mode = FLEET_EXPLORE_UNIFORM, g.noise_mode = FLEET_EXPLORE_NOISE_DRAW, g.noise = nullptr;
    } else if (x->noise) {
      if (const int rc = fleet_noise_next_dev(x->noise, h->start(cur), eps); rc != FLEET_OK) return failed(rc, fleet_noise_last_error(x->noise));
      h->launches += 1;
      g.mode = FLEET_EXPLORE_ACTION_NOISE, g.noise_mode = FLEET_EXPLORE_NOISE_GIVEN, g.noise = eps;
    } else {
      g.mode = FLEET_EXPLORE_ACTION_NOISE, g.noise_mode = FLEET_EXPLORE_NOISE_DRAW, g.noise = nullptr;
    }
    if (const int rc = fleet_explore_act_dev(h->policy, h->obs(cur), h->E, nullptr, &g); rc != FLEET_OK) return failed(rc, fleet_policy_last_error(h->policy));
    return (int)FLEET_OK;
  };
  return offpolicy_loop(h, "fleet_collect_offpolicy_dev", x->replay, x->n_steps, x->first_step, x->stats, action);
}

int fleet_saccollect_sac_dev(fleet_collect_handle h, const FleetSacCollectArgs* x) {
  std::string why = check_sac_args(x);
  if (h && why.empty()) why = h->nets ? check_replay(h, x->replay) : std::string(kServedByPolicy);
  if (const int rc = handle_enter("fleet_saccollect_sac_dev", why, h, g_collect_error); rc != FLEET_OK) return rc;
  float* act = h->arr<float>(kEnvAct);
  FleetSacUniformArgs u{};
  u.struct_bytes = (int32_t)sizeof u;
  u.env_id_offset = x->env_id_offset, u.lo = x->noise_lo, u.hi = x->noise_hi, u.seed = x->seed, u.actions = act;
  FleetSacActArgs g{};
  g.struct_bytes = (int32_t)sizeof g;
  g.noise_mode = FLEET_EXPLORE_NOISE_DRAW, g.deterministic = 0, g.env_id_offset = x->env_id_offset, g.seed = x->seed, g.actions = act;
  const auto action = [&](uint64_t s, int cur, const auto& failed) {
    u.step = g.step = s;
    const int rc = s < x->learning_starts ? fleet_saccollect_uniform_dev(h->nets, h->E, &u) : fleet_sac_act_dev(h->nets, h->obs(cur), h->E, nullptr, &g);
    return rc != FLEET_OK ? failed(rc, fleet_sac_last_error(h->nets)) : (int)FLEET_OK;
  };
  return offpolicy_loop(h, "fleet_saccollect_sac_dev", x->replay, x->n_steps, x->first_step, x->stats, action);
}

int fleet_collect_episodes_dev(fleet_collect_handle h, const uint8_t* done, const double* ep_return, const int32_t* ep_len, int E) {
  const std::string why = check_episode_args(done, ep_return, ep_len, E);
  if (const int rc = handle_enter("fleet_collect_episodes_dev", why, h, g_collect_error); rc != FLEET_OK) return rc;
  EpisodeArgs a{};
  a.done = done, a.ep_ret = ep_return, a.ep_len = ep_len;
  a.ring_return = h->arr<double>(kRingReturn), a.ring_length = h->arr<int32_t>(kRingLength), a.counts = h->arr<uint64_t>(kCounts);
  a.E = E, a.W = (uint32_t)h->W;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  hipLaunchKernelGGL(collect_episodes<false>, dim3(1), dim3(kCollectScanThreads), 0, h->stream(), a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

int fleet_collect_finish_dev(fleet_collect_handle h, uint64_t first_step, int32_t steps, double* stats) {
  const std::string why = check_finish_args(steps, stats);
  if (const int rc = handle_enter("fleet_collect_finish_dev", why, h, g_collect_error); rc != FLEET_OK) return rc;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  const int before = h->launches;
  const int rc = launch_finish(h, first_step + (uint64_t)steps, stats);
  h->launches = before;  // (describe reports the run calls')
  return rc;
}

int fleet_collect_episodes_read(fleet_collect_handle h, double* ring_return, int32_t* ring_length, uint64_t* count) {
  if (const int rc = handle_enter("fleet_collect_episodes_read", "", h, g_collect_error); rc != FLEET_OK) return rc;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->env->device));
  const size_t w = (size_t)h->W;
  if (ring_return) FLEET_HANDLE_TRY(h, hipMemcpyAsync(ring_return, h->arr<double>(kRingReturn), w * 8, hipMemcpyDeviceToHost, h->stream()));
  if (ring_length) FLEET_HANDLE_TRY(h, hipMemcpyAsync(ring_length, h->arr<int32_t>(kRingLength), w * 4, hipMemcpyDeviceToHost, h->stream()));
  if (count) FLEET_HANDLE_TRY(h, hipMemcpyAsync(count, h->arr<uint64_t>(kCounts), 8, hipMemcpyDeviceToHost, h->stream()));
  FLEET_HANDLE_TRY(h, hipStreamSynchronize(h->stream()));
  return FLEET_OK;
}

}  // extern "C"
