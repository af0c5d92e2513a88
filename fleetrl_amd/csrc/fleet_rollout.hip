// fleet_rollout.hip -- stable-baselines3 `RolloutBuffer` on the device: the storage a PPO rollout fills, its advantages and returns,
// and the minibatch gather (include/fleet_hip.h "rollout buffer on the device").
//
// One allocation holds the eight [K,E,...] arrays, time-major as in SB3, and one error word.  Three kernels, one launch each; the
// launch boundaries are the only visibility mechanism (no atomics, no LDS, no host synchronisation in any *_dev call):
//   rollout_add     time row t <- the step's tensors: flat copies (16-byte words where the sizes and addresses allow), the reward
//                   rounded once to float32, the optional time-limit bootstrap.  A source that already is the row is not copied.
//   rollout_gae     SB3's compute_returns_and_advantage.  One lane per env, adjacent lanes adjacent envs (every [K,E] access is
//                   coalesced); the recurrence runs backwards in time in SB3's operation order (-ffp-contract=off: bit-identical to
//                   the float32 NumPy restatement).  The chain is serial but its loads are not: a lane issues the loads of
//                   FLEET_GAE_ROWS time rows, and of the block after them, before it consumes the first.
//   rollout_gather  SB3's get() for one minibatch: rows of six arrays picked by flat indices e * K + t, one launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "fleet_handle.h"
#include "fleet_rollout.h"

namespace {

constexpr int kGaeThreads = FLEET_GAE_THREADS;
constexpr int kGaeRows = FLEET_GAE_ROWS;

// ---- rollout_add -------------------------------------------------------------------------------------------------------------
struct AddArgs {
  const float* obs;  // NULL: the row already holds it (every source)
  float* obs_dst;
  const float* act;
  float* act_dst;
  const void* reward;
  float* rew_dst;
  const uint8_t* start;
  uint8_t* start_dst;
  const float* value;
  float* value_dst;
  const float* logp;
  float* logp_dst;
  const float* term_value;  // NULL: no bootstrap
  const uint8_t* done;
  float g;
  int E;
  unsigned n_obs, n_act;    // floats, or 16-byte words when *_vec
  int reward_f64, obs_vec, act_vec;
};

template <typename T>
__device__ inline void copy_flat(const void* src, void* dst, unsigned n, unsigned gid, unsigned stride) {
  const T* s = static_cast<const T*>(src);
  T* d = static_cast<T*>(dst);
  for (unsigned i = gid; i < n; i += stride) d[i] = s[i];
}

__global__ __launch_bounds__(kRolloutThreads) void rollout_add(AddArgs a) {
  const unsigned gid = blockIdx.x * kRolloutThreads + threadIdx.x;
  const unsigned stride = gridDim.x * kRolloutThreads;
  for (unsigned e = gid; e < (unsigned)a.E; e += stride) {
    if (a.reward) {
      float r = a.reward_f64 ? (float)static_cast<const double*>(a.reward)[e] : static_cast<const float*>(a.reward)[e];
      if (a.term_value && a.done[e]) r = r + a.g * a.term_value[e];
      a.rew_dst[e] = r;
    }
    if (a.start) a.start_dst[e] = a.start[e];
    if (a.value) a.value_dst[e] = a.value[e];
    if (a.logp) a.logp_dst[e] = a.logp[e];
  }
  if (a.obs) {
    if (a.obs_vec) copy_flat<float4>(a.obs, a.obs_dst, a.n_obs, gid, stride);
    else copy_flat<float>(a.obs, a.obs_dst, a.n_obs, gid, stride);
  }
  if (a.act) {
    if (a.act_vec) copy_flat<float4>(a.act, a.act_dst, a.n_act, gid, stride);
    else copy_flat<float>(a.act, a.act_dst, a.n_act, gid, stride);
  }
}

// ---- rollout_gae -------------------------------------------------------------------------------------------------------------
struct GaeRows {
  float r[kGaeRows], v[kGaeRows];
  uint8_t s[kGaeRows];
};

// rows t, t-1, ... t-kGaeRows+1 of env e; rows below 0 read row 0 instead (a valid address: no branch around any load) and are
// not consumed
__device__ inline void gae_load(GaeRows& b, const float* __restrict__ rewards, const float* __restrict__ values,
                                const uint8_t* __restrict__ starts, int t, int e, int E) {
#pragma unroll
  for (int u = 0; u < kGaeRows; ++u) {
    const int row = t - u > 0 ? t - u : 0;
    const size_t i = (size_t)row * E + e;
    b.r[u] = rewards[i];
    b.v[u] = values[i];
    b.s[u] = starts[i];
  }
}

__global__ __launch_bounds__(kGaeThreads) void rollout_gae(const float* __restrict__ rewards, const float* __restrict__ values,
                                                           const uint8_t* __restrict__ starts, const float* __restrict__ last_values,
                                                           const uint8_t* __restrict__ dones, float* __restrict__ advantages,
                                                           float* __restrict__ returns, int E, int K, float g, float gl) {
  const int e = blockIdx.x * kGaeThreads + threadIdx.x;
  if (e >= E) return;
  GaeRows cur, nxt;
  int t = K - 1;
  gae_load(cur, rewards, values, starts, t, e, E);
  float nv = last_values[e];
  float nnt = 1.0f - (dones[e] ? 1.0f : 0.0f);
  float last = 0.0f;
  for (; t >= 0; t -= kGaeRows) {
    gae_load(nxt, rewards, values, starts, t - kGaeRows, e, E);  // (past row 0: row 0 again, never consumed)
#pragma unroll
    for (int u = 0; u < kGaeRows; ++u) {
      if (t - u >= 0) {  // uniform over the launch
        const float v = cur.v[u];
        const float delta = (cur.r[u] + (g * nv) * nnt) - v;
        last = delta + (gl * nnt) * last;
        const size_t i = (size_t)(t - u) * E + e;
        advantages[i] = last;
        returns[i] = last + v;
        nv = v;
        nnt = 1.0f - (cur.s[u] ? 1.0f : 0.0f);  // episode_starts[t] is row t-1's "next is terminal"
      }
    }
    cur = nxt;
  }
}

// ---- rollout_gather ----------------------------------------------------------------------------------------------------------
struct GatherArgs {
  const float *obs, *act, *values, *logp, *adv, *ret;
  float *o_obs, *o_act, *o_values, *o_logp, *o_adv, *o_ret;
  const int32_t* idx;
  uint32_t* err;
  unsigned B, E, K, total;  // total = K * E
  unsigned D, A;
  unsigned n_obs, n_act;    // items: B * D (or B * D / 4 when obs_vec), likewise the actions
  int obs_vec, act_vec;
};

// the buffer row (t * E + e) of flat index e * K + t; false (and the error word set) when the index is out of range
__device__ inline bool gather_row(const GatherArgs& a, unsigned b, size_t* row) {
  const unsigned i = (unsigned)a.idx[b];  // (a negative index is a large unsigned one)
  if (i >= a.total) {
    *a.err = 1u;  // every offending lane stores the same constant: no atomic needed
    return false;
  }
  const unsigned e = i / a.K, t = i - e * a.K;
  *row = (size_t)t * a.E + e;
  return true;
}

// items of `per_row` words each: word c of output row b <- word c of the buffer row the index names
template <typename T>
__device__ inline void gather_rows(const GatherArgs& a, const float* src, float* dst, unsigned items, unsigned per_row, unsigned gid,
                                   unsigned stride) {
  const T* s = reinterpret_cast<const T*>(src);
  T* d = reinterpret_cast<T*>(dst);
  for (unsigned i = gid; i < items; i += stride) {
    const unsigned b = i / per_row, c = i - b * per_row;
    size_t row;
    if (gather_row(a, b, &row)) d[i] = s[row * per_row + c];
  }
}

__global__ __launch_bounds__(kRolloutThreads) void rollout_gather(GatherArgs a) {
  const unsigned gid = blockIdx.x * kRolloutThreads + threadIdx.x;
  const unsigned stride = gridDim.x * kRolloutThreads;
  if (a.o_values || a.o_logp || a.o_adv || a.o_ret)
    for (unsigned b = gid; b < a.B; b += stride) {
      size_t row;
      if (!gather_row(a, b, &row)) continue;
      if (a.o_values) a.o_values[b] = a.values[row];
      if (a.o_logp) a.o_logp[b] = a.logp[row];
      if (a.o_adv) a.o_adv[b] = a.adv[row];
      if (a.o_ret) a.o_ret[b] = a.ret[row];
    }
  if (a.o_obs) {
    if (a.obs_vec) gather_rows<float4>(a, a.obs, a.o_obs, a.n_obs, a.D / 4, gid, stride);
    else gather_rows<float>(a, a.obs, a.o_obs, a.n_obs, a.D, gid, stride);
  }
  if (a.o_act) {
    if (a.act_vec) gather_rows<float4>(a, a.act, a.o_act, a.n_act, a.A / 4, gid, stride);
    else gather_rows<float>(a, a.act, a.o_act, a.n_act, a.A, gid, stride);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_rollout_create_error;

// copy_flat and gather_rows count their items in an `unsigned` that advances by the grid's stride: the loop ends only if the last
// item's index plus one stride still fits the counter.  The host refuses, before any launch, a count the widest grid cannot finish.
constexpr uint64_t kRolloutMaxStride = (uint64_t)kRolloutMaxBlocks * kRolloutThreads;
constexpr uint64_t kRolloutMaxItems = ((uint64_t)1 << 32) - kRolloutMaxStride;
static_assert(kRolloutMaxStride < ((uint64_t)1 << 31), "an env counter below 2^31 plus one stride fits 32 bits");
const std::string kRolloutItemsWhy = std::to_string(kRolloutMaxItems) + " (2^32 - " + std::to_string(kRolloutMaxBlocks) + " * " +
                                     std::to_string(kRolloutThreads) + ": a 32-bit item counter advances by up to that stride)";
const std::string kRowItemsError = "num_envs * obs_dim and num_envs * act_dim must be <= " + kRolloutItemsWhy;
const std::string kGatherItemsError =
    "fleet_rollout_gather_dev: batch * obs_dim (act_dim) must be <= " + kRolloutItemsWhy + ": gather in pieces";

const char* validate(const FleetRolloutParams* p) {
  if (!p) return "null FleetRolloutParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetRolloutParams)) return "FleetRolloutParams.struct_bytes does not match this library";
  if (p->num_envs < 1) return "num_envs must be >= 1";
  if (p->n_steps < 1) return "n_steps must be >= 1";
  if (p->obs_dim < 1) return "obs_dim must be >= 1";
  if (p->act_dim < 1) return "act_dim must be >= 1";
  if ((uint64_t)p->num_envs * (uint64_t)p->n_steps >= ((uint64_t)1 << 31)) return "num_envs * n_steps must be < 2^31 (flat indices are int32)";
  if ((uint64_t)p->num_envs * (uint64_t)(p->obs_dim > p->act_dim ? p->obs_dim : p->act_dim) > kRolloutMaxItems)
    return kRowItemsError.c_str();
  if (!(p->gamma >= 0 && p->gamma <= 1)) return "gamma must be in [0, 1]";
  if (!(p->gae_lambda >= 0 && p->gae_lambda <= 1)) return "gae_lambda must be in [0, 1]";
  return nullptr;
}

void layout_of(const FleetRolloutParams* p, FleetRolloutLayout* L) {
  const uint64_t E = p->num_envs, K = p->n_steps, D = p->obs_dim, A = p->act_dim;
  const uint64_t row[FLEET_ROLLOUT_ARRAYS] = {E * D * 4, E * A * 4, E * 4, E, E * 4, E * 4, E * 4, E * 4};
  *L = FleetRolloutLayout{};
  L->struct_bytes = (int32_t)sizeof(FleetRolloutLayout);
  L->alignment = FLEET_ROLLOUT_ALIGN;
  handle_layout(row, FLEET_ROLLOUT_ARRAYS, K, FLEET_ROLLOUT_ALIGN, L->offset, L->bytes, L->row_bytes, &L->error_offset, &L->total_bytes);
}

}  // namespace

// block: the eight arrays, then the error word
struct FleetRollout : FleetBufferBase<FleetRolloutLayout> {
  FleetRolloutParams p{};
  int E = 0, K = 0, D = 0, A = 0;
  float g = 0.f, gl = 0.f;
};

extern "C" {

int fleet_rollout_layout(const FleetRolloutParams* p, FleetRolloutLayout* out) {
  const char* why = validate(p);
  if (!why && !out) why = "null FleetRolloutLayout";
  if (why) {
    g_rollout_create_error = why;
    return FLEET_ERR_INVALID;
  }
  layout_of(p, out);
  return FLEET_OK;
}

int fleet_rollout_create(int device, const FleetRolloutParams* p, fleet_rollout_handle* out) {
  if (out) *out = nullptr;
  const char* why = validate(p);  // before the device is touched
  if (!why && !out) why = "null output handle";
  if (why) {
    g_rollout_create_error = why;
    return FLEET_ERR_INVALID;
  }
  FleetRollout* r = new FleetRollout();
  r->p = *p;
  r->E = p->num_envs, r->K = p->n_steps, r->D = p->obs_dim, r->A = p->act_dim;
  r->g = (float)p->gamma;
  r->gl = (float)(p->gamma * p->gae_lambda);  // the product in float64 first, as Python forms it
  layout_of(p, &r->L);
  const int rc = handle_open_buffer(r, device, "rollout buffer", &g_rollout_create_error);
  if (rc != FLEET_OK) {
    fleet_rollout_destroy(r);
    return rc;
  }
  *out = r;
  return FLEET_OK;
}

int fleet_rollout_destroy(fleet_rollout_handle r) {
  if (!r) return FLEET_OK;
  handle_close(r);
  delete r;
  return FLEET_OK;
}

const char* fleet_rollout_last_error(fleet_rollout_handle r) { return r ? r->error.c_str() : g_rollout_create_error.c_str(); }

int fleet_rollout_set_stream(fleet_rollout_handle r, void* hip_stream) { return r ? handle_set_stream(r, hip_stream) : FLEET_ERR_INVALID; }

int fleet_rollout_arrays(fleet_rollout_handle r, FleetRolloutArrays* out) {
  if (!r || !out) return FLEET_ERR_INVALID;
  out->obs = r->array<float>(FLEET_ROLLOUT_OBS);
  out->actions = r->array<float>(FLEET_ROLLOUT_ACTIONS);
  out->rewards = r->array<float>(FLEET_ROLLOUT_REWARDS);
  out->episode_starts = r->array<uint8_t>(FLEET_ROLLOUT_EPISODE_STARTS);
  out->values = r->array<float>(FLEET_ROLLOUT_VALUES);
  out->log_probs = r->array<float>(FLEET_ROLLOUT_LOG_PROBS);
  out->advantages = r->array<float>(FLEET_ROLLOUT_ADVANTAGES);
  out->returns = r->array<float>(FLEET_ROLLOUT_RETURNS);
  return FLEET_OK;
}

int fleet_rollout_slot(fleet_rollout_handle r, int t, FleetRolloutSlot* out) {
  if (!r) return FLEET_ERR_INVALID;
  if (!out || t < 0 || t >= r->K) {
    r->error = "fleet_rollout_slot: t must be in [0, n_steps) and the output non-null";
    return FLEET_ERR_INVALID;
  }
  out->obs = r->array<float>(FLEET_ROLLOUT_OBS, t);
  out->actions = r->array<float>(FLEET_ROLLOUT_ACTIONS, t);
  out->reward = r->array<float>(FLEET_ROLLOUT_REWARDS, t);
  out->episode_start = r->array<uint8_t>(FLEET_ROLLOUT_EPISODE_STARTS, t);
  out->value = r->array<float>(FLEET_ROLLOUT_VALUES, t);
  out->log_prob = r->array<float>(FLEET_ROLLOUT_LOG_PROBS, t);
  return FLEET_OK;
}

int fleet_rollout_add_dev(fleet_rollout_handle r, int t, const float* obs, const float* actions, const void* reward, int reward_dtype,
                          const uint8_t* episode_start, const float* value, const float* log_prob, const float* terminal_value,
                          const uint8_t* done) {
  if (!r) return FLEET_ERR_INVALID;
  if (t < 0 || t >= r->K) {
    r->error = "fleet_rollout_add_dev: t must be in [0, n_steps)";
    return FLEET_ERR_INVALID;
  }
  if (!obs || !actions || !reward || !episode_start || !value || !log_prob) {
    r->error = "fleet_rollout_add_dev: null source (pass the row's own address, fleet_rollout_slot, for an array written in place)";
    return FLEET_ERR_INVALID;
  }
  if (reward_dtype != FLEET_ACT_F32 && reward_dtype != FLEET_ACT_F64) {
    r->error = "fleet_rollout_add_dev: reward_dtype must be FLEET_ACT_F32 or FLEET_ACT_F64";
    return FLEET_ERR_INVALID;
  }
  if (terminal_value && !done) {
    r->error = "fleet_rollout_add_dev: terminal_value needs the step's dones";
    return FLEET_ERR_INVALID;
  }
  FleetRolloutSlot s;
  fleet_rollout_slot(r, t, &s);
  if (reward == s.reward && reward_dtype != FLEET_ACT_F32) {
    r->error = "fleet_rollout_add_dev: the row's own reward address holds float32";
    return FLEET_ERR_INVALID;
  }
  AddArgs a{};
  a.E = r->E;
  a.g = r->g;
  a.obs = obs == s.obs ? nullptr : obs;
  a.obs_dst = s.obs;
  a.act = actions == s.actions ? nullptr : actions;
  a.act_dst = s.actions;
  a.reward = (reward == s.reward && !terminal_value) ? nullptr : reward;
  a.rew_dst = s.reward;
  a.reward_f64 = reward_dtype == FLEET_ACT_F64;
  a.start = episode_start == s.episode_start ? nullptr : episode_start;
  a.start_dst = s.episode_start;
  a.value = value == s.value ? nullptr : value;
  a.value_dst = s.value;
  a.logp = log_prob == s.log_prob ? nullptr : log_prob;
  a.logp_dst = s.log_prob;
  a.term_value = terminal_value;
  a.done = done;
  const size_t n_obs = (size_t)r->E * r->D, n_act = (size_t)r->E * r->A;
  a.obs_vec = n_obs % 4 == 0 && aligned16(obs) && aligned16(s.obs);
  a.act_vec = n_act % 4 == 0 && aligned16(actions) && aligned16(s.actions);
  a.n_obs = (unsigned)(a.obs_vec ? n_obs / 4 : n_obs);
  a.n_act = (unsigned)(a.act_vec ? n_act / 4 : n_act);
  size_t items = (size_t)r->E;
  if (a.obs && a.n_obs > items) items = a.n_obs;
  if (a.act && a.n_act > items) items = a.n_act;
  FLEET_HANDLE_TRY(r, hipSetDevice(r->device));
  hipLaunchKernelGGL(rollout_add, dim3(grid_for(items, kRolloutThreads, kRolloutMaxBlocks)), dim3(kRolloutThreads), 0, r->stream, a);
  FLEET_HANDLE_TRY(r, hipGetLastError());
  return FLEET_OK;
}

int fleet_rollout_finish_dev(fleet_rollout_handle r, const float* last_values, const uint8_t* dones) {
  if (!r) return FLEET_ERR_INVALID;
  if (!last_values || !dones) {
    r->error = "fleet_rollout_finish_dev: null buffer";
    return FLEET_ERR_INVALID;
  }
  FLEET_HANDLE_TRY(r, hipSetDevice(r->device));
  hipLaunchKernelGGL(rollout_gae, dim3((r->E + kGaeThreads - 1) / kGaeThreads), dim3(kGaeThreads), 0, r->stream,
                     r->array<float>(FLEET_ROLLOUT_REWARDS), r->array<float>(FLEET_ROLLOUT_VALUES),
                     r->array<uint8_t>(FLEET_ROLLOUT_EPISODE_STARTS), last_values, dones, r->array<float>(FLEET_ROLLOUT_ADVANTAGES),
                     r->array<float>(FLEET_ROLLOUT_RETURNS), r->E, r->K, r->g, r->gl);
  FLEET_HANDLE_TRY(r, hipGetLastError());
  return FLEET_OK;
}

int fleet_rollout_gather_dev(fleet_rollout_handle r, const int32_t* indices, int batch, float* out_obs, float* out_actions,
                             float* out_values, float* out_log_probs, float* out_advantages, float* out_returns) {
  if (!r) return FLEET_ERR_INVALID;
  if (!indices || batch < 0) {
    r->error = "fleet_rollout_gather_dev: null indices or negative batch";
    return FLEET_ERR_INVALID;
  }
  const size_t n_obs = (size_t)batch * r->D, n_act = (size_t)batch * r->A;
  if ((out_obs && n_obs > kRolloutMaxItems) || (out_actions && n_act > kRolloutMaxItems)) {
    r->error = kGatherItemsError;
    return FLEET_ERR_INVALID;
  }
  if (batch == 0) return FLEET_OK;
  GatherArgs a{};
  a.obs = r->array<float>(FLEET_ROLLOUT_OBS), a.act = r->array<float>(FLEET_ROLLOUT_ACTIONS);
  a.values = r->array<float>(FLEET_ROLLOUT_VALUES), a.logp = r->array<float>(FLEET_ROLLOUT_LOG_PROBS);
  a.adv = r->array<float>(FLEET_ROLLOUT_ADVANTAGES), a.ret = r->array<float>(FLEET_ROLLOUT_RETURNS);
  a.o_obs = out_obs, a.o_act = out_actions, a.o_values = out_values, a.o_logp = out_log_probs, a.o_adv = out_advantages;
  a.o_ret = out_returns;
  a.idx = indices;
  a.err = r->err;
  a.B = (unsigned)batch, a.E = (unsigned)r->E, a.K = (unsigned)r->K, a.total = (unsigned)r->E * (unsigned)r->K;
  a.D = (unsigned)r->D, a.A = (unsigned)r->A;
  a.obs_vec = r->D % 4 == 0 && aligned16(out_obs);  // (the buffer's rows then start at multiples of 16 bytes too)
  a.act_vec = r->A % 4 == 0 && aligned16(out_actions);
  a.n_obs = (unsigned)(a.obs_vec ? n_obs / 4 : n_obs);
  a.n_act = (unsigned)(a.act_vec ? n_act / 4 : n_act);
  size_t items = (size_t)batch;
  if (out_obs && a.n_obs > items) items = a.n_obs;
  if (out_actions && a.n_act > items) items = a.n_act;
  FLEET_HANDLE_TRY(r, hipSetDevice(r->device));
  hipLaunchKernelGGL(rollout_gather, dim3(grid_for(items, kRolloutThreads, kRolloutMaxBlocks)), dim3(kRolloutThreads), 0, r->stream, a);
  FLEET_HANDLE_TRY(r, hipGetLastError());
  return FLEET_OK;
}

int fleet_rollout_check_errors(fleet_rollout_handle r) {
  if (!r) return FLEET_ERR_INVALID;
  return handle_check_errors(r, "a gather met an index outside [0, n_steps * num_envs): its output rows were left untouched");
}

}  // extern "C"
