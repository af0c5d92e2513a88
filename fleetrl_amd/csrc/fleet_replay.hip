// fleet_replay.hip -- stable-baselines3 `ReplayBuffer` on the device: the ring an off-policy algorithm (TD3, DDPG, SAC) fills and
// the minibatch it samples (include/fleet_hip.h "replay buffer on the device").
//
// One allocation holds the six [R,E,...] arrays and one error word.  Two kernels, one launch each; the launch boundaries are the
// only visibility mechanism (no atomics, no host synchronisation in any *_dev call):
//   replay_add     ring row pos <- the step's tensors.  One wavefront per env row: the done flag that selects between the step's
//                  output and the terminal observation is uniform over the wavefront, and no item needs a division to find its
//                  row.  The observations are COPIED (16-byte words where the sizes and addresses allow): a row written in place
//                  would, in a ring, corrupt the oldest transition until the next add.
//   replay_sample  one wavefront per sample: the index pair (loaded, or drawn with one Philox4x32-10 block) is uniform over the
//                  wavefront, the lanes take the row's 16-byte words.  The observations and the reward are stored raw and
//                  normalised here, with the normaliser's arithmetic (fleet_norm.h) and its statistics as they are when the
//                  launch runs; mean[D] and sd[D] are staged once per workgroup into the LDS.  Outputs are written once and read
//                  by other kernels next: plain stores.
// Offsets into the two observation arrays are 64-bit: R * E * D passes 2^31 at sizes people ask for.
#include <hip/hip_runtime.h>

#include <string>

#include "fleet_handle.h"
#include "fleet_norm.h"
#include "fleet_philox.h"
#include "fleet_replay.h"

namespace {

// the words [lane, lane + 64, ...) of a row of n floats; kVec: n % 4 == 0 and both addresses 16-byte aligned
__device__ inline void copy_row(const float* __restrict__ s, float* __restrict__ d, int n, bool vec, int lane) {
  if (vec) {
    const float4* s4 = reinterpret_cast<const float4*>(s);
    float4* d4 = reinterpret_cast<float4*>(d);
    for (int i = lane; i < n / 4; i += 64) d4[i] = s4[i];
  } else {
    for (int i = lane; i < n; i += 64) d[i] = s[i];
  }
}

// ---- replay_add ----------------------------------------------------------------------------------------------------------------
struct AddArgs {
  const float *obs, *next, *term, *act;  // term NULL: no substitution
  const void* reward;
  const uint8_t *done, *timeout;         // timeout NULL: zeros
  float *obs_dst, *next_dst, *act_dst, *rew_dst;
  uint8_t *done_dst, *tmo_dst;
  int E, D, A;
  int reward_f64, obs_vec, next_vec, act_vec;
};

__global__ __launch_bounds__(kReplayThreads) void replay_add(AddArgs a) {
  const unsigned gid = blockIdx.x * kReplayThreads + threadIdx.x;
  const unsigned stride = gridDim.x * kReplayThreads;
  for (unsigned e = gid; e < (unsigned)a.E; e += stride) {
    a.rew_dst[e] = a.reward_f64 ? (float)static_cast<const double*>(a.reward)[e] : static_cast<const float*>(a.reward)[e];
    a.done_dst[e] = a.done[e] != 0;
    a.tmo_dst[e] = a.timeout ? a.timeout[e] : (uint8_t)0;
  }
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int e = blockIdx.x * kReplayWaves + w; e < a.E; e += gridDim.x * kReplayWaves) {
    const size_t o = (size_t)e * a.D;
    copy_row(a.obs + o, a.obs_dst + o, a.D, a.obs_vec, lane);
    // the terminal row of an env that is not done is stale: never read
    const float* nsrc = (a.term && a.done[e]) ? a.term : a.next;
    copy_row(nsrc + o, a.next_dst + o, a.D, a.next_vec, lane);
    const size_t oa = (size_t)e * a.A;
    copy_row(a.act + oa, a.act_dst + oa, a.A, a.act_vec, lane);
  }
}

// ---- replay_sample -------------------------------------------------------------------------------------------------------------
struct SampleArgs {
  const float *obs, *next, *act, *rew;
  const uint8_t *done, *tmo;
  float *o_obs, *o_next, *o_act, *o_done, *o_rew;
  const int32_t *rows, *envs;      // explicit indices, or both NULL: drawn
  int32_t *out_rows, *out_envs;    // what was drawn (or NULL)
  uint32_t* err;
  const double *mean, *sd, *ret_stat;  // the normaliser's device block (NULL: raw)
  double clip_obs, clip_reward;
  uint64_t seed, call;
  unsigned B, E, upper;
  int D, A;
  int norm_obs, norm_reward, obs_vec, act_vec;
};

// one row of D floats, normalised column by column when kNorm; mean / sd in the LDS or in global memory
template <bool kNorm>
__device__ inline void sample_row(const float* __restrict__ s, float* __restrict__ d, int D, bool vec, int lane,
                                  const double* mean, const double* sd, double c) {
  if (vec) {
    const float4* s4 = reinterpret_cast<const float4*>(s);
    float4* d4 = reinterpret_cast<float4*>(d);
    for (int i = lane; i < D / 4; i += 64) {
      float4 x = s4[i];
      if (kNorm) {
        const double* m = mean + 4 * i;
        const double* q = sd + 4 * i;
        x = make_float4(fleet_norm_obs1(x.x, m[0], q[0], c), fleet_norm_obs1(x.y, m[1], q[1], c), fleet_norm_obs1(x.z, m[2], q[2], c),
                        fleet_norm_obs1(x.w, m[3], q[3], c));
      }
      d4[i] = x;
    }
  } else {
    for (int i = lane; i < D; i += 64) d[i] = kNorm ? fleet_norm_obs1(s[i], mean[i], sd[i], c) : s[i];
  }
}

template <bool kNorm, bool kLds>
__global__ __launch_bounds__(kReplayThreads) void replay_sample(SampleArgs a) {
  extern __shared__ double stats[];  // kLds: mean[D], sd[D]
  if (kNorm && kLds) {
    for (int i = threadIdx.x; i < a.D; i += kReplayThreads) {
      stats[i] = a.mean[i];
      stats[a.D + i] = a.sd[i];
    }
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (unsigned b = blockIdx.x * kReplayWaves + w; b < a.B; b += gridDim.x * kReplayWaves) {
    unsigned row, env;
    if (a.rows) {
      row = (unsigned)a.rows[b];  // (a negative index is a large unsigned one)
      env = (unsigned)a.envs[b];
      if (row >= a.upper || env >= a.E) {
        if (lane == 0) *a.err = 1u;  // every offender stores the same constant: no atomic needed
        continue;
      }
    } else {
      uint32_t x[4];
      philox4x32_10(b, 0u, (uint32_t)a.call, (uint32_t)(a.call >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32), x);
      row = (unsigned)__umul64hi((uint64_t)x[0] | ((uint64_t)x[1] << 32), (uint64_t)a.upper);
      env = (unsigned)__umul64hi((uint64_t)x[2] | ((uint64_t)x[3] << 32), (uint64_t)a.E);
      if (lane == 0) {
        if (a.out_rows) a.out_rows[b] = (int32_t)row;
        if (a.out_envs) a.out_envs[b] = (int32_t)env;
      }
    }
    const size_t t = (size_t)row * a.E + env;  // < 2^31
    const size_t src = t * (size_t)a.D, dst = (size_t)b * (size_t)a.D;
    const double* mean = kLds ? stats : a.mean;
    const double* sd = kLds ? stats + a.D : a.sd;
    if (a.o_obs) sample_row<kNorm>(a.obs + src, a.o_obs + dst, a.D, a.obs_vec, lane, mean, sd, a.clip_obs);
    if (a.o_next) sample_row<kNorm>(a.next + src, a.o_next + dst, a.D, a.obs_vec, lane, mean, sd, a.clip_obs);
    if (a.o_act) copy_row(a.act + t * (size_t)a.A, a.o_act + (size_t)b * (size_t)a.A, a.A, a.act_vec, lane);
    if (lane == 0) {
      if (a.o_done) a.o_done[b] = (float)a.done[t] * (1.0f - (float)a.tmo[t]);
      if (a.o_rew) {
        const float r = a.rew[t];
        a.o_rew[b] = a.norm_reward ? (float)fleet_norm_reward1((double)r, a.ret_stat[2], a.clip_reward) : r;
      }
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_replay_create_error;

// replay_add walks the env rows, and copy_row / sample_row the words of a row, with an `int` that advances by a fixed stride: the
// loop ends only if the last index plus one stride still fits the counter.  Create refuses what the widest grid cannot finish.
constexpr int64_t kReplayLaneStride = kReplayThreads / kReplayWaves;  // the lanes of a wavefront
constexpr int64_t kReplayMaxEnvStride = (int64_t)kReplayMaxBlocks * kReplayWaves;
constexpr int64_t kReplayMaxEnvs = ((int64_t)1 << 31) - kReplayMaxEnvStride;
constexpr int64_t kReplayMaxDim = ((int64_t)1 << 31) - kReplayLaneStride;
static_assert(kReplayMaxEnvs > 0 && kReplayMaxDim > 0, "a stride that leaves no size to accept");
const std::string kEnvsError = "num_envs must be <= " + std::to_string(kReplayMaxEnvs) + " (2^31 - " + std::to_string(kReplayMaxBlocks) +
                               " * " + std::to_string(kReplayWaves) + ": a 32-bit env counter advances by up to that stride)";
const std::string kDimWhy = std::to_string(kReplayMaxDim) + " (2^31 - " + std::to_string(kReplayLaneStride) +
                            ": a 32-bit column counter advances by that stride)";
const std::string kObsDimError = "obs_dim must be <= " + kDimWhy;
const std::string kActDimError = "act_dim must be <= " + kDimWhy;

uint64_t rows_of(const FleetReplayParams* p) {
  const uint64_t R = (uint64_t)p->buffer_size / (uint64_t)p->num_envs;
  return R < 1 ? 1 : R;  // SB3: max(buffer_size // n_envs, 1)
}

const char* validate(const FleetReplayParams* p) {
  if (!p) return "null FleetReplayParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetReplayParams)) return "FleetReplayParams.struct_bytes does not match this library";
  if (p->num_envs < 1) return "num_envs must be >= 1";
  if (p->buffer_size < 1) return "buffer_size must be >= 1";
  if (p->obs_dim < 1) return "obs_dim must be >= 1";
  if (p->act_dim < 1) return "act_dim must be >= 1";
  if (p->num_envs > kReplayMaxEnvs) return kEnvsError.c_str();
  if (p->obs_dim > kReplayMaxDim) return kObsDimError.c_str();
  if (p->act_dim > kReplayMaxDim) return kActDimError.c_str();
  if (rows_of(p) * (uint64_t)p->num_envs >= ((uint64_t)1 << 31))
    return "rows * num_envs (rows = max(buffer_size / num_envs, 1)) must be < 2^31 (transition indices are int32)";
  return nullptr;
}

void layout_of(const FleetReplayParams* p, FleetReplayLayout* L) {
  const uint64_t E = p->num_envs, R = rows_of(p), D = p->obs_dim, A = p->act_dim;
  const uint64_t row[FLEET_REPLAY_ARRAYS] = {E * D * 4, E * D * 4, E * A * 4, E * 4, E, E};
  *L = FleetReplayLayout{};
  L->struct_bytes = (int32_t)sizeof(FleetReplayLayout);
  L->alignment = FLEET_REPLAY_ALIGN;
  L->rows = (int32_t)R;
  handle_layout(row, FLEET_REPLAY_ARRAYS, R, FLEET_REPLAY_ALIGN, L->offset, L->bytes, L->row_bytes, &L->error_offset, &L->total_bytes);
}

}  // namespace

// block: the six arrays, then the error word
struct FleetReplay : FleetBufferBase<FleetReplayLayout> {
  FleetReplayParams p{};
  int E = 0, R = 0, D = 0, A = 0;
  int pos = 0;
  bool full = false;
  uint64_t calls = 0;  // minibatches drawn so far: the high half of the Philox counter
};

namespace {

// the launch both index sources share; `rows` NULL: drawn with call number `call`
int launch_sample(FleetReplay* r, const char* who, const int32_t* rows, const int32_t* envs, uint64_t call, int batch,
                  fleet_norm_handle norm, float* out_obs, float* out_actions, float* out_next_obs, float* out_dones,
                  float* out_rewards, int32_t* out_rows, int32_t* out_envs) {
  SampleArgs a{};
  a.obs = r->array<float>(FLEET_REPLAY_OBS), a.next = r->array<float>(FLEET_REPLAY_NEXT_OBS);
  a.act = r->array<float>(FLEET_REPLAY_ACTIONS), a.rew = r->array<float>(FLEET_REPLAY_REWARDS);
  a.done = r->array<uint8_t>(FLEET_REPLAY_DONES), a.tmo = r->array<uint8_t>(FLEET_REPLAY_TIMEOUTS);
  a.o_obs = out_obs, a.o_next = out_next_obs, a.o_act = out_actions, a.o_done = out_dones, a.o_rew = out_rewards;
  a.rows = rows, a.envs = envs, a.out_rows = out_rows, a.out_envs = out_envs;
  a.err = r->err;
  a.seed = r->p.seed, a.call = call;
  a.B = (unsigned)batch, a.E = (unsigned)r->E, a.upper = (unsigned)(r->full ? r->R : r->pos);
  a.D = r->D, a.A = r->A;
  // (the buffer's rows start at multiples of 16 bytes when D % 4 == 0: the arrays are 256-byte aligned)
  a.obs_vec = r->D % 4 == 0 && aligned16(out_obs) && aligned16(out_next_obs);
  a.act_vec = r->A % 4 == 0 && aligned16(out_actions);
  FLEET_HANDLE_TRY(r, hipSetDevice(r->device));
  bool norm_obs = false;
  if (norm) {
    FleetNormView v{};
    FLEET_HANDLE_TRY(r, fleet_norm_begin_read(norm, r->stream, &v));
    if (v.D != r->D || v.device != r->device) {
      r->error = std::string(who) + ": the normaliser has obs_dim " + std::to_string(v.D) + " on device " + std::to_string(v.device) +
                 ", the buffer " + std::to_string(r->D) + " on device " + std::to_string(r->device);
      return FLEET_ERR_INVALID;
    }
    a.mean = v.obs_mean, a.sd = v.obs_sd, a.ret_stat = v.ret_stat;
    a.clip_obs = v.clip_obs, a.clip_reward = v.clip_reward;
    a.norm_obs = v.norm_obs, a.norm_reward = v.norm_reward;
    norm_obs = v.norm_obs && (out_obs || out_next_obs);
  }
  const size_t lds = norm_obs ? (size_t)r->D * 16 : 0;
  const bool use_lds = lds > 0 && lds <= kReplayLdsBytes;
  const dim3 grid(grid_for((size_t)batch, kReplayWaves, kReplayMaxBlocks)), block(kReplayThreads);
  if (!norm_obs) hipLaunchKernelGGL((replay_sample<false, false>), grid, block, 0, r->stream, a);
  else if (use_lds) hipLaunchKernelGGL((replay_sample<true, true>), grid, block, lds, r->stream, a);
  else hipLaunchKernelGGL((replay_sample<true, false>), grid, block, 0, r->stream, a);
  FLEET_HANDLE_TRY(r, hipGetLastError());
  if (norm) FLEET_HANDLE_TRY(r, fleet_norm_end_read(norm, r->stream));
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_replay_layout(const FleetReplayParams* p, FleetReplayLayout* out) {
  const char* why = validate(p);
  if (!why && !out) why = "null FleetReplayLayout";
  if (why) {
    g_replay_create_error = why;
    return FLEET_ERR_INVALID;
  }
  layout_of(p, out);
  return FLEET_OK;
}

int fleet_replay_create(int device, const FleetReplayParams* p, fleet_replay_handle* out) {
  if (out) *out = nullptr;
  const char* why = validate(p);  // before the device is touched
  if (!why && !out) why = "null output handle";
  if (why) {
    g_replay_create_error = why;
    return FLEET_ERR_INVALID;
  }
  FleetReplay* r = new FleetReplay();
  r->p = *p;
  r->E = p->num_envs, r->R = (int)rows_of(p), r->D = p->obs_dim, r->A = p->act_dim;
  layout_of(p, &r->L);
  const int rc = handle_open_buffer(r, device, "replay buffer", &g_replay_create_error);
  if (rc != FLEET_OK) {
    fleet_replay_destroy(r);
    return rc;
  }
  *out = r;
  return FLEET_OK;
}

int fleet_replay_destroy(fleet_replay_handle r) {
  if (!r) return FLEET_OK;
  handle_close(r);
  delete r;
  return FLEET_OK;
}

const char* fleet_replay_last_error(fleet_replay_handle r) { return r ? r->error.c_str() : g_replay_create_error.c_str(); }

int fleet_replay_set_stream(fleet_replay_handle r, void* hip_stream) { return r ? handle_set_stream(r, hip_stream) : FLEET_ERR_INVALID; }

int fleet_replay_arrays(fleet_replay_handle r, FleetReplayArrays* out) {
  if (!r || !out) return FLEET_ERR_INVALID;
  out->observations = r->array<float>(FLEET_REPLAY_OBS);
  out->next_observations = r->array<float>(FLEET_REPLAY_NEXT_OBS);
  out->actions = r->array<float>(FLEET_REPLAY_ACTIONS);
  out->rewards = r->array<float>(FLEET_REPLAY_REWARDS);
  out->dones = r->array<uint8_t>(FLEET_REPLAY_DONES);
  out->timeouts = r->array<uint8_t>(FLEET_REPLAY_TIMEOUTS);
  return FLEET_OK;
}

int fleet_replay_add_dev(fleet_replay_handle r, const float* obs, const float* next_obs, const float* action, const void* reward,
                         int reward_dtype, const uint8_t* done, const float* terminal, const uint8_t* timeout) {
  if (!r) return FLEET_ERR_INVALID;
  if (!obs || !next_obs || !action || !reward || !done) {
    r->error = "fleet_replay_add_dev: null source (only terminal and timeout may be NULL)";
    return FLEET_ERR_INVALID;
  }
  if (reward_dtype != FLEET_ACT_F32 && reward_dtype != FLEET_ACT_F64) {
    r->error = "fleet_replay_add_dev: reward_dtype must be FLEET_ACT_F32 or FLEET_ACT_F64";
    return FLEET_ERR_INVALID;
  }
  AddArgs a{};
  a.obs = obs, a.next = next_obs, a.term = terminal, a.act = action, a.reward = reward, a.done = done, a.timeout = timeout;
  a.obs_dst = r->array<float>(FLEET_REPLAY_OBS, r->pos), a.next_dst = r->array<float>(FLEET_REPLAY_NEXT_OBS, r->pos);
  a.act_dst = r->array<float>(FLEET_REPLAY_ACTIONS, r->pos), a.rew_dst = r->array<float>(FLEET_REPLAY_REWARDS, r->pos);
  a.done_dst = r->array<uint8_t>(FLEET_REPLAY_DONES, r->pos), a.tmo_dst = r->array<uint8_t>(FLEET_REPLAY_TIMEOUTS, r->pos);
  a.E = r->E, a.D = r->D, a.A = r->A;
  a.reward_f64 = reward_dtype == FLEET_ACT_F64;
  // (the destination rows start at multiples of 16 bytes when D % 4 == 0, resp. A % 4 == 0)
  a.obs_vec = r->D % 4 == 0 && aligned16(obs);
  a.next_vec = r->D % 4 == 0 && aligned16(next_obs) && aligned16(terminal);
  a.act_vec = r->A % 4 == 0 && aligned16(action);
  FLEET_HANDLE_TRY(r, hipSetDevice(r->device));
  hipLaunchKernelGGL(replay_add, dim3(grid_for((size_t)r->E, kReplayWaves, kReplayMaxBlocks)), dim3(kReplayThreads), 0, r->stream, a);
  FLEET_HANDLE_TRY(r, hipGetLastError());
  if (++r->pos == r->R) {
    r->pos = 0;
    r->full = true;
  }
  return FLEET_OK;
}

int fleet_replay_gather_dev(fleet_replay_handle r, const int32_t* rows, const int32_t* envs, int batch, fleet_norm_handle norm,
                            float* out_obs, float* out_actions, float* out_next_obs, float* out_dones, float* out_rewards) {
  if (!r) return FLEET_ERR_INVALID;
  if (!rows || !envs || batch < 0) {
    r->error = "fleet_replay_gather_dev: null indices or negative batch";
    return FLEET_ERR_INVALID;
  }
  if (batch == 0) return FLEET_OK;
  return launch_sample(r, "fleet_replay_gather_dev", rows, envs, 0, batch, norm, out_obs, out_actions, out_next_obs, out_dones,
                       out_rewards, nullptr, nullptr);
}

int fleet_replay_sample_dev(fleet_replay_handle r, int batch, fleet_norm_handle norm, float* out_obs, float* out_actions,
                            float* out_next_obs, float* out_dones, float* out_rewards, int32_t* out_rows, int32_t* out_envs) {
  if (!r) return FLEET_ERR_INVALID;
  if (batch < 0) {
    r->error = "fleet_replay_sample_dev: negative batch";
    return FLEET_ERR_INVALID;
  }
  if (!r->full && r->pos == 0) {
    r->error = "fleet_replay_sample_dev: the buffer is empty";
    return FLEET_ERR_STATE;
  }
  if (batch > 0) {
    const int rc = launch_sample(r, "fleet_replay_sample_dev", nullptr, nullptr, r->calls, batch, norm, out_obs, out_actions,
                                 out_next_obs, out_dones, out_rewards, out_rows, out_envs);
    if (rc != FLEET_OK) return rc;
  }
  r->calls += 1;
  return FLEET_OK;
}

int fleet_replay_check_errors(fleet_replay_handle r) {
  if (!r) return FLEET_ERR_INVALID;
  return handle_check_errors(r, "a gather met an index pair outside [0, rows filled) x [0, num_envs): its sample was left untouched");
}

int fleet_replay_size(fleet_replay_handle r, int32_t* pos, int32_t* full, int32_t* rows, uint64_t* calls) {
  if (!r) return FLEET_ERR_INVALID;
  if (pos) *pos = r->pos;
  if (full) *full = r->full ? 1 : 0;
  if (rows) *rows = r->R;
  if (calls) *calls = r->calls;
  return FLEET_OK;
}

int fleet_replay_set_position(fleet_replay_handle r, int32_t pos, int32_t full, uint64_t calls) {
  if (!r) return FLEET_ERR_INVALID;
  if (pos < 0 || pos >= r->R || (full != 0 && full != 1)) {
    r->error = "fleet_replay_set_position: pos must be in [0, rows) and full 0 or 1";
    return FLEET_ERR_INVALID;
  }
  r->pos = pos;
  r->full = full != 0;
  r->calls = calls;
  return FLEET_OK;
}

}  // extern "C"
