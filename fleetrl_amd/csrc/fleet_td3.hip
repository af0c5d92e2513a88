// fleet_td3.hip -- the critic and actor minibatch gradients of a TD3 / DDPG agent on the device (include/fleet_hip.h "TD3 / DDPG
// minibatch gradients on the device"): what stable-baselines3's TD3.train computes with its two MSE losses and their backward, and on
// a delayed step with -critic.q1_forward(obs, actor(obs)).mean() and its backward, each in two launches.  The handle borrows the
// weight image of a fleet_qtarget handle that holds the ONLINE networks (fleet_mlp.h, fleet_qtarget.h) and owns a scratch.  The layer
// functions, the compensated sum and the weights launch's tile are fleet_grad_dev.h's, shared with fleet_ppo.hip.
//   td3_critic_rows  grid (ceil(B / 16), n_critics), 256 threads.  The tile's 16 action rows are copied to act[16][A64] in the LDS;
//              critic c's first layer stages its input 128 columns at a time as qtarget_target does (kStageConcat: columns below D from
//              obs in global memory, columns D .. D+A-1 from act[][], wherever the seam falls in a chunk).  Every hidden activation goes
//              to the scratch.  Threads 0..15 form e = q - y, dq = (2 / B) e; the SAME workgroup walks back through the layers, every
//              layer's delta goes to the scratch.  Thread 0 writes the tile's partial sum of e * e.
//   td3_actor_rows   grid (ceil(B / 16), 1).  The actor, its last layer untransformed in the LDS; an epilogue writes a = output_of(mean)
//              to act[16][A64] and the transform's derivative g to the scratch, where the actor's last delta will lie.  Critic 0
//              runs from act[][] -- the target launch's flow -- with its hidden activations to the scratch.  dq = -1 / B goes back
//              through critic 0 with the deltas in the LDS only (no critic gradient is produced), then from the first layer's delta
//              into the ACTION columns: da[j] = fmaf chain over i ascending of Wt0[D + j][i] * d0[i]; dmean = da * g, in place of g;
//              then back through the actor, every delta to the scratch.  Thread 0 writes the tile's partial sum of q.
//   td3_weights  one grid over 32 x 32 tiles of every weight gradient of the entry's networks, then one workgroup for the statistics.
//              A critic's first layer takes its input from two arrays: obs below column D, actions behind.
//   LDS of a rows launch: two buffers [16][S], S the widest out64 of all networks, the staged chunk [16][128], act [16][A64], 32 row
//              scalars: 20.1 KiB .. 104.1 KiB.
// The scratch, for a capacity of max_batch rows (floats; every array's row stride is its layer's out64):
//   per network and layer: act [max_batch][out64] (hidden layers), delta [max_batch][out64] (every layer);
//   part [ceil(max_batch / 16)][8]: the tiles' partial sums ([0]: q of the actor entry; [1], [2]: e * e of critic 0, 1).
// Rows at and past B are never read or written.  No atomics, no ordering between workgroups: launch boundaries only.  float32.
#include <hip/hip_runtime.h>

#include <string>

#include "fleet_grad_dev.h"
#include "fleet_mlp.h"
#include "fleet_policy.h"
#include "fleet_policy_dev.h"
#include "fleet_qtarget.h"

namespace {

constexpr int kPartStride = 8;  // floats per tile in part[][]
constexpr int kRowScalars = 2 * kPolicyRows;

struct Td3Scratch {  // offsets in floats from the scratch's start
  uint64_t act[kQNets][FLEET_POLICY_MAX_LAYERS];
  uint64_t delta[kQNets][FLEET_POLICY_MAX_LAYERS];
  uint64_t part, floats;
};

struct RowsArgs {
  const QTargetDesc* desc;
  const float* base;
  const float *obs, *actions, *target_q;  // (actions, target_q: the critic entry's)
  float *q, *actions_out;
  float* scratch;
  Td3Scratch s;
  int B, S;
  float invB;
};

__global__ __launch_bounds__(kPolicyThreads) void td3_critic_rows(RowsArgs t) {
  extern __shared__ float lds[];  // two buffers [16][S], the staged input [16][kPolicyChunk], act [16][M], the rows' scalars [2][16]
  const QTargetDesc* __restrict__ d = t.desc;
  const int c = blockIdx.y, net = 1 + c;
  const PolicyHeadDesc* __restrict__ H = &d->net[net];
  const int S = t.S, B = t.B, D = d->obs_dim, A = d->act_dim, M = d->act64, nc = d->n_critics;
  float *cur = lds, *nxt = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* act = xs + kPolicyRows * kPolicyChunk;
  float* rowv = act + kPolicyRows * M;  // [0][r]: dq; [1][r]: e * e
  const int row0 = blockIdx.x * kPolicyRows;
  const int n = H->n_layers;
  // the tile's action rows (zeros past A and in the rows past B); the first layer's barrier stands between this and the staging
  for (int item = threadIdx.x; item < kPolicyRows * M; item += kPolicyThreads) {
    const int r = item / M, j = item - r * M;
    const int row = row0 + r;
    act[item] = (row < B && j < A) ? t.actions[(size_t)row * A + j] : 0.0f;
  }
  ForwardArgs a{};
  a.base = t.base, a.obs = t.obs, a.E = B;
  grad_head<kStageConcat>(a, H, cur, nxt, xs, S, row0, t.scratch, t.s.act[net], StageTail{act, M, D});
  // cur: q in column 0 of y[16][S]; nxt is free
  const PolicyLayer LL = H->layer[n - 1];
  float* gdl = t.scratch + t.s.delta[net][n - 1];
  if (threadIdx.x < kPolicyRows) {
    const int r = threadIdx.x, row = row0 + r;
    float dq = 0.0f, sq = 0.0f;
    if (row < B) {
      const float qv = cur[r * S];
      if (t.q) t.q[(size_t)row * nc + c] = qv;
      const float e = qv - t.target_q[row];
      dq = (2.0f * t.invB) * e;
      sq = e * e;
      gdl[(size_t)row * LL.out64] = dq;
    }
    rowv[r] = dq, rowv[kPolicyRows + r] = sq;
  }
  __syncthreads();
  for (int item = threadIdx.x; item < kPolicyRows * 64; item += kPolicyThreads) {  // (a critic's last out64 is 64)
    const int r = item >> 6, j = item & 63;
    cur[r * S + j] = j == 0 ? rowv[r] : 0.0f;
  }
  if (threadIdx.x == 0) {
    CompSum sq;
    for (int r = 0; r < kPolicyRows && row0 + r < B; ++r) sq.add(rowv[kPolicyRows + r]);
    t.scratch[t.s.part + (size_t)blockIdx.x * kPartStride + 1 + c] = sq.value();
  }
  __syncthreads();
  grad_back_head<true>(t.base, H, cur, nxt, S, row0, B, t.scratch, t.s.act[net], t.s.delta[net]);
}

__global__ __launch_bounds__(kPolicyThreads) void td3_actor_rows(RowsArgs t) {
  extern __shared__ float lds[];  // as td3_critic_rows
  const QTargetDesc* __restrict__ d = t.desc;
  const PolicyHeadDesc* __restrict__ H0 = &d->net[0];
  const PolicyHeadDesc* __restrict__ H1 = &d->net[1];
  const int S = t.S, B = t.B, D = d->obs_dim, A = d->act_dim, M = d->act64;
  float *cur = lds, *nxt = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* act = xs + kPolicyRows * kPolicyChunk;
  float* rowv = act + kPolicyRows * M;  // [0][r]: q
  const int row0 = blockIdx.x * kPolicyRows;
  ForwardArgs a{};
  a.base = t.base, a.obs = t.obs, a.E = B;
  // ---- the actor ----
  grad_head<kStagePlain>(a, H0, cur, nxt, xs, S, row0, t.scratch, t.s.act[0], StageTail{});
  // cur: mean[16][S].  a -> act[][]; the transform's derivative g -> where the actor's last delta will lie (the thread that writes an
  // element here is the one that replaces it below: the two loops map items alike)
  float* gda = t.scratch + t.s.delta[0][H0->n_layers - 1];
  {
    const int output = H0->output;
    const float lo = H0->lo, hi = H0->hi;
    for (int item = threadIdx.x; item < kPolicyRows * M; item += kPolicyThreads) {
      const int r = item / M, j = item - r * M;
      const int row = row0 + r;
      const float m = cur[r * S + j];
      const float av = output_of(m, output, lo, hi);
      act[item] = av;
      if (row < B && j < A) {
        if (t.actions_out) t.actions_out[(size_t)row * A + j] = av;
        float g = 1.0f;
        if (output == FLEET_POLICY_OUT_TANH) g = fmaf(-av, av, 1.0f);
        else if (output == FLEET_POLICY_OUT_CLIP) g = (m >= lo && m <= hi) ? 1.0f : 0.0f;
        gda[(size_t)row * M + j] = g;
      }
    }
  }
  // ---- critic 0 over concat(obs, a) (the first layer's barrier stands between the epilogue and the staging) ----
  grad_head<kStageConcat>(a, H1, cur, nxt, xs, S, row0, t.scratch, t.s.act[1], StageTail{act, M, D});
  if (threadIdx.x < kPolicyRows) {
    const int r = threadIdx.x, row = row0 + r;
    float qv = 0.0f;
    if (row < B) {
      qv = cur[r * S];
      if (t.q) t.q[row] = qv;
    }
    rowv[r] = qv;
  }
  __syncthreads();
  for (int item = threadIdx.x; item < kPolicyRows * 64; item += kPolicyThreads) {
    const int r = item >> 6, j = item & 63;
    cur[r * S + j] = (j == 0 && row0 + r < B) ? -t.invB : 0.0f;
  }
  if (threadIdx.x == 0) {
    CompSum q;
    for (int r = 0; r < kPolicyRows && row0 + r < B; ++r) q.add(rowv[r]);
    t.scratch[t.s.part + (size_t)blockIdx.x * kPartStride] = q.value();
  }
  __syncthreads();
  // ---- back through critic 0, the deltas in the LDS only ----
  grad_back_head<false>(t.base, H1, cur, nxt, S, row0, B, t.scratch, t.s.act[1], t.s.delta[1]);
  // cur: d0[16][S] of critic 0's first layer (zero past its `out`) -> dmean[16][S] in nxt (zero past A and in the rows past B)
  {
    const PolicyLayer L0 = H1->layer[0];
    const float* W0 = t.base + L0.w_off;
    const int out4 = (L0.out + 3) & ~3;
    for (int item = threadIdx.x; item < kPolicyRows * M; item += kPolicyThreads) {
      const int r = item / M, j = item - r * M;
      const int row = row0 + r;
      float v = 0.0f;
      if (row < B && j < A) {
        const float* wk = W0 + (size_t)(D + j) * L0.out64;  // (D + j < the layer's `in`: a row of Wt)
        float acc = 0.0f;
        for (int i = 0; i < out4; i += 4) {
          const float4 w4 = *reinterpret_cast<const float4*>(wk + i);
          const float4 d4 = *reinterpret_cast<const float4*>(cur + r * S + i);
          acc = fmaf(w4.w, d4.w, fmaf(w4.z, d4.z, fmaf(w4.y, d4.y, fmaf(w4.x, d4.x, acc))));
        }
        v = acc * gda[(size_t)row * M + j];
        gda[(size_t)row * M + j] = v;
      }
      nxt[r * S + j] = v;
    }
  }
  __syncthreads();
  {
    float* tmp = cur;
    cur = nxt;
    nxt = tmp;
  }
  // ---- back through the actor ----
  grad_back_head<true>(t.base, H0, cur, nxt, S, row0, B, t.scratch, t.s.act[0], t.s.delta[0]);
}

// ---- td3_weights ---------------------------------------------------------------------------------------------------------------------
constexpr int kMaxEntries = 2 * FLEET_POLICY_MAX_LAYERS;  // the critic entry's: two critics
constexpr int kCriticEntry = 0, kActorEntry = 1;

struct WeightArgs {
  GradEntry e[kMaxEntries];
  int n_entries, tile_blocks, B, n_tiles, entry, nc;
  const float* part;
  float* stats;
  float invB;
};

__global__ __launch_bounds__(256) void td3_weights(WeightArgs a) {
  __shared__ float ds[kGradRows][kGradTile], xs[kGradRows][kGradTile];
  const int bid = blockIdx.x;
  if (bid < a.tile_blocks) {
    const GradEntry& E = a.e[grad_entry_of(a.e, a.n_entries, bid)];
    grad_tile<true>(E, bid - E.first, a.B, ds, xs);
  } else if (threadIdx.x == 0) {
    CompSum s0, s1;
    float st[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (a.entry == kCriticEntry) {
      for (int t = 0; t < a.n_tiles; ++t) {
        const float* q = a.part + (size_t)t * kPartStride;
        s0.add(q[1]);
        if (a.nc == 2) s1.add(q[2]);
      }
      st[1] = s0.value() * a.invB;
      st[2] = a.nc == 2 ? s1.value() * a.invB : 0.0f;
      st[0] = st[1] + st[2];
    } else {
      for (int t = 0; t < a.n_tiles; ++t) s0.add(a.part[(size_t)t * kPartStride]);
      st[0] = -(s0.value() * a.invB);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) a.stats[i] = st[i];
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_td3_error;  // of the last failed call without a handle

std::string check_params(const FleetTd3Params* p) {
  if (!p) return "null FleetTd3Params";
  if (p->struct_bytes != (int32_t)sizeof(FleetTd3Params)) return "FleetTd3Params.struct_bytes does not match this library";
  if (p->max_batch < 1 || p->max_batch > (1 << 24)) return "max_batch must be in 1..16777216, got " + std::to_string(p->max_batch);
  return "";
}

// what both entries refuse about their gradient tensors, looked at without the handle
std::string check_grads(float* const* grads, int count) {
  if (!grads) return "null grads";
  if (count < 1 || count > kMlpMaxTensors) return "count must be in 1.." + std::to_string(kMlpMaxTensors) + ", got " + std::to_string(count);
  for (int i = 0; i < count; ++i)
    if (!grads[i]) return "gradient tensor " + std::to_string(i) + " is null";
  return "";
}

std::string check_critic_args(const FleetTd3CriticArgs* args, float* const* grads, int count) {
  if (!args) return "null FleetTd3CriticArgs";
  const FleetTd3CriticArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetTd3CriticArgs)) return "FleetTd3CriticArgs.struct_bytes does not match this library";
  if (x.B < 1) return "B must be >= 1, got " + std::to_string(x.B);
  if (!x.obs) return "null obs";
  if (!x.actions) return "null actions";
  if (!x.target_q) return "null target_q";
  if (!x.stats) return "null stats";
  if (x.reserved != 0) return "reserved must be 0";
  return check_grads(grads, count);
}

std::string check_actor_args(const FleetTd3ActorArgs* args, float* const* grads, int count) {
  if (!args) return "null FleetTd3ActorArgs";
  const FleetTd3ActorArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetTd3ActorArgs)) return "FleetTd3ActorArgs.struct_bytes does not match this library";
  if (x.B < 1) return "B must be >= 1, got " + std::to_string(x.B);
  if (!x.obs) return "null obs";
  if (!x.stats) return "null stats";
  if (x.reserved != 0) return "reserved must be 0";
  return check_grads(grads, count);
}

}  // namespace

struct FleetTd3 : FleetMlpUser {  // img: the ONLINE networks'; block: the scratch
  FleetTd3Params p{};
  Td3Scratch s{};
  int S = 64;  // the widest layer of all networks, out64
  size_t lds_bytes = 0;
};

namespace {

// the launches of one entry: `rows` over grid (tiles, grid_y), then the weights of networks net0 .. net0 + n_nets - 1
int launch_entry(FleetTd3* h, void (*rows)(RowsArgs), int grid_y, RowsArgs& t, int entry, int net0, int n_nets, float* const* grads, float* stats) {
  FleetMlpHandle* img = h->img;
  const QTargetDesc* desc = static_cast<const QTargetDesc*>(img->record);
  const int B = t.B, n_tiles = (B + kPolicyRows - 1) / kPolicyRows;
  t.desc = reinterpret_cast<const QTargetDesc*>(img->block);
  t.base = reinterpret_cast<const float*>(img->block);
  t.scratch = h->floats(), t.s = h->s, t.S = h->S;
  t.invB = 1.0f / (float)B;
  WeightArgs g{};
  grad_fill_entries(g.e, &g.n_entries, &g.tile_blocks, img->nets, net0, n_nets, t.scratch, h->s.act, h->s.delta, t.obs, desc->obs_dim,
                    net0 > 0 ? t.actions : nullptr, desc->act_dim, grads);  // (the critics' first layers take the actions behind the seam)
  g.B = B, g.n_tiles = n_tiles, g.entry = entry, g.nc = desc->n_critics;
  g.part = t.scratch + h->s.part, g.stats = stats, g.invB = t.invB;
  FLEET_HANDLE_TRY(h, hipSetDevice(img->device));
  hipLaunchKernelGGL(rows, dim3((unsigned)n_tiles, (unsigned)grid_y), dim3(kPolicyThreads), h->lds_bytes, img->stream, t);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(td3_weights, dim3((unsigned)(g.tile_blocks + 1)), dim3(256), 0, img->stream, g);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_td3_create(fleet_qtarget_handle nets_handle, const FleetTd3Params* p, fleet_td3_handle* out) {
  if (out) *out = nullptr;
  std::string why = check_params(p);
  if (why.empty() && !out) why = "null output handle";
  FleetMlpHandle* img = why.empty() ? mlp_borrow(nets_handle, sizeof(QTargetDesc), "networks", &why) : nullptr;
  if (!why.empty()) return handle_refuse(g_td3_error, "fleet_td3_create", why, FLEET_ERR_INVALID);
  const QTargetDesc* desc = static_cast<const QTargetDesc*>(img->record);
  FleetTd3* h = new FleetTd3();
  h->p = *p;
  const uint64_t mb = (uint64_t)p->max_batch;
  uint64_t off = grad_scratch_layout(img->nets, img->n_nets, mb, h->s.act, h->s.delta, &h->S);
  h->s.part = off, off += (mb + kPolicyRows - 1) / kPolicyRows * kPartStride;
  h->s.floats = off;
  h->lds_bytes = ((size_t)2 * kPolicyRows * h->S + (size_t)kPolicyRows * kPolicyChunk + (size_t)kPolicyRows * desc->act64 + kRowScalars) * sizeof(float);
  constexpr int kMaxLds = (3 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk + kRowScalars) * (int)sizeof(float);
  const int rc = mlp_user_open(h, img, off * sizeof(float), "scratch",
                               {{reinterpret_cast<const void*>(&td3_critic_rows), kMaxLds}, {reinterpret_cast<const void*>(&td3_actor_rows), kMaxLds}},
                               "rows", &why);
  if (rc != FLEET_OK) {
    fleet_td3_destroy(h);
    return handle_refuse(g_td3_error, "fleet_td3_create", why, rc);
  }
  *out = h;
  return FLEET_OK;
}

int fleet_td3_destroy(fleet_td3_handle h) {
  if (!h) return FLEET_OK;
  mlp_user_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_td3_last_error(fleet_td3_handle h) { return h ? h->error.c_str() : g_td3_error.c_str(); }

int fleet_td3_describe(fleet_td3_handle h, FleetTd3Params* out, uint64_t* scratch_bytes, int32_t* tile_rows) {
  if (!h || !out || !scratch_bytes || !tile_rows) return FLEET_ERR_INVALID;
  *out = h->p;
  *scratch_bytes = h->s.floats * sizeof(float);
  *tile_rows = kPolicyRows;
  return FLEET_OK;
}

int fleet_td3_critic_grad_dev(fleet_td3_handle h, const FleetTd3CriticArgs* args, float* const* grads, int count) {
  std::string why = check_critic_args(args, grads, count);
  if (h && why.empty())
    grad_check_sizes(&why, count, h->img->n_tensors - 2 * h->img->nets[0].n_layers, "W, b per layer, critic after critic", args->B, h->p.max_batch);
  if (const int rc = handle_enter("fleet_td3_critic_grad_dev", why, h, g_td3_error); rc != FLEET_OK) return rc;
  const int nc = h->img->n_nets - 1;
  RowsArgs t{};
  t.obs = args->obs, t.actions = args->actions, t.target_q = args->target_q, t.q = args->q, t.B = args->B;
  return launch_entry(h, td3_critic_rows, nc, t, kCriticEntry, 1, nc, grads, args->stats);
}

int fleet_td3_actor_grad_dev(fleet_td3_handle h, const FleetTd3ActorArgs* args, float* const* grads, int count) {
  std::string why = check_actor_args(args, grads, count);
  if (h && why.empty()) grad_check_sizes(&why, count, 2 * h->img->nets[0].n_layers, "W, b per layer of the actor", args->B, h->p.max_batch);
  if (const int rc = handle_enter("fleet_td3_actor_grad_dev", why, h, g_td3_error); rc != FLEET_OK) return rc;
  if (qtarget_squashed(h->img)) {  // (td3_actor_rows takes act64 for the actor's last out64 and the last layer for the action)
    h->error = "fleet_td3_actor_grad_dev: the networks' actor is a squashed Gaussian (fleet_sac_create): its gradient is not this entry's";
    return FLEET_ERR_INVALID;
  }
  RowsArgs t{};
  t.obs = args->obs, t.q = args->q, t.actions_out = args->actions_out, t.B = args->B;
  return launch_entry(h, td3_actor_rows, 1, t, kActorEntry, 0, 1, grads, args->stats);
}

}  // extern "C"
