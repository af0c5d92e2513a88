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
//   sac_actor_rows   grid (ceil(B / 16), 1): SAC's actor entry (fleet_sac_actor_grad_dev, on the image of a fleet_sac_create handle).  The
//              actor, its last layer [2A] untransformed in the LDS; fleet_sac_dev.h's sac_epilogue -- the code fleet_sac_act_dev runs --
//              writes a to act[16][A64], the row's log-probability to 16 scalars and eps and the unclamped l to keep[16][M2].  Critic 0
//              and, when present, critic 1 run from act[][] with their hidden activations to the scratch; threads 0..15 form qmin
//              and the selecting critic.  Each critic is walked back with the deltas in the LDS only, seeded with -1 / B in the rows
//              it won and 0 elsewhere, and into the action columns as td3_actor_rows does; critic 0's da waits in the scratch where
//              the actor's last delta will lie.  The head deltas dm, dl (include/fleet_hip.h states their float32 order) replace it,
//              then back through the actor, every delta to the scratch.  Thread 0 writes the tile's three partial sums.
//   sac_weights  td3_weights' grid over the actor's tiles alone, then one workgroup for SAC's statistics and the gradient of
//              log_ent_coef (a kernel of its own: td3_weights stays what it was).
//   td3_weights  one grid over 32 x 32 tiles of every weight gradient of the entry's networks, then one workgroup for the statistics.
//              A critic's first layer takes its input from two arrays: obs below column D, actions behind.
//   LDS of a rows launch: two buffers [16][S], S the widest out64 of all networks, the staged chunk [16][128], act [16][A64], 32 row
//              scalars: 20.1 KiB .. 104.1 KiB.  sac_actor_rows: keep [16][M2] more (M2: the actor's last out64) and 16 scalars, what
//              sac_target takes: (2 * 16 * S + 16 * 128 + 16 * (M2 + A64 + 1)) * 4 bytes, 24.1 KiB .. 120.1 KiB.
// The scratch, for a capacity of max_batch rows (floats; every array's row stride is its layer's out64):
//   per network and layer: act [max_batch][out64] (hidden layers), delta [max_batch][out64] (every layer);
//   part [ceil(max_batch / 16)][8]: the tiles' partial sums ([0]: q of the actor entry; [1], [2]: e * e of critic 0, 1; SAC's actor
//   entry: [0]: alpha * lp - qmin, [1]: lp, [2]: qmin).
// Rows at and past B are never read or written.  No atomics, no ordering between workgroups: launch boundaries only.  float32.
#include <hip/hip_runtime.h>

#include <string>

#include "fleet_grad_dev.h"
#include "fleet_mlp.h"
#include "fleet_policy.h"
#include "fleet_policy_dev.h"
#include "fleet_qtarget.h"
#include "fleet_sac_dev.h"

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

// ---- sac_actor_rows ------------------------------------------------------------------------------------------------------------------
struct SacRowsArgs {
  const QTargetDesc* desc;
  const float* base;
  const float *obs, *ent_coef;
  float *q, *dheads;
  float* scratch;
  Td3Scratch s;
  SacEpilogue x;
  int B, S;
  float invB;
};

// critic `net` from act[][]: its hidden activations to the scratch; returns q of row threadIdx.x (threads 0..15; 0 past B).  The
// value is read before the next head's first barrier, when nobody has written the buffer yet.
__device__ __forceinline__ float sac_critic_forward(const SacRowsArgs& t, const ForwardArgs& a, const PolicyHeadDesc* H, int net, float*& cur, float*& nxt,
                                                    float* xs, int row0, const StageTail& tail) {
  grad_head<kStageConcat>(a, H, cur, nxt, xs, t.S, row0, t.scratch, t.s.act[net], tail);
  return (threadIdx.x < kPolicyRows && row0 + (int)threadIdx.x < t.B) ? cur[threadIdx.x * t.S] : 0.0f;
}

__global__ __launch_bounds__(kPolicyThreads) void sac_actor_rows(SacRowsArgs t) {
  extern __shared__ float lds[];  // two buffers [16][S], the staged input [16][kPolicyChunk], keep [16][M2], act [16][M], lp [16]
  const QTargetDesc* __restrict__ d = t.desc;
  const PolicyHeadDesc* __restrict__ H0 = &d->net[0];
  const int S = t.S, B = t.B, D = d->obs_dim, A = d->act_dim, M = d->act64, nc = d->n_critics;
  const int M2 = H0->layer[H0->n_layers - 1].out64;
  float *cur = lds, *nxt = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* keep = xs + kPolicyRows * kPolicyChunk;  // [r][j]: eps; [r][A + j]: the unclamped l
  float* act = keep + kPolicyRows * M2;
  float* rowlp = act + kPolicyRows * M;
  float* rowv = xs;  // behind the last forward the staged chunk is free: [0][r]: qmin; [1][r]: the selecting critic; [2][r]: alpha * lp - qmin
  const int row0 = blockIdx.x * kPolicyRows;
  const float alpha = t.ent_coef[0];
  ForwardArgs a{};
  a.base = t.base, a.obs = t.obs, a.E = B;
  // ---- the actor and its epilogue: a -> act[][], lp -> rowlp[], eps and l -> keep[][] ----
  grad_head<kStagePlain>(a, H0, cur, nxt, xs, S, row0, t.scratch, t.s.act[0], StageTail{});
  sac_epilogue(t.x, cur, S, A, B, row0, act, M, rowlp, keep, M2);
  __syncthreads();
  // ---- the critics over concat(obs, a) ----
  const StageTail tail{act, M, D};
  const float q0 = sac_critic_forward(t, a, &d->net[1], 1, cur, nxt, xs, row0, tail);
  const float q1 = nc == 2 ? sac_critic_forward(t, a, &d->net[2], 2, cur, nxt, xs, row0, tail) : 0.0f;
  if (threadIdx.x < kPolicyRows) {
    const int r = threadIdx.x, row = row0 + r;
    const int sel = (nc == 2 && !(q0 <= q1)) ? 1 : 0;  // critic 0 on q_0 <= q_1
    const float qmin = sel ? q1 : q0;
    if (row < B && t.q) {
      t.q[(size_t)row * nc] = q0;
      if (nc == 2) t.q[(size_t)row * nc + 1] = q1;
    }
    const float p = alpha * rowlp[r];
    rowv[r] = qmin, rowv[kPolicyRows + r] = (float)sel, rowv[2 * kPolicyRows + r] = p - qmin;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    CompSum sl, sp, sq;
    for (int r = 0; r < kPolicyRows && row0 + r < B; ++r) sl.add(rowv[2 * kPolicyRows + r]), sp.add(rowlp[r]), sq.add(rowv[r]);
    float* part = t.scratch + t.s.part + (size_t)blockIdx.x * kPartStride;
    part[0] = sl.value(), part[1] = sp.value(), part[2] = sq.value();
  }
  // ---- back through each critic, the deltas in the LDS only; da = sum over the critics (one addend is an exact zero in every row) ----
  float* gda = t.scratch + t.s.delta[0][H0->n_layers - 1];  // [row][M2]: critic 0's da in columns below A until the head deltas replace it
  for (int c = 0; c < nc; ++c) {
    const PolicyHeadDesc* __restrict__ H = &d->net[1 + c];
    for (int item = threadIdx.x; item < kPolicyRows * 64; item += kPolicyThreads) {  // (a critic's last out64 is 64)
      const int r = item >> 6, j = item & 63;
      cur[r * S + j] = (j == 0 && row0 + r < B && rowv[kPolicyRows + r] == (float)c) ? -t.invB : 0.0f;
    }
    __syncthreads();
    grad_back_head<false>(t.base, H, cur, nxt, S, row0, B, t.scratch, t.s.act[1 + c], t.s.delta[1 + c]);
    // cur: d0[16][S] of the critic's first layer (zero past its `out`)
    const PolicyLayer L0 = H->layer[0];
    const float* W0 = t.base + L0.w_off;
    const int out4 = (L0.out + 3) & ~3;
    for (int item = threadIdx.x; item < kPolicyRows * M; item += kPolicyThreads) {  // (the loops over act's items map alike: a thread
      const int r = item / M, j = item - r * M;                                      //  meets its own element of gda again)
      const int row = row0 + r;
      if (row < B && j < A) {
        const float* wk = W0 + (size_t)(D + j) * L0.out64;  // (D + j < the layer's `in`: a row of Wt)
        float acc = 0.0f;
        for (int i = 0; i < out4; i += 4) {
          const float4 w4 = *reinterpret_cast<const float4*>(wk + i);
          const float4 d4 = *reinterpret_cast<const float4*>(cur + r * S + i);
          acc = fmaf(w4.w, d4.w, fmaf(w4.z, d4.z, fmaf(w4.y, d4.y, fmaf(w4.x, d4.x, acc))));
        }
        gda[(size_t)row * M2 + j] = c == 0 ? acc : gda[(size_t)row * M2 + j] + acc;
      }
    }
    __syncthreads();  // the readers of cur are done before the next seed is written
  }
  // ---- the head deltas (include/fleet_hip.h states the order): dm in column j, dl in column A + j, into nxt[16][S], the scratch and dheads ----
  {
    const float ab = alpha * t.invB;
    for (int item = threadIdx.x; item < kPolicyRows * M; item += kPolicyThreads) {
      const int r = item / M, j = item - r * M;
      const int row = row0 + r;
      float dm = 0.0f, dl = 0.0f;
      if (row < B && j < A) {
        const float av = act[item], eps = keep[r * M2 + j], l = keep[r * M2 + A + j];
        const float w = 1.0f - av * av;
        const float g = (2.0f * av) / (w + 1e-6f);
        const float dla = gda[(size_t)row * M2 + j] + ab * g;
        const float du = dla * w;
        dm = du;
        if (l >= -20.0f && l <= 2.0f) {  // (torch's clamp backward: the bounds inclusive; inside them ls = l)
          const float sd = (float)exp((double)l);
          const float se = sd * eps;
          const float ds = du * se;
          dl = ds - ab;
        }
        gda[(size_t)row * M2 + j] = dm, gda[(size_t)row * M2 + A + j] = dl;
        if (t.dheads) t.dheads[(size_t)row * 2 * A + j] = dm, t.dheads[(size_t)row * 2 * A + A + j] = dl;
      }
      if (j < A) nxt[r * S + j] = dm, nxt[r * S + A + j] = dl;
      if (j < 4 && 2 * A + j < S) nxt[r * S + 2 * A + j] = 0.0f;  // (the backward reads whole float4s: up to 3 columns past 2A)
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

// ---- sac_weights ---------------------------------------------------------------------------------------------------------------------
struct SacWeightArgs {
  GradEntry e[FLEET_POLICY_MAX_LAYERS];
  int n_entries, tile_blocks, B, n_tiles;
  const float *part, *ent_coef, *log_ent_coef;
  float *stats, *log_ent_coef_grad;
  float invB, target_entropy;
};

__global__ __launch_bounds__(256) void sac_weights(SacWeightArgs a) {
  __shared__ float ds[kGradRows][kGradTile], xs[kGradRows][kGradTile];
  const int bid = blockIdx.x;
  if (bid < a.tile_blocks) {
    const GradEntry& E = a.e[grad_entry_of(a.e, a.n_entries, bid)];
    grad_tile<false>(E, bid - E.first, a.B, ds, xs);
  } else if (threadIdx.x == 0) {
    CompSum sl, sp, sq;
    for (int t = 0; t < a.n_tiles; ++t) {
      const float* q = a.part + (size_t)t * kPartStride;
      sl.add(q[0]), sp.add(q[1]), sq.add(q[2]);
    }
    float st[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    st[0] = sl.value() * a.invB;
    st[2] = sp.value() * a.invB;
    st[3] = sq.value() * a.invB;
    st[4] = a.ent_coef[0];
    if (a.log_ent_coef) {
      const float g = -(st[2] + a.target_entropy);
      st[1] = a.log_ent_coef[0] * g;
      a.log_ent_coef_grad[0] = g;
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

std::string check_sac_actor_args(const FleetSacActorArgs* args, float* const* grads, int count) {
  if (!args) return "null FleetSacActorArgs";
  const FleetSacActorArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetSacActorArgs)) return "FleetSacActorArgs.struct_bytes does not match this library";
  if (x.noise_mode != FLEET_EXPLORE_NOISE_DRAW && x.noise_mode != FLEET_EXPLORE_NOISE_GIVEN) return "unknown noise_mode " + std::to_string(x.noise_mode);
  if (x.B < 1) return "B must be >= 1, got " + std::to_string(x.B);
  if (!x.obs) return "null obs";
  if (!x.ent_coef) return "null ent_coef";
  if (!x.stats) return "null stats";
  if (x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN && !x.noise) return "noise_mode GIVEN with a null noise";
  if (x.row_offset < 0) return "row_offset must be >= 0, got " + std::to_string(x.row_offset);
  if ((x.log_ent_coef == nullptr) != (x.log_ent_coef_grad == nullptr)) return "log_ent_coef and log_ent_coef_grad must be given together or both be null";
  if (x.reserved != 0) return "reserved must be 0";
  return check_grads(grads, count);
}

}  // namespace

struct FleetTd3 : FleetMlpUser {  // img: the ONLINE networks'; block: the scratch
  FleetTd3Params p{};
  Td3Scratch s{};
  int S = 64;  // the widest layer of all networks, out64
  size_t lds_bytes = 0;
  size_t sac_lds_bytes = 0;  // of sac_actor_rows (a squashed actor's image)
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
  const int M2 = img->nets[0].layer[img->nets[0].n_layers - 1].out64;
  h->sac_lds_bytes = ((size_t)2 * kPolicyRows * h->S + (size_t)kPolicyRows * kPolicyChunk + (size_t)kPolicyRows * (M2 + desc->act64 + 1)) * sizeof(float);
  constexpr int kMaxLds = (3 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk + kRowScalars) * (int)sizeof(float);
  // (sac_actor_rows: what sac_target takes at most, fleet_sac.hip)
  constexpr int kMaxSacLds = (3 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk + kPolicyRows * (FLEET_POLICY_MAX_WIDTH / 2 + 1)) * (int)sizeof(float);
  const int rc = mlp_user_open(h, img, off * sizeof(float), "scratch",
                               {{reinterpret_cast<const void*>(&td3_critic_rows), kMaxLds},
                                {reinterpret_cast<const void*>(&td3_actor_rows), kMaxLds},
                                {reinterpret_cast<const void*>(&sac_actor_rows), kMaxSacLds}},
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

int fleet_sac_actor_grad_dev(fleet_td3_handle h, const FleetSacActorArgs* args, float* const* grads, int count) {
  std::string why = check_sac_actor_args(args, grads, count);
  if (h && why.empty()) grad_check_sizes(&why, count, 2 * h->img->nets[0].n_layers, "W, b per layer of the actor", args->B, h->p.max_batch);
  if (const int rc = handle_enter("fleet_sac_actor_grad_dev", why, h, g_td3_error); rc != FLEET_OK) return rc;
  FleetMlpHandle* img = h->img;
  if (!qtarget_squashed(img)) {
    h->error = "fleet_sac_actor_grad_dev: the networks' actor is not a squashed Gaussian (fleet_sac_create makes one): a TD3 actor's gradient is fleet_td3_actor_grad_dev's";
    return FLEET_ERR_INVALID;
  }
  const FleetSacActorArgs& x = *args;
  const QTargetDesc* desc = static_cast<const QTargetDesc*>(img->record);
  const int B = x.B, n_tiles = (B + kPolicyRows - 1) / kPolicyRows;
  SacRowsArgs t{};
  t.desc = reinterpret_cast<const QTargetDesc*>(img->block);
  t.base = reinterpret_cast<const float*>(img->block);
  t.obs = x.obs, t.ent_coef = x.ent_coef, t.q = x.q_out, t.dheads = x.dheads_out;
  t.scratch = h->floats(), t.s = h->s, t.S = h->S, t.B = B;
  t.invB = 1.0f / (float)B;
  t.x.noise = x.noise, t.x.actions = x.actions_out, t.x.log_prob = x.log_prob_out;
  t.x.seed = x.seed, t.x.step = x.step, t.x.id0 = (uint32_t)x.row_offset;
  t.x.given = x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN, t.x.deterministic = 0;
  SacWeightArgs g{};
  grad_fill_entries(g.e, &g.n_entries, &g.tile_blocks, img->nets, 0, 1, t.scratch, h->s.act, h->s.delta, t.obs, desc->obs_dim, nullptr, 0, grads);
  g.B = B, g.n_tiles = n_tiles, g.part = t.scratch + h->s.part, g.ent_coef = x.ent_coef;
  g.log_ent_coef = x.log_ent_coef, g.log_ent_coef_grad = x.log_ent_coef_grad;
  g.stats = x.stats, g.invB = t.invB, g.target_entropy = x.target_entropy;
  FLEET_HANDLE_TRY(h, hipSetDevice(img->device));
  hipLaunchKernelGGL(sac_actor_rows, dim3((unsigned)n_tiles), dim3(kPolicyThreads), h->sac_lds_bytes, img->stream, t);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(sac_weights, dim3((unsigned)(g.tile_blocks + 1)), dim3(256), 0, img->stream, g);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // extern "C"
