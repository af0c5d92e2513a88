// fleet_ppo.hip -- the gradients of PPO's minibatch loss on the device (include/fleet_hip.h "PPO minibatch gradients on the device"):
// what stable-baselines3's PPO.train computes per minibatch with evaluate_actions, the clipped loss and loss.backward(), in two
// launches on the policy's stream.  The handle borrows the weight image of a two-head policy (fleet_mlp.h) and owns a scratch.
//   ppo_rows   grid (ceil(B / 16), 2), 256 threads: the policy's tile.  A workgroup takes 16 rows through one head with the chain of
//              fleet_policy_dev.h (stage, accumulate, hidden_act as they are); its layer function (fleet_grad_dev.h, shared with
//              fleet_td3.hip, as are the backward layer, the compensated sum and the weights launch's tile) also stores every hidden
//              activation to the scratch.  The last layer leaves its rows untransformed in the LDS.  Head 0's epilogue forms the
//              log-probability terms with sample_epilogue's expression and sums them in its order, then the row's ratio, clip and
//              d loss / d log-probability; head 1's forms d loss / d value (through SB3's value clip in the second instance,
//              ppo_rows<true>, which fleet_ppo_grad_vclip_dev launches: the same text, the clip compiled in).  The SAME workgroup then walks back through its layers:
//              a thread owns input column k of all 16 rows, d_prev[r][k] = (fmaf chain over j ascending of Wt[k][j] * d[r][j]) *
//              act'(h[r][k]); every layer's delta goes to the scratch.  Thread 0 writes the tile's partial sums of the statistics.
//              LDS: two buffers [16][T], T the widest layer of both heads (out64), the staged chunk [16][128], 64 row scalars.
//   ppo_weights  one grid over 32 x 32 tiles of every weight gradient, then the log_std gradient's blocks, then one workgroup for the
//              statistics.  A thread owns 2 x 2 elements of dW; each is ONE chain over the rows in ascending b, acc = fmaf(d[b][j],
//              x[b][k], acc), with 16 rows at a time staged in the LDS (d and the activations from the scratch, obs for a first
//              layer); db[j] is the ascending sum of d[b][j], kept by the threads of the first k tile.  Stored with torch's index.
// The scratch, for a capacity of max_batch rows (floats; every array's row stride is its layer's out64):
//   per head and layer: act [max_batch][out64] (hidden layers), delta [max_batch][out64] (every layer);
//   ls [max_batch][A64]: the rows' log_std terms;  part [ceil(max_batch / 16)][8]: the tiles' partial sums.
// Rows at and past B are never read or written.  No atomics, no ordering between workgroups: launch boundaries only.  float32.
// The gated instances (kGated; fleet_ppo_grad_gated_dev launches them, the others keep their text and their code): every workgroup
// of both launches reads the word `skip` once at its top, one uniform load and a scalar branch, and returns when it is set; the
// statistics workgroup of ppo_weights then writes `decided` = ((double)approx_kl > threshold) behind the statistics.  The property
// that makes this safe without atomics: NO launch reads a word that a workgroup of the SAME launch may write -- `skip` was written
// by an earlier launch, and `decided` is read by later launches only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <type_traits>

#include "fleet_grad_dev.h"
#include "fleet_mlp.h"
#include "fleet_policy.h"
#include "fleet_policy_dev.h"

namespace {

constexpr int kPartStride = 8;  // floats per tile in part[][]: policy term, squared value error, kl term, clipped rows

struct PpoScratch {  // offsets in floats from the scratch's start
  uint64_t act[FLEET_POLICY_MAX_HEADS][FLEET_POLICY_MAX_LAYERS];
  uint64_t delta[FLEET_POLICY_MAX_HEADS][FLEET_POLICY_MAX_LAYERS];
  uint64_t ls, part, floats;
};

struct RowsArgs {
  const PolicyDesc* desc;
  const float* base;
  const float *obs, *actions, *old_lp, *adv, *ret, *log_std;
  float *values, *log_prob;
  float* scratch;
  PpoScratch s;
  int B, T;
  float clip, vf_coef, invB;
};

struct RowsArgsVclip : RowsArgs {
  const float* old_v;  // the value clip's old values
  float cv;            // clip_range_vf
};

struct RowsArgsGated : RowsArgsVclip {  // (old_v and cv are not read without the value clip)
  const uint32_t* skip;  // nonzero: the launch returns at once
};

// kVclip: the instance with the value clip (a second instance, so that the first one stays the code it was)
// kGated: the instances that return at their top when *skip is set (further instances, for the same reason)
template <bool kVclip, bool kGated = false>
__global__ __launch_bounds__(kPolicyThreads) void ppo_rows(
    std::conditional_t<kGated, RowsArgsGated, std::conditional_t<kVclip, RowsArgsVclip, RowsArgs>> t) {
  if constexpr (kGated) {
    if (__builtin_amdgcn_readfirstlane(*t.skip)) return;
  }
  extern __shared__ float lds[];  // two buffers [16][T], the staged input [16][kPolicyChunk], the rows' scalars [4][16]
  const PolicyDesc* __restrict__ d = t.desc;
  const int head = blockIdx.y;
  const PolicyHeadDesc* __restrict__ H = &d->head[head];
  const int S = t.T, B = t.B;
  float *cur = lds, *nxt = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* rowv = xs + kPolicyRows * kPolicyChunk;  // [0][r]: glp or dv; [1..3][r]: the row's terms of the statistics
  const int row0 = blockIdx.x * kPolicyRows;
  const int n = H->n_layers;
  ForwardArgs a{};
  a.base = t.base, a.obs = t.obs, a.E = B;
  // ---- forward ----
  grad_head<kStagePlain>(a, H, cur, nxt, xs, S, row0, t.scratch, t.s.act[head], StageTail{});
  // cur: y[16][S] of the last layer; nxt is free
  const PolicyLayer LL = H->layer[n - 1];
  float* gdl = t.scratch + t.s.delta[head][n - 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (head == 0) {
    const int A = LL.out, M = LL.out64;
    // the log-probability terms, sample_epilogue's expression on the stored action -> nxt
    for (int item = threadIdx.x; item < kPolicyRows * A; item += kPolicyThreads) {
      const int r = item / A, j = item - r * A;
      const int row = row0 + r;
      if (row >= B) continue;
      const float sc = t.log_std[j], m = cur[r * S + j];
      const float sd = expf(sc);
      const float dm = t.actions[(size_t)row * A + j] - m;
      nxt[r * S + j] = -(dm * dm) / (2.0f * sd * sd) - sc - 0.9189385332f;
    }
    __syncthreads();
    // a wavefront sums 4 rows: every lane its columns lane, lane + 64, ... in ascending order, then a butterfly over the 64 lanes
    for (int r = w * (kPolicyRows / kPolicyWaves); r < (w + 1) * (kPolicyRows / kPolicyWaves); ++r) {
      const int row = row0 + r;
      float sum = 0.0f;
      if (row < B)  // (uniform over the wavefront)
        for (int j = lane; j < A; j += 64) sum += nxt[r * S + j];
#pragma unroll
      for (int dd = 1; dd < 64; dd <<= 1) sum += __shfl_xor(sum, dd, 64);
      float glp = 0.0f, pterm = 0.0f, kl = 0.0f, cf = 0.0f;
      if (lane == 0 && row < B) {
        const float lp = sum, adv = t.adv[row];
        if (t.log_prob) t.log_prob[row] = lp;
        const float lr = lp - t.old_lp[row];
        const float ratio = expf(lr);
        const float lo = 1.0f - t.clip, hi = 1.0f + t.clip;
        const float cl = ratio < lo ? lo : (ratio > hi ? hi : ratio);
        const float s1 = adv * ratio, s2 = adv * cl;
        pterm = -(s1 < s2 ? s1 : s2);
        const bool alive = (ratio >= lo && ratio <= hi) || s1 < s2;
        glp = alive ? -(adv * ratio) * t.invB : 0.0f;
        kl = (ratio - 1.0f) - lr;
        cf = fabsf(ratio - 1.0f) > t.clip ? 1.0f : 0.0f;
      }
      if (lane == 0) rowv[r] = glp, rowv[16 + r] = pterm, rowv[32 + r] = kl, rowv[48 + r] = cf;
    }
    __syncthreads();
    // the last layer's delta in place of y (zero past A and in the rows past B), and the rows' log_std terms
    float* gls = t.scratch + t.s.ls;
    for (int item = threadIdx.x; item < kPolicyRows * M; item += kPolicyThreads) {
      const int r = item / M, j = item - r * M;
      const int row = row0 + r;
      float dmean = 0.0f;
      if (row < B && j < A) {
        const float sc = t.log_std[j], glp = rowv[r];
        const float sd = expf(sc);
        const float dm = t.actions[(size_t)row * A + j] - cur[r * S + j];
        dmean = glp * (dm / (sd * sd));
        gdl[(size_t)row * M + j] = dmean;
        gls[(size_t)row * M + j] = glp * ((dm * dm) / (sd * sd) - 1.0f);
      }
      cur[r * S + j] = dmean;
    }
    if (threadIdx.x == 0) {
      CompSum p, k, c;
      for (int r = 0; r < kPolicyRows && row0 + r < B; ++r) p.add(rowv[16 + r]), k.add(rowv[32 + r]), c.add(rowv[48 + r]);
      float* part = t.scratch + t.s.part + (size_t)blockIdx.x * kPartStride;
      part[0] = p.value(), part[2] = k.value(), part[3] = c.value();
    }
  } else {
    if (threadIdx.x < kPolicyRows) {
      const int r = threadIdx.x, row = row0 + r;
      float dv = 0.0f, sq = 0.0f;
      if (row < B) {
        const float v = cur[r * S], ret = t.ret[row];
        if (t.values) t.values[row] = v;
        float vp = v;
        bool inside = true;
        if constexpr (kVclip) {
          const float ov = t.old_v[row], cv = t.cv;
          const float dl = v - ov;
          const float cd = dl < -cv ? -cv : (dl > cv ? cv : dl);
          vp = ov + cd;
          inside = dl >= -cv && dl <= cv;  // torch's clamp backward: ties pass, NaN does not
        }
        dv = inside ? ((2.0f * t.vf_coef) * t.invB) * (vp - ret) : 0.0f;
        const float e = ret - vp;
        sq = e * e;
        gdl[(size_t)row * LL.out64] = dv;
      }
      rowv[r] = dv, rowv[16 + r] = sq;
    }
    __syncthreads();
    for (int item = threadIdx.x; item < kPolicyRows * 64; item += kPolicyThreads) {  // (the critic's last out64 is 64)
      const int r = item >> 6, j = item & 63;
      cur[r * S + j] = j == 0 ? rowv[r] : 0.0f;
    }
    if (threadIdx.x == 0) {
      CompSum q;
      for (int r = 0; r < kPolicyRows && row0 + r < B; ++r) q.add(rowv[16 + r]);
      t.scratch[t.s.part + (size_t)blockIdx.x * kPartStride + 1] = q.value();
    }
  }
  __syncthreads();
  // ---- backward: layer l's delta in cur -> layer l - 1's in nxt, and to the scratch ----
  grad_back_head<true>(t.base, H, cur, nxt, S, row0, B, t.scratch, t.s.act[head], t.s.delta[head]);
}

// ---- ppo_weights ---------------------------------------------------------------------------------------------------------------------
constexpr int kMaxEntries = FLEET_POLICY_MAX_HEADS * FLEET_POLICY_MAX_LAYERS;

struct WeightArgs {
  GradEntry e[kMaxEntries];
  int n_entries, tile_blocks, ls_blocks, B;
  const float *ls, *part, *log_std;
  float *dlog_std, *stats;
  int A, M, n_tiles;
  float invB, vf_coef, ent_coef;
};

struct WeightArgsGated : WeightArgs {
  const uint32_t* skip;  // nonzero: the launch returns at once
  uint32_t* decided;     // written by the statistics workgroup: (double)approx_kl > thr
  double thr;
};

template <bool kGated>
__global__ __launch_bounds__(256) void ppo_weights(std::conditional_t<kGated, WeightArgsGated, WeightArgs> a) {
  if constexpr (kGated) {
    if (__builtin_amdgcn_readfirstlane(*a.skip)) return;
  }
  __shared__ float ds[kGradRows][kGradTile], xs[kGradRows][kGradTile];
  const int bid = blockIdx.x, B = a.B;
  if (bid < a.tile_blocks) {
    const GradEntry& E = a.e[grad_entry_of(a.e, a.n_entries, bid)];
    grad_tile<false>(E, bid - E.first, B, ds, xs);
  } else if (bid < a.tile_blocks + a.ls_blocks) {
    const int j = (bid - a.tile_blocks) * 256 + (int)threadIdx.x;
    if (j < a.A) {
      float sum = 0.0f;
      for (int b = 0; b < B; ++b) sum += a.ls[(size_t)b * a.M + j];
      a.dlog_std[j] = sum - a.ent_coef;
    }
  } else if (threadIdx.x == 0) {
    CompSum p, v, k, c;
    for (int t = 0; t < a.n_tiles; ++t) {
      const float* q = a.part + (size_t)t * kPartStride;
      p.add(q[0]), v.add(q[1]), k.add(q[2]), c.add(q[3]);
    }
    float ent = 0.0f;
    for (int j = 0; j < a.A; ++j) ent += 1.4189385332f + a.log_std[j];
    const float pl = p.value() * a.invB, vl = v.value() * a.invB, el = -ent;
    a.stats[0] = pl, a.stats[1] = vl, a.stats[2] = el;
    a.stats[3] = (pl + a.ent_coef * el) + a.vf_coef * vl;
    a.stats[4] = k.value() * a.invB, a.stats[5] = c.value() * a.invB, a.stats[6] = 0.0f, a.stats[7] = 0.0f;
    if constexpr (kGated) {
      const float kl = k.value() * a.invB;                 // (stats[4]'s bits)
      *a.decided = (double)kl > a.thr ? 1u : 0u;  // (a NaN does not stop the update, as in SB3)
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_ppo_error;  // of the last failed call without a handle

std::string check_params(const FleetPpoParams* p) {
  if (!p) return "null FleetPpoParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetPpoParams)) return "FleetPpoParams.struct_bytes does not match this library";
  if (p->max_batch < 1 || p->max_batch > (1 << 24)) return "max_batch must be in 1..16777216, got " + std::to_string(p->max_batch);
  return "";
}

// what fleet_ppo_grad_dev refuses, looked at without the handle; "" when the arguments pass
std::string check_grad_args(const FleetPpoGradArgs* args, float* const* grads, int count) {
  if (!args) return "null FleetPpoGradArgs";
  const FleetPpoGradArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetPpoGradArgs)) return "FleetPpoGradArgs.struct_bytes does not match this library";
  if (x.B < 1) return "B must be >= 1, got " + std::to_string(x.B);
  if (!x.obs) return "null obs";
  if (!x.actions) return "null actions";
  if (!x.old_log_prob) return "null old_log_prob";
  if (!x.advantages) return "null advantages";
  if (!x.returns) return "null returns";
  if (!x.log_std) return "null log_std";
  if (!x.stats) return "null stats";
  if (!(x.clip_range > 0.0f && x.clip_range < 1.0f)) return "clip_range must be in (0, 1)";
  if (std::isnan(x.vf_coef)) return "vf_coef is NaN";
  if (std::isnan(x.ent_coef)) return "ent_coef is NaN";
  if (!grads) return "null grads";
  if (count < 1 || count > 2 * kMaxEntries + 1) return "count must be the policy's tensors plus one (log_std), got " + std::to_string(count);
  for (int i = 0; i < count; ++i)
    if (!grads[i]) return "gradient tensor " + std::to_string(i) + " is null";
  return "";
}

// what fleet_ppo_grad_gated_dev refuses on top of fleet_ppo_grad_dev
std::string check_gated_args(const FleetPpoGradGatedArgs* args, float* const* grads, int count) {
  if (!args) return "null FleetPpoGradGatedArgs";
  if (args->struct_bytes != (int32_t)sizeof(FleetPpoGradGatedArgs)) return "FleetPpoGradGatedArgs.struct_bytes does not match this library";
  std::string why = check_grad_args(&args->base, grads, count);
  if (!why.empty()) return why;
  if (!(std::isfinite(args->clip_range_vf) && args->clip_range_vf >= 0.0f)) return "clip_range_vf must be finite and >= 0 (0: no value clip)";
  if (args->clip_range_vf > 0.0f && !args->old_values) return "null old_values";
  if (!args->gate.skip) return "null gate.skip";
  if (!args->gate.decided) return "null gate.decided";
  if (args->gate.skip == args->gate.decided) return "gate.skip and gate.decided are the same word";
  if (std::isnan(args->gate.threshold)) return "gate.threshold is NaN";
  return "";
}

// what fleet_ppo_grad_vclip_dev refuses on top of that
std::string check_vclip_args(const FleetPpoGradVclipArgs* args, float* const* grads, int count) {
  if (!args) return "null FleetPpoGradVclipArgs";
  if (args->struct_bytes != (int32_t)sizeof(FleetPpoGradVclipArgs)) return "FleetPpoGradVclipArgs.struct_bytes does not match this library";
  std::string why = check_grad_args(&args->base, grads, count);
  if (!why.empty()) return why;
  if (!args->old_values) return "null old_values";
  if (!(std::isfinite(args->clip_range_vf) && args->clip_range_vf > 0.0f)) return "clip_range_vf must be finite and > 0";
  return "";
}

}  // namespace

struct FleetPpo : FleetMlpUser {  // img: a two-head policy's; block: the scratch
  FleetPpoParams p{};
  PpoScratch s{};
  int T = 64;  // the widest layer of both heads, out64
  size_t lds_bytes = 0;
};

extern "C" {

int fleet_ppo_create(fleet_policy_handle policy, const FleetPpoParams* p, fleet_ppo_handle* out) {
  if (out) *out = nullptr;
  std::string why = check_params(p);
  if (why.empty() && !out) why = "null output handle";
  FleetMlpHandle* pol = why.empty() ? mlp_borrow(policy, sizeof(PolicyDesc), "policy", &why) : nullptr;
  if (pol && pol->n_nets != 2) why = "the policy has one head: the loss needs the critic (head 1)";
  if (why.empty()) {
    const PolicyHeadDesc& critic = pol->nets[1];
    if (critic.layer[critic.n_layers - 1].out != 1)
      why = "the critic's last width must be 1, got " + std::to_string(critic.layer[critic.n_layers - 1].out);
    else if (critic.output != FLEET_POLICY_OUT_NONE) why = "the critic's output transform must be NONE";
  }
  if (!why.empty()) return handle_refuse(g_ppo_error, "fleet_ppo_create", why, FLEET_ERR_INVALID);
  FleetPpo* h = new FleetPpo();
  h->p = *p;
  const PolicyHeadDesc* nets = pol->nets;
  const uint64_t mb = (uint64_t)p->max_batch;
  uint64_t off = grad_scratch_layout(nets, 2, mb, h->s.act, h->s.delta, &h->T);
  h->s.ls = off, off += mb * (uint64_t)nets[0].layer[nets[0].n_layers - 1].out64;
  h->s.part = off, off += (mb + kPolicyRows - 1) / kPolicyRows * kPartStride;
  h->s.floats = off;
  h->lds_bytes = ((size_t)2 * kPolicyRows * h->T + (size_t)kPolicyRows * kPolicyChunk + 64) * sizeof(float);
  constexpr int kMaxLds = (2 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk + 64) * (int)sizeof(float);
  const int rc = mlp_user_open(h, pol, off * sizeof(float), "scratch", {{reinterpret_cast<const void*>(&ppo_rows<false>), kMaxLds}, {reinterpret_cast<const void*>(&ppo_rows<true>), kMaxLds},
                                 {reinterpret_cast<const void*>(&ppo_rows<false, true>), kMaxLds}, {reinterpret_cast<const void*>(&ppo_rows<true, true>), kMaxLds}}, "rows", &why);
  if (rc != FLEET_OK) {
    fleet_ppo_destroy(h);
    return handle_refuse(g_ppo_error, "fleet_ppo_create", why, rc);
  }
  *out = h;
  return FLEET_OK;
}

int fleet_ppo_destroy(fleet_ppo_handle h) {
  if (!h) return FLEET_OK;
  mlp_user_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_ppo_last_error(fleet_ppo_handle h) { return h ? h->error.c_str() : g_ppo_error.c_str(); }

int fleet_ppo_describe(fleet_ppo_handle h, FleetPpoParams* out, uint64_t* scratch_bytes, int32_t* tile_rows) {
  if (!h || !out || !scratch_bytes || !tile_rows) return FLEET_ERR_INVALID;
  *out = h->p;
  *scratch_bytes = h->s.floats * sizeof(float);
  *tile_rows = kPolicyRows;
  return FLEET_OK;
}

}  // extern "C"

namespace {

// the two launches of every entry; old_values null: no value clip; gate null: the ungated instances
int ppo_grad_launch(fleet_ppo_handle h, const FleetPpoGradArgs& x, const float* old_values, float clip_range_vf, float* const* grads, int count,
                    const FleetPpoGate* gate = nullptr) {
  FleetMlpHandle* pol = h->img;
  const PolicyHeadDesc* nets = pol->nets;
  const int B = x.B, n_tiles = (B + kPolicyRows - 1) / kPolicyRows;
  const float invB = 1.0f / (float)B;
  float* scratch = h->floats();
  RowsArgsGated t{};
  t.desc = reinterpret_cast<const PolicyDesc*>(pol->block);
  t.base = reinterpret_cast<const float*>(pol->block);
  t.obs = x.obs, t.actions = x.actions, t.old_lp = x.old_log_prob, t.adv = x.advantages, t.ret = x.returns, t.log_std = x.log_std;
  t.values = x.values, t.log_prob = x.log_prob;
  t.scratch = scratch, t.s = h->s, t.B = B, t.T = h->T;
  t.clip = x.clip_range, t.vf_coef = x.vf_coef, t.invB = invB;
  t.old_v = old_values, t.cv = clip_range_vf;
  WeightArgsGated g{};
  grad_fill_entries(g.e, &g.n_entries, &g.tile_blocks, nets, 0, 2, scratch, h->s.act, h->s.delta, x.obs, nets[0].layer[0].in, nullptr, 0, grads);
  const PolicyLayer& LA = nets[0].layer[nets[0].n_layers - 1];
  g.ls_blocks = (LA.out + 255) / 256, g.B = B;
  g.ls = scratch + h->s.ls, g.part = scratch + h->s.part, g.log_std = x.log_std;
  g.dlog_std = grads[count - 1], g.stats = x.stats;
  g.A = LA.out, g.M = LA.out64, g.n_tiles = n_tiles;
  g.invB = invB, g.vf_coef = x.vf_coef, g.ent_coef = x.ent_coef;
  FLEET_HANDLE_TRY(h, hipSetDevice(pol->device));
  const dim3 rows_grid((unsigned)n_tiles, 2), weights_grid((unsigned)(g.tile_blocks + g.ls_blocks + 1));
  if (gate) {
    t.skip = g.skip = gate->skip, g.decided = gate->decided, g.thr = gate->threshold;
    if (old_values) hipLaunchKernelGGL((ppo_rows<true, true>), rows_grid, dim3(kPolicyThreads), h->lds_bytes, pol->stream, t);
    else hipLaunchKernelGGL((ppo_rows<false, true>), rows_grid, dim3(kPolicyThreads), h->lds_bytes, pol->stream, t);
    FLEET_HANDLE_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(ppo_weights<true>, weights_grid, dim3(256), 0, pol->stream, g);
    FLEET_HANDLE_TRY(h, hipGetLastError());
    return FLEET_OK;
  }
  if (old_values) hipLaunchKernelGGL(ppo_rows<true>, rows_grid, dim3(kPolicyThreads), h->lds_bytes, pol->stream, static_cast<const RowsArgsVclip&>(t));
  else hipLaunchKernelGGL(ppo_rows<false>, rows_grid, dim3(kPolicyThreads), h->lds_bytes, pol->stream, static_cast<const RowsArgs&>(t));
  FLEET_HANDLE_TRY(h, hipGetLastError());
  hipLaunchKernelGGL(ppo_weights<false>, weights_grid, dim3(256), 0, pol->stream, static_cast<const WeightArgs&>(g));
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_ppo_grad_dev(fleet_ppo_handle h, const FleetPpoGradArgs* args, float* const* grads, int count) {
  std::string why = check_grad_args(args, grads, count);
  if (h && why.empty()) grad_check_sizes(&why, count, h->img->n_tensors + 1, "W, b per layer, then log_std", args->B, h->p.max_batch);
  if (const int rc = handle_enter("fleet_ppo_grad_dev", why, h, g_ppo_error); rc != FLEET_OK) return rc;
  return ppo_grad_launch(h, *args, nullptr, 0.0f, grads, count);
}

int fleet_ppo_grad_vclip_dev(fleet_ppo_handle h, const FleetPpoGradVclipArgs* args, float* const* grads, int count) {
  std::string why = check_vclip_args(args, grads, count);
  if (h && why.empty()) grad_check_sizes(&why, count, h->img->n_tensors + 1, "W, b per layer, then log_std", args->base.B, h->p.max_batch);
  if (const int rc = handle_enter("fleet_ppo_grad_vclip_dev", why, h, g_ppo_error); rc != FLEET_OK) return rc;
  return ppo_grad_launch(h, args->base, args->old_values, args->clip_range_vf, grads, count);
}

int fleet_ppo_grad_gated_dev(fleet_ppo_handle h, const FleetPpoGradGatedArgs* args, float* const* grads, int count) {
  std::string why = check_gated_args(args, grads, count);
  if (h && why.empty()) grad_check_sizes(&why, count, h->img->n_tensors + 1, "W, b per layer, then log_std", args->base.B, h->p.max_batch);
  if (const int rc = handle_enter("fleet_ppo_grad_gated_dev", why, h, g_ppo_error); rc != FLEET_OK) return rc;
  const bool vclip = args->clip_range_vf > 0.0f;
  return ppo_grad_launch(h, args->base, vclip ? args->old_values : nullptr, args->clip_range_vf, grads, count, &args->gate);
}

}  // extern "C"
