// fleet_adam.hip -- clip_grad_norm_ and torch.optim.Adam's step on the device, writing every new weight to torch's parameter AND to the
// weight image it was created on (include/fleet_hip.h "Adam and clip_grad_norm_ on the device"; fleet_adam.h, fleet_mlp.h): what a
// gradient step did with about ten foreach launches, several multi-tensor launches and a *_load_dev, in TWO launches.  The handle
// borrows the image of a fleet_policy or a fleet_qtarget handle and owns one block: exp_avg and exp_avg_sq of every tensor in torch's
// layout, the norm's partial sums, and the three tables of fleet_adam.h.
//   adam_norm  grid (chunks), 256 threads.  A chunk is 1024 consecutive elements of one gradient tensor (the last chunk of a tensor is
//              short: a chunk never straddles two tensors).  Thread t: acc = 0; acc = fmaf(g, g, acc) over elements 4t .. 4t + 3 in
//              ascending order (those past the tensor's end are skipped); an xor butterfly over the wavefront, offsets 32, 16, 8, 4, 2, 1
//              (every lane ends with the same bits: a + b is b + a); the four wavefronts' sums added in wave order by thread 0 ->
//              part[chunk].  Scalar loads only: the bits do not depend on a tensor's alignment.
//   adam_step  grid (work items), 256 threads.  Every workgroup adds part[] in float64 in ascending order, norm = (float)sqrt(sum),
//              and forms the clip coefficient from it: all workgroups hold the same bits with no ordering between them.  Workgroup 0
//              writes norm_out.  Then one work item: a 32 x 32 tile of a W -- g, m, v, p read and m', v', p' written with lanes along
//              `in`, p' also into tile[32][33] in the LDS, and after the barrier into Wt[k][j] of the image with lanes along `out` --
//              or 1024 elements of a bias (p' to b[j] of the image too) or of an extra.  Only real elements are visited: the image's
//              zero padding stays what create made it.
// No atomics, no ordering between workgroups: the launch boundary between the two is the only one.  float32 but for the sum above.
// The gated instances (kGated; fleet_adam_step_gated_dev launches them, the others keep their text and their code): every workgroup
// of both launches reads the word `skip` once at its top, one uniform load and a scalar branch, and returns when it is set, having
// written nothing -- no parameter, no moment, no image word, no part[], no norm_out.  An EARLIER launch wrote that word: no launch
// reads a word that a workgroup of the same launch may write.
// The step count lives on the host.  After a gated train call only the device knows how many steps ran: fleet_adam_settle_dev copies
// that word to a pinned host word behind everything enqueued and records an event; every entry that reads or writes the count waits
// for that event first (adam_settle, below).  No kernel writes host memory.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "fleet_adam.h"
#include "fleet_policy.h"
#include "fleet_qtarget.h"

namespace {

struct NormArgs {
  const float* g[kAdamMaxTensors];
  const AdamTensor* tensors;
  const AdamChunk* chunks;
  float* part;
};

struct NormArgsGated : NormArgs {
  const uint32_t* skip;  // nonzero: the launch returns at once
};

template <bool kGated>
__global__ __launch_bounds__(kAdamThreads) void adam_norm(std::conditional_t<kGated, NormArgsGated, NormArgs> a) {
  if constexpr (kGated) {
    if (__builtin_amdgcn_readfirstlane(*a.skip)) return;
  }
  __shared__ float ws[kAdamThreads / 64];
  const AdamChunk ch = a.chunks[blockIdx.x];
  const int t = __builtin_amdgcn_readfirstlane(ch.tensor);
  const float* __restrict__ g = a.g[t];
  const uint32_t len = a.tensors[t].len;
  const uint32_t i0 = ch.start + 4u * threadIdx.x;  // (start < len <= 2^24 + ...: no wrap)
  float acc = 0.0f;
#pragma unroll
  for (uint32_t e = 0; e < 4; ++e)
    if (i0 + e < len) {
      const float x = g[i0 + e];
      acc = fmaf(x, x, acc);
    }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

struct StepArgs {
  float* p[kAdamMaxTensors];
  const float* g[kAdamMaxTensors];
  const AdamTensor* tensors;
  const AdamItem* items;
  const float* part;
  float* block;  // exp_avg of tensor t at block + tensors[t].state_off, its exp_avg_sq n_elements behind
  float* image;  // the borrowed weight image
  float* norm_out;
  uint64_t n_elements;
  int n_chunks;  // of the norm launch that ran before this one; 0: none did
  int clip;
  float maxn, omb1, omb2, b2, nstep, bs, eps;
};

struct AdamCoef {
  float c, omb1, omb2, b2, nstep, bs, eps;
  int clip;
};

// one element: the header's four lines; returns p'
__device__ __forceinline__ float adam_element(float g, float* __restrict__ m, float* __restrict__ v, float p, const AdamCoef& k) {
  if (k.clip) g = g * k.c;
  const float m0 = *m, v0 = *v;
  const float m1 = fmaf(g - m0, k.omb1, m0);
  const float v1 = fmaf(g * k.omb2, g, v0 * k.b2);
  const float den = sqrtf(v1) / k.bs + k.eps;
  *m = m1, *v = v1;
  return fmaf(m1 / den, k.nstep, p);
}

struct StepArgsGated : StepArgs {
  const uint32_t* skip;  // nonzero: the launch returns at once
};

template <bool kGated>
__global__ __launch_bounds__(kAdamThreads) void adam_step(std::conditional_t<kGated, StepArgsGated, StepArgs> a) {
  if constexpr (kGated) {
    if (__builtin_amdgcn_readfirstlane(*a.skip)) return;
  }
  __shared__ float tile[kAdamTile][kAdamTile + 1];
  AdamCoef k{1.0f, a.omb1, a.omb2, a.b2, a.nstep, a.bs, a.eps, a.clip};
  if (a.n_chunks > 0) {
    const float* __restrict__ part = a.part;
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < a.n_chunks; ++i) s += (double)part[i];
    const float norm = (float)sqrt(s);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.norm_out) *a.norm_out = norm;
    const float q = a.maxn / (norm + 1e-6f);
    k.c = q > 1.0f ? 1.0f : q;  // (a NaN stays a NaN, as torch.clamp keeps it)
  }
  const AdamItem it = a.items[blockIdx.x];
  const int t = __builtin_amdgcn_readfirstlane(it.tensor);
  const AdamTensor T = a.tensors[t];
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.block + T.state_off;
  float* __restrict__ v = m + a.n_elements;
  if (T.kind == kAdamMatrix) {
    const uint32_t tx = threadIdx.x % kAdamTile, ty = threadIdx.x / kAdamTile;
    constexpr uint32_t kPass = kAdamThreads / kAdamTile;  // rows of the tile one pass covers
    const uint32_t kcol = it.k0 + tx;
#pragma unroll
    for (uint32_t r = 0; r < kAdamTile / kPass; ++r) {
      const uint32_t jj = ty + kPass * r, j = it.j0 + jj;
      if (j < (uint32_t)T.out && kcol < (uint32_t)T.in) {
        const size_t i = (size_t)j * T.in + kcol;
        const float pn = adam_element(g[i], m + i, v + i, p[i], k);
        p[i] = pn;
        tile[jj][tx] = pn;
      }
    }
    __syncthreads();
    float* __restrict__ Wt = a.image + T.img_off;
    const uint32_t jo = it.j0 + tx;
#pragma unroll
    for (uint32_t r = 0; r < kAdamTile / kPass; ++r) {
      const uint32_t kk = ty + kPass * r, ki = it.k0 + kk;
      if (jo < (uint32_t)T.out && ki < (uint32_t)T.in) Wt[(size_t)ki * T.out64 + jo] = tile[tx][kk];
    }
  } else {
    float* __restrict__ b = a.image + T.img_off;
#pragma unroll
    for (uint32_t r = 0; r < kAdamChunk / kAdamThreads; ++r) {
      const uint32_t i = it.j0 + threadIdx.x + kAdamThreads * r;
      if (i < T.len) {
        const float pn = adam_element(g[i], m + i, v + i, p[i], k);
        p[i] = pn;
        if (T.kind == kAdamBias) b[i] = pn;
      }
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_adam_error;  // of the last failed call without a handle

const std::string kArgsLater;  // fleet_adam_export_image_dev's reason: mlp_launch_relay looks at its arguments

constexpr int32_t kMaxExtraLen = 1 << 24;

std::string check_params(const FleetAdamParams* p) {
  if (!p) return "null FleetAdamParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetAdamParams)) return "FleetAdamParams.struct_bytes does not match this library";
  if (p->first_net < 0 || p->n_nets < 0 || p->first_net > kMlpMaxNets || p->n_nets > kMlpMaxNets)
    return "the span of nets " + std::to_string(p->first_net) + " .. +" + std::to_string(p->n_nets) + " lies outside every image";
  if (p->n_extra < 0 || p->n_extra > FLEET_ADAM_MAX_EXTRA)
    return "n_extra must be in 0.." + std::to_string(FLEET_ADAM_MAX_EXTRA) + ", got " + std::to_string(p->n_extra);
  for (int i = 0; i < p->n_extra; ++i)
    if (p->extra_len[i] < 1 || p->extra_len[i] > kMaxExtraLen)
      return "extra_len[" + std::to_string(i) + "] must be in 1.." + std::to_string(kMaxExtraLen) + ", got " + std::to_string(p->extra_len[i]);
  if (p->n_nets == 0 && p->n_extra == 0) return "nothing to optimise: n_nets and n_extra are both 0";
  return "";
}

// what fleet_adam_step_dev refuses, looked at without the handle; "" when the arguments pass
std::string check_step_args(const FleetAdamStepArgs* x, float* const* params, float* const* grads, int count) {
  if (!x) return "null FleetAdamStepArgs";
  if (x->struct_bytes != (int32_t)sizeof(FleetAdamStepArgs)) return "FleetAdamStepArgs.struct_bytes does not match this library";
  if (!std::isfinite(x->lr) || x->lr < 0.0) return "lr must be finite and >= 0";
  if (!std::isfinite(x->eps) || x->eps < 0.0) return "eps must be finite and >= 0";
  if (!(x->beta1 >= 0.0 && x->beta1 < 1.0)) return "beta1 must be in [0, 1)";
  if (!(x->beta2 >= 0.0 && x->beta2 < 1.0)) return "beta2 must be in [0, 1)";
  if (std::isnan(x->max_grad_norm)) return "max_grad_norm is NaN";
  if (!params) return "null params";
  if (!grads) return "null grads";
  if (count < 1 || count > kAdamMaxTensors) return "count must be in 1.." + std::to_string(kAdamMaxTensors) + ", got " + std::to_string(count);
  for (int i = 0; i < count; ++i) {
    if (!params[i]) return "parameter tensor " + std::to_string(i) + " is null";
    if (!grads[i]) return "gradient tensor " + std::to_string(i) + " is null";
    if (params[i] == grads[i]) return "parameter tensor " + std::to_string(i) + " is its own gradient";
  }
  return "";
}

std::string check_state_args(int mode, float* const* exp_avg, float* const* exp_avg_sq, int count, const int64_t* step) {
  if (mode != FLEET_ADAM_STATE_EXPORT && mode != FLEET_ADAM_STATE_LOAD) return "unknown mode " + std::to_string(mode);
  if (!exp_avg) return "null exp_avg";
  if (!exp_avg_sq) return "null exp_avg_sq";
  if (!step) return "null step";
  if (count < 1 || count > kAdamMaxTensors) return "count must be in 1.." + std::to_string(kAdamMaxTensors) + ", got " + std::to_string(count);
  for (int i = 0; i < count; ++i) {
    if (!exp_avg[i]) return "exp_avg tensor " + std::to_string(i) + " is null";
    if (!exp_avg_sq[i]) return "exp_avg_sq tensor " + std::to_string(i) + " is null";
  }
  if (mode == FLEET_ADAM_STATE_LOAD && *step < 0) return "step must be >= 0, got " + std::to_string(*step);
  return "";
}

}  // namespace

struct FleetAdam : FleetMlpUser {  // img: either family's; block: the state, the norm's partial sums, the tables
  FleetAdamParams p{};
  std::vector<AdamTensor> tensors;
  uint64_t n_elements = 0;
  int n_chunks = 0, n_items = 0;
  int64_t step = 0;  // on the host, as torch's non-capturable Adam keeps it
  const AdamTensor* d_tensors = nullptr;
  const AdamChunk* d_chunks = nullptr;
  const AdamItem* d_items = nullptr;
  float* d_part = nullptr;
  // a settlement (fleet_adam_settle_dev): once `settle_event` has completed, step = settle_base + *settle_word
  uint32_t* settle_word = nullptr;  // pinned host memory, owned
  hipEvent_t settle_event = nullptr;
  int64_t settle_base = 0;
  bool settle_pending = false;
  ~FleetAdam();  // (out of line, below: the one place that takes the tables down)
};
FleetAdam::~FleetAdam() = default;

namespace {

// what the step and the state entries refuse once they have their handle
void check_count(std::string* why, int count, const FleetAdam* h) {
  if (count != (int)h->tensors.size())
    *why = "expected " + std::to_string(h->tensors.size()) + " tensors (W, b per layer, net after net, then the extras), got " + std::to_string(count);
}

// Settling on use: what every entry that reads or writes h->step calls first.  A pending settlement is waited for (in a training
// loop a whole rollout lies between two updates: the event completed long ago) and fixes the count.
int adam_settle(FleetAdam* h) {
  if (!h->settle_pending) return FLEET_OK;
  FLEET_HANDLE_TRY(h, hipEventSynchronize(h->settle_event));
  h->step = h->settle_base + (int64_t)*h->settle_word;
  h->settle_pending = false;
  return FLEET_OK;
}

// a stream that is being captured cannot take the settlement's event wait: the gated entries refuse it
int adam_refuse_capture(const char* entry, FleetAdam* h) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  FLEET_HANDLE_TRY(h, hipStreamIsCapturing(h->img->stream, &st));
  if (st == hipStreamCaptureStatusNone) return FLEET_OK;
  h->error = std::string(entry) + ": the image handle's stream is capturing a graph; a step count that the device decides cannot be captured";
  return FLEET_ERR_STATE;
}

int adam_create(const char* entry, const char* noun, void* image, size_t record_bytes, const FleetAdamParams* p, fleet_adam_handle* out) {
  if (out) *out = nullptr;
  std::string why = check_params(p);
  if (why.empty() && !out) why = "null output handle";
  FleetMlpHandle* img = why.empty() ? mlp_borrow(image, record_bytes, noun, &why) : nullptr;
  if (img && p->first_net + p->n_nets > img->n_nets)
    why = "the span of nets " + std::to_string(p->first_net) + " .. " + std::to_string(p->first_net + p->n_nets - 1) +
          " lies outside the image's " + std::to_string(img->n_nets) + " nets";
  if (!why.empty()) return handle_refuse(g_adam_error, entry, why, FLEET_ERR_INVALID);
  FleetAdam* h = new FleetAdam();
  h->p = *p;
  uint64_t off = 0;
  const auto add = [&](int kind, int out_, int in_, int out64, uint32_t img_off) {
    AdamTensor T{};
    T.kind = kind, T.out = out_, T.in = in_, T.out64 = out64, T.img_off = img_off;
    T.len = (uint32_t)out_ * (uint32_t)in_;  // (<= 8192 * 512, or an extra's <= 2^24)
    T.state_off = off;
    off += T.len;
    h->tensors.push_back(T);
  };
  for (int nt = p->first_net; nt < p->first_net + p->n_nets; ++nt)
    for (int l = 0; l < img->nets[nt].n_layers; ++l) {
      const PolicyLayer& L = img->nets[nt].layer[l];
      add(kAdamMatrix, L.out, L.in, L.out64, L.w_off);
      add(kAdamBias, L.out, 1, L.out64, L.b_off);
    }
  for (int i = 0; i < p->n_extra; ++i) add(kAdamExtra, p->extra_len[i], 1, 0, 0);
  h->n_elements = off;
  std::vector<AdamChunk> chunks;
  std::vector<AdamItem> items;
  for (int t = 0; t < (int)h->tensors.size(); ++t) {
    const AdamTensor& T = h->tensors[t];
    for (uint32_t s = 0; s < T.len; s += kAdamChunk) chunks.push_back(AdamChunk{t, s});
    if (T.kind == kAdamMatrix) {
      for (uint32_t j0 = 0; j0 < (uint32_t)T.out; j0 += kAdamTile)
        for (uint32_t k0 = 0; k0 < (uint32_t)T.in; k0 += kAdamTile) items.push_back(AdamItem{t, j0, k0, 0});
    } else {
      for (uint32_t s = 0; s < T.len; s += kAdamChunk) items.push_back(AdamItem{t, s, 0, 0});
    }
  }
  h->n_chunks = (int)chunks.size(), h->n_items = (int)items.size();
  // the block: exp_avg [n], exp_avg_sq [n], part [chunks], then the tables at multiples of 16 bytes
  const auto up16 = [](uint64_t b) { return (b + 15) / 16 * 16; };
  const uint64_t state_bytes = 2 * h->n_elements * sizeof(float);
  const uint64_t part_at = state_bytes, tensors_at = up16(part_at + chunks.size() * sizeof(float));
  const uint64_t chunks_at = up16(tensors_at + h->tensors.size() * sizeof(AdamTensor));
  const uint64_t items_at = up16(chunks_at + chunks.size() * sizeof(AdamChunk));
  const uint64_t total = items_at + items.size() * sizeof(AdamItem);
  std::vector<char> tables(total - tensors_at, 0);
  memcpy(tables.data(), h->tensors.data(), h->tensors.size() * sizeof(AdamTensor));
  memcpy(tables.data() + (chunks_at - tensors_at), chunks.data(), chunks.size() * sizeof(AdamChunk));
  memcpy(tables.data() + (items_at - tensors_at), items.data(), items.size() * sizeof(AdamItem));
  int rc = mlp_user_open(h, img, total, "optimiser", {}, "", &why);
  // a zero state and the tables, waited for: the first step may come on any stream
  if (rc == FLEET_OK && (hipMemset(h->block, 0, tensors_at) != hipSuccess ||
                         hipMemcpy(h->block + tensors_at, tables.data(), tables.size(), hipMemcpyHostToDevice) != hipSuccess ||
                         hipDeviceSynchronize() != hipSuccess)) {
    (void)hipGetLastError();
    why = "clearing the optimiser's state failed", rc = FLEET_ERR_HIP;
  }
  if (rc != FLEET_OK) {
    fleet_adam_destroy(h);
    return handle_refuse(g_adam_error, entry, why, rc);
  }
  h->d_part = reinterpret_cast<float*>(h->block + part_at);
  h->d_tensors = reinterpret_cast<const AdamTensor*>(h->block + tensors_at);
  h->d_chunks = reinterpret_cast<const AdamChunk*>(h->block + chunks_at);
  h->d_items = reinterpret_cast<const AdamItem*>(h->block + items_at);
  *out = h;
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_adam_create_policy(fleet_policy_handle policy, const FleetAdamParams* p, fleet_adam_handle* out) {
  return adam_create("fleet_adam_create_policy", "policy", policy, sizeof(PolicyDesc), p, out);
}

int fleet_adam_create_qtarget(fleet_qtarget_handle nets, const FleetAdamParams* p, fleet_adam_handle* out) {
  return adam_create("fleet_adam_create_qtarget", "networks", nets, sizeof(QTargetDesc), p, out);
}

int fleet_adam_destroy(fleet_adam_handle h) {
  if (!h) return FLEET_OK;
  mlp_user_close(h);  // (waits for the device: a settlement's copy has landed)
  if (h->settle_event) (void)hipEventDestroy(h->settle_event);
  if (h->settle_word) (void)hipHostFree(h->settle_word);
  delete h;
  return FLEET_OK;
}

const char* fleet_adam_last_error(fleet_adam_handle h) { return h ? h->error.c_str() : g_adam_error.c_str(); }

int fleet_adam_describe(fleet_adam_handle h, FleetAdamParams* out, FleetAdamInfo* info) {
  if (!h || !out || !info) return FLEET_ERR_INVALID;
  if (const int rc = adam_settle(h); rc != FLEET_OK) return rc;
  *out = h->p;
  info->state_bytes = 2 * h->n_elements * sizeof(float);
  info->n_elements = h->n_elements;
  info->step = h->step;
  info->n_tensors = (int32_t)h->tensors.size();
  info->norm_chunk = kAdamChunk;
  info->step_tile = kAdamTile;
  info->reserved = 0;
  return FLEET_OK;
}

}  // extern "C"

namespace {

// both step entries; skip null: the ungated instances
int adam_step_launch(const char* entry, fleet_adam_handle h, std::string why, const FleetAdamStepArgs* x, float* const* params,
                     float* const* grads, int count, const uint32_t* skip) {
  if (h && why.empty()) check_count(&why, count, h);
  if (const int rc = handle_enter(entry, why, h, g_adam_error); rc != FLEET_OK) return rc;
  if (const int rc = adam_settle(h); rc != FLEET_OK) return rc;
  FleetMlpHandle* img = h->img;
  const bool clip = x->max_grad_norm > 0.0, norm = clip || x->norm_out;
  // the scalars in double, as torch's Python forms them, then rounded
  const double t = (double)(h->step + 1);
  const double bc1 = 1.0 - std::pow(x->beta1, t), bc2 = 1.0 - std::pow(x->beta2, t);
  StepArgsGated s{};
  s.skip = skip;
  for (int i = 0; i < count; ++i) s.p[i] = params[i], s.g[i] = grads[i];
  s.tensors = h->d_tensors, s.items = h->d_items, s.part = h->d_part;
  s.block = reinterpret_cast<float*>(h->block), s.image = reinterpret_cast<float*>(img->block), s.norm_out = x->norm_out;
  s.n_elements = h->n_elements, s.n_chunks = norm ? h->n_chunks : 0, s.clip = clip ? 1 : 0;
  s.maxn = (float)x->max_grad_norm, s.omb1 = (float)(1.0 - x->beta1), s.omb2 = (float)(1.0 - x->beta2), s.b2 = (float)x->beta2;
  s.nstep = (float)-(x->lr / bc1), s.bs = (float)std::sqrt(bc2), s.eps = (float)x->eps;
  FLEET_HANDLE_TRY(h, hipSetDevice(img->device));
  if (norm) {
    NormArgsGated n{};
    n.skip = skip;
    for (int i = 0; i < count; ++i) n.g[i] = grads[i];
    n.tensors = h->d_tensors, n.chunks = h->d_chunks, n.part = h->d_part;
    if (skip) hipLaunchKernelGGL(adam_norm<true>, dim3((unsigned)h->n_chunks), dim3(kAdamThreads), 0, img->stream, n);
    else hipLaunchKernelGGL(adam_norm<false>, dim3((unsigned)h->n_chunks), dim3(kAdamThreads), 0, img->stream, static_cast<const NormArgs&>(n));
    FLEET_HANDLE_TRY(h, hipGetLastError());
  }
  if (skip) hipLaunchKernelGGL(adam_step<true>, dim3((unsigned)h->n_items), dim3(kAdamThreads), 0, img->stream, s);
  else hipLaunchKernelGGL(adam_step<false>, dim3((unsigned)h->n_items), dim3(kAdamThreads), 0, img->stream, static_cast<const StepArgs&>(s));
  FLEET_HANDLE_TRY(h, hipGetLastError());
  h->step += 1;
  return FLEET_OK;
}

}  // namespace

extern "C" {

int fleet_adam_step_dev(fleet_adam_handle h, const FleetAdamStepArgs* x, float* const* params, float* const* grads, int count) {
  return adam_step_launch("fleet_adam_step_dev", h, check_step_args(x, params, grads, count), x, params, grads, count, nullptr);
}

int fleet_adam_step_gated_dev(fleet_adam_handle h, const FleetAdamStepArgs* x, float* const* params, float* const* grads, int count,
                              const uint32_t* skip) {
  std::string why = check_step_args(x, params, grads, count);
  if (why.empty() && !skip) why = "null skip";
  return adam_step_launch("fleet_adam_step_gated_dev", h, why, x, params, grads, count, skip);
}

int fleet_adam_settle_dev(fleet_adam_handle h, int64_t base_step, const uint32_t* steps_taken) {
  std::string why;
  if (base_step < 0) why = "base_step must be >= 0, got " + std::to_string(base_step);
  else if (!steps_taken) why = "null steps_taken";
  if (const int rc = handle_enter("fleet_adam_settle_dev", why, h, g_adam_error); rc != FLEET_OK) return rc;
  if (const int rc = adam_settle(h); rc != FLEET_OK) return rc;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->img->device));
  if (const int rc = adam_refuse_capture("fleet_adam_settle_dev", h); rc != FLEET_OK) return rc;
  if (!h->settle_word) FLEET_HANDLE_TRY(h, hipHostMalloc(reinterpret_cast<void**>(&h->settle_word), sizeof(uint32_t), hipHostMallocDefault));
  if (!h->settle_event) FLEET_HANDLE_TRY(h, hipEventCreateWithFlags(&h->settle_event, hipEventDisableTiming));
  FLEET_HANDLE_TRY(h, hipMemcpyAsync(h->settle_word, steps_taken, sizeof(uint32_t), hipMemcpyDeviceToHost, h->img->stream));
  FLEET_HANDLE_TRY(h, hipEventRecord(h->settle_event, h->img->stream));
  h->settle_base = base_step, h->settle_pending = true;
  return FLEET_OK;
}

int fleet_adam_state_dev(fleet_adam_handle h, int mode, float* const* exp_avg, float* const* exp_avg_sq, int count, int64_t* step) {
  std::string why = check_state_args(mode, exp_avg, exp_avg_sq, count, step);
  if (h && why.empty()) check_count(&why, count, h);
  if (const int rc = handle_enter("fleet_adam_state_dev", why, h, g_adam_error); rc != FLEET_OK) return rc;
  if (const int rc = adam_settle(h); rc != FLEET_OK) return rc;
  FleetMlpHandle* img = h->img;
  FLEET_HANDLE_TRY(h, hipSetDevice(img->device));
  float* base = reinterpret_cast<float*>(h->block);
  for (int i = 0; i < count; ++i) {
    const AdamTensor& T = h->tensors[i];
    float *m = base + T.state_off, *v = m + h->n_elements;
    const size_t bytes = (size_t)T.len * sizeof(float);
    if (mode == FLEET_ADAM_STATE_EXPORT) {
      FLEET_HANDLE_TRY(h, hipMemcpyAsync(exp_avg[i], m, bytes, hipMemcpyDeviceToDevice, img->stream));
      FLEET_HANDLE_TRY(h, hipMemcpyAsync(exp_avg_sq[i], v, bytes, hipMemcpyDeviceToDevice, img->stream));
    } else {
      FLEET_HANDLE_TRY(h, hipMemcpyAsync(m, exp_avg[i], bytes, hipMemcpyDeviceToDevice, img->stream));
      FLEET_HANDLE_TRY(h, hipMemcpyAsync(v, exp_avg_sq[i], bytes, hipMemcpyDeviceToDevice, img->stream));
    }
  }
  if (mode == FLEET_ADAM_STATE_EXPORT) *step = h->step;
  else h->step = *step;
  return FLEET_OK;
}

int fleet_adam_export_image_dev(fleet_adam_handle h, float* const* tensors, int count) {
  if (const int rc = handle_enter("fleet_adam_export_image_dev", kArgsLater, h, g_adam_error); rc != FLEET_OK) return rc;
  const int rc = mlp_launch_relay(h->img, kMlpExport, "fleet_adam_export_image_dev", tensors, count, 0.0f, 0.0f);
  if (rc != FLEET_OK) h->error = h->img->error;
  return rc;
}

}  // extern "C"
