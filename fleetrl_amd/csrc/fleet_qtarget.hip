// fleet_qtarget.hip -- the target networks of a TD3 / DDPG agent on the device (include/fleet_hip.h "TD3 / DDPG learning targets on
// the device"): the bootstrap target of a minibatch in one launch, the Polyak update in one launch, loads and the export.
//
// One allocation holds the record (QTargetDesc) and every layer's weights of the actor, critic 0 and critic 1, laid out as the
// policy's are (PolicyLayer, fleet_policy.h).  Two kernels:
//   qtarget_target  grid ceil(B / 16).  A workgroup of 256 threads takes 16 rows through the ACTOR with the layer functions of
//                   fleet_policy_dev.h; its last layer leaves the rows untransformed in the LDS, act[16][A64], as
//                   policy_forward_sample's does.  An epilogue phase -- one thread per (row, 4 columns) -- turns them into the
//                   target action a' in place.  The SAME workgroup then runs critic 0 and critic 1, one after the other: their first
//                   layer stages its input 128 columns at a time, columns below D from next_obs in global memory, columns D .. D+A-1
//                   from act[][] in the LDS, zeros behind.  A critic's last layer (64 padded columns) goes to the activation buffer
//                   its layer before did not read; threads 0..15 pick column 0 of their row up into a register.  The final phase
//                   is those 16 threads: q, qmin, y.
//                   LDS: two activation buffers [16][S], S the widest hidden layer of all three networks, the staged chunk
//                   [16][128], act [16][A64]: 20 KiB .. 104 KiB.
//   qtarget_relay   grid (64, tensors): load (torch's [out, in] -> the image), polyak (the same walk, t' = fmaf(tau, p, t * omt)) and
//                   export (the image -> torch's layout).  Only real elements are visited: the padding stays what create made it.
// Launch boundaries are the only visibility mechanism; no atomics.  float32 throughout.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fleet_handle.h"
#include "fleet_philox.h"
#include "fleet_policy.h"
#include "fleet_policy_dev.h"

namespace {

constexpr int kQNets = 3;  // actor, critic 0, critic 1
constexpr int kQTensors = 2 * kQNets * FLEET_POLICY_MAX_LAYERS;

struct QTargetDesc {
  int32_t obs_dim, act_dim, n_critics;
  int32_t stride;  // floats between rows of an activation buffer: the widest hidden layer's out64 over all networks (64 without one)
  int32_t act64;   // floats between rows of act[][]: the actor's last out64
  int32_t reserved[3];
  PolicyHeadDesc net[kQNets];
};

struct TargetArgs {
  const QTargetDesc* desc;
  const float* base;
  const float *next_obs, *rewards, *dones, *sigma;
  float *noise, *target_q, *next_actions, *q;
  uint64_t seed, step;
  uint32_t row_id0;  // global id of row 0
  int given, B;
  float gamma, noise_clip, lo, hi;
};

// act[16][M]: the actor's last layer before its transform -> a' in place; the optional noise and next_actions
__device__ __forceinline__ void action_epilogue(const TargetArgs& t, const PolicyHeadDesc* H, float* act, int M, int A, int row0) {
  const int nb = (A + 3) / 4;  // Philox blocks per row
  const int output = H->output;
  const float hlo = H->lo, hhi = H->hi;
  const float nlo = -t.noise_clip, nhi = t.noise_clip;
  for (int item = threadIdx.x; item < kPolicyRows * nb; item += kPolicyThreads) {
    const int r = item / nb, b = item - r * nb;
    const int row = row0 + r;
    if (row >= t.B) continue;  // (such a row keeps the untransformed numbers: the critics run on them and nobody reads the result)
    const size_t o = (size_t)row * A;
    float z[4];
    if (t.given) {
#pragma unroll
      for (int c = 0; c < 4; ++c) z[c] = 4 * b + c < A ? t.noise[o + 4 * b + c] : 0.0f;
    } else {
      uint32_t w[4];
      philox4x32_10(t.row_id0 + (uint32_t)row, (uint32_t)b, (uint32_t)t.step, (uint32_t)(t.step >> 32), (uint32_t)t.seed,
                    (uint32_t)(t.seed >> 32), w);
      normals4(w, z);
    }
    const float4 m4 = *reinterpret_cast<const float4*>(act + r * M + 4 * b);  // (M is a multiple of 64: aligned, inside the row)
    const float mz[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = 4 * b + c;
      if (j >= A) break;
      const float eps = z[c];
      if (!t.given && t.noise) t.noise[o + j] = eps;
      const float d = output_of(mz[c], output, hlo, hhi);
      float n = t.sigma[j] * eps;
      n = n < nlo ? nlo : (n > nhi ? nhi : n);
      float v = d + n;
      v = v < t.lo ? t.lo : (v > t.hi ? t.hi : v);
      act[r * M + j] = v;
      if (t.next_actions) t.next_actions[o + j] = v;
    }
  }
}

__global__ __launch_bounds__(kPolicyThreads) void qtarget_target(TargetArgs t) {
  extern __shared__ float lds[];  // two activation buffers [16][S], the staged input [16][kPolicyChunk], act [16][M]
  const QTargetDesc* __restrict__ d = t.desc;
  const int S = d->stride, D = d->obs_dim, A = d->act_dim, M = d->act64, nc = d->n_critics;
  float *buf0 = lds, *buf1 = lds + kPolicyRows * S, *xs = lds + 2 * kPolicyRows * S;
  float* act = xs + kPolicyRows * kPolicyChunk;
  const int row0 = blockIdx.x * kPolicyRows;
  ForwardArgs a{};
  a.base = t.base, a.obs = t.next_obs, a.E = t.B;
  run_head<kStagePlain, true>(a, &d->net[0], buf0, buf1, xs, S, row0, nullptr, act, StageTail{});
  action_epilogue(t, &d->net[0], act, M, A, row0);
  __syncthreads();
  const StageTail tail{act, M, D};
  float q0 = 0.0f, q1 = 0.0f;
  {
    const PolicyHeadDesc* H = &d->net[1];
    float* qrows = (H->n_layers - 1) & 1 ? buf0 : buf1;  // the buffer the last layer does not read (run_head)
    run_head<kStageConcat, true>(a, H, buf0, buf1, xs, S, row0, nullptr, qrows, tail);
    if (threadIdx.x < kPolicyRows) q0 = qrows[threadIdx.x * 64];  // (before the next head's first barrier: nobody has written yet)
  }
  if (nc == 2) {
    const PolicyHeadDesc* H = &d->net[2];
    float* qrows = (H->n_layers - 1) & 1 ? buf0 : buf1;
    run_head<kStageConcat, true>(a, H, buf0, buf1, xs, S, row0, nullptr, qrows, tail);
    if (threadIdx.x < kPolicyRows) q1 = qrows[threadIdx.x * 64];
  }
  const int row = row0 + (int)threadIdx.x;
  if (threadIdx.x < kPolicyRows && row < t.B) {
    if (t.q) {
      t.q[(size_t)row * nc] = q0;
      if (nc == 2) t.q[(size_t)row * nc + 1] = q1;
    }
    const float qmin = nc == 2 ? (q1 < q0 ? q1 : q0) : q0;
    const float keep = (1.0f - t.dones[row]) * t.gamma;
    const float boot = keep * qmin;  // (its own rounding: -ffp-contract=off, and no fmaf here)
    t.target_q[row] = t.rewards[row] + boot;
  }
}

// ---- qtarget_relay ---------------------------------------------------------------------------------------------------------------
constexpr int kRelayLoad = 0, kRelayPolyak = 1, kRelayExport = 2;
struct QRelayArgs {
  float* tensor[kQTensors];  // (read in the load and polyak modes, written in the export mode)
  const QTargetDesc* desc;
  float* base;
  float tau, omt;
};

// tensor blockIdx.y (W, b per layer; actor, critic 0, critic 1): W[out][in] <-> Wt[in][out64], b <-> b
template <int kMode>
__global__ __launch_bounds__(256) void qtarget_relay(QRelayArgs a) {
  const QTargetDesc* __restrict__ d = a.desc;
  int t = blockIdx.y, net = 0;
  while (net < kQNets - 1 && t >= 2 * d->net[net].n_layers) t -= 2 * d->net[net++].n_layers;
  const PolicyLayer L = d->net[net].layer[t >> 1];
  float* __restrict__ ext = a.tensor[blockIdx.y];
  const unsigned stride = gridDim.x * 256, gid = blockIdx.x * 256 + threadIdx.x;
  const unsigned count = t & 1 ? (unsigned)L.out : (unsigned)L.in * (unsigned)L.out;  // <= 8192 * 512
  for (unsigned i = gid; i < count; i += stride) {
    size_t img, e;
    if (t & 1) {
      img = L.b_off + i, e = i;
    } else {
      const unsigned k = i / (unsigned)L.out, j = i - k * (unsigned)L.out;
      img = L.w_off + (size_t)k * L.out64 + j, e = (size_t)j * L.in + k;
    }
    if (kMode == kRelayLoad) a.base[img] = ext[e];
    else if (kMode == kRelayExport) ext[e] = a.base[img];
    else a.base[img] = fmaf(a.tau, ext[e], a.base[img] * a.omt);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
thread_local std::string g_qtarget_error;  // of the last failed call without a handle

std::string validate(const FleetQTargetParams* p) {
  if (!p) return "null FleetQTargetParams";
  if (p->struct_bytes != (int32_t)sizeof(FleetQTargetParams)) return "FleetQTargetParams.struct_bytes does not match this library";
  if (p->obs_dim < 1 || p->obs_dim > FLEET_POLICY_MAX_OBS_DIM)
    return "obs_dim must be in 1.." + std::to_string(FLEET_POLICY_MAX_OBS_DIM) + ", got " + std::to_string(p->obs_dim);
  if (p->n_critics < 1 || p->n_critics > 2) return "n_critics must be 1 or 2, got " + std::to_string(p->n_critics);
  std::string why = policy_validate_head(p->actor, "actor: ");
  if (!why.empty()) return why;
  const int A = p->actor.width[p->actor.n_layers - 1];
  if (p->obs_dim + A > FLEET_POLICY_MAX_OBS_DIM)
    return "obs_dim + act_dim must be at most " + std::to_string(FLEET_POLICY_MAX_OBS_DIM) + " (a critic's input), got " +
           std::to_string(p->obs_dim) + " + " + std::to_string(A);
  for (int c = 0; c < p->n_critics; ++c) {
    const std::string who = "critic " + std::to_string(c) + ": ";
    why = policy_validate_head(p->critic[c], who);
    if (!why.empty()) return why;
    if (p->critic[c].width[p->critic[c].n_layers - 1] != 1)
      return who + "the last width must be 1, got " + std::to_string(p->critic[c].width[p->critic[c].n_layers - 1]);
    if (p->critic[c].output != FLEET_POLICY_OUT_NONE) return who + "the output transform must be NONE";
  }
  return "";
}

const FleetPolicyHead& head_of(const FleetQTargetParams& p, int net) { return net ? p.critic[net - 1] : p.actor; }

// the record of the networks and the size of the block (floats)
size_t describe_layout(const FleetQTargetParams& p, QTargetDesc* d) {
  *d = QTargetDesc{};
  const int A = p.actor.width[p.actor.n_layers - 1];
  d->obs_dim = p.obs_dim, d->act_dim = A, d->n_critics = p.n_critics, d->stride = 64, d->act64 = policy_round_up(A, 64);
  size_t off = policy_round_up((int)sizeof(QTargetDesc), 256) / 4;
  for (int net = 0; net < 1 + p.n_critics; ++net) {
    const FleetPolicyHead& H = head_of(p, net);
    PolicyHeadDesc& o = d->net[net];
    o.n_layers = H.n_layers, o.activation = H.activation, o.output = H.output, o.lo = H.lo, o.hi = H.hi;
    for (int l = 0; l < H.n_layers; ++l) {
      PolicyLayer& L = o.layer[l];
      L.in = l ? H.width[l - 1] : (net ? p.obs_dim + A : p.obs_dim), L.out = H.width[l];
      L.in4 = policy_round_up(L.in, 4), L.out64 = policy_round_up(L.out, 64);
      L.w_off = (uint32_t)off;
      off += (size_t)L.in4 * L.out64;
      L.b_off = (uint32_t)off;
      off += (size_t)L.out64;
      if (l < H.n_layers - 1 && L.out64 > d->stride) d->stride = L.out64;
    }
  }
  return off;  // <= 256 + 3 * 4 * (8192 * 512 + 512) floats: fits the 32-bit offsets
}

}  // namespace

struct FleetQTarget : FleetHandleBase {
  FleetQTargetParams p{};
  QTargetDesc desc{};
  size_t floats = 0;     // of the block
  size_t lds_bytes = 0;  // of one workgroup of qtarget_target
  int n_tensors = 0;
};

namespace {

const char* const kNetName[kQNets] = {"actor", "critic 0", "critic 1"};

// the packed weights -> the block's image (the record included); "" or why not
std::string build_image(const FleetQTarget* h, const float* weights, std::vector<float>* image) {
  image->assign(h->floats, 0.0f);
  memcpy(image->data(), &h->desc, sizeof(QTargetDesc));
  const float* src = weights;
  for (int net = 0; net < 1 + h->desc.n_critics; ++net)
    for (int l = 0; l < h->desc.net[net].n_layers; ++l) {
      const PolicyLayer& L = h->desc.net[net].layer[l];
      const size_t count = (size_t)L.in * L.out + L.out;
      for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(src[i]))
          return std::string(kNetName[net]) + ", layer " + std::to_string(l) + ": " + (i < count - L.out ? "weight " : "bias ") +
                 std::to_string(i < count - L.out ? i : i - (count - L.out)) + " is not finite";
      for (int j = 0; j < L.out; ++j)
        for (int k = 0; k < L.in; ++k) (*image)[L.w_off + (size_t)k * L.out64 + j] = src[(size_t)j * L.in + k];
      src += (size_t)L.in * L.out;
      for (int j = 0; j < L.out; ++j) (*image)[L.b_off + j] = src[j];
      src += L.out;
    }
  return "";
}

int upload(FleetQTarget* h, const std::vector<float>& image) {
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  FLEET_HANDLE_TRY(h, hipMemcpyAsync(h->block, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  FLEET_HANDLE_TRY(h, hipStreamSynchronize(h->stream));  // (the image is the caller's stack from here on)
  return FLEET_OK;
}

// load_dev, polyak_dev, export_dev: one launch over the tensors
template <int kMode>
int relay(FleetQTarget* h, const char* entry, float* const* tensors, int count, float tau, float omt) {
  if (!tensors || count != h->n_tensors) {
    h->error = std::string(entry) + ": expected " + std::to_string(h->n_tensors) + " tensors (W, b per layer), got " +
               (tensors ? std::to_string(count) : std::string("a null array"));
    return FLEET_ERR_INVALID;
  }
  QRelayArgs a{};
  for (int i = 0; i < count; ++i) {
    if (!tensors[i]) {
      h->error = std::string(entry) + ": tensor " + std::to_string(i) + " is null";
      return FLEET_ERR_INVALID;
    }
    a.tensor[i] = tensors[i];
  }
  a.desc = reinterpret_cast<const QTargetDesc*>(h->block);
  a.base = reinterpret_cast<float*>(h->block);
  a.tau = tau, a.omt = omt;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(qtarget_relay<kMode>, dim3(64, count), dim3(256), 0, h->stream, a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

// what fleet_qtarget_target_dev refuses, looked at without the handle; "" when the arguments pass
std::string check_target_args(const float* next_obs, const float* rewards, const float* dones, int B, const FleetQTargetArgs* args) {
  if (!args) return "null FleetQTargetArgs";
  const FleetQTargetArgs& x = *args;
  if (x.struct_bytes != (int32_t)sizeof(FleetQTargetArgs)) return "FleetQTargetArgs.struct_bytes does not match this library";
  if (x.noise_mode != FLEET_EXPLORE_NOISE_DRAW && x.noise_mode != FLEET_EXPLORE_NOISE_GIVEN)
    return "unknown noise_mode " + std::to_string(x.noise_mode);
  if (B < 1) return "B must be >= 1, got " + std::to_string(B);
  if (!next_obs) return "null next_obs";
  if (!rewards) return "null rewards";
  if (!dones) return "null dones";
  if (!x.sigma) return "null sigma";
  if (!x.target_q) return "null target_q";
  if (!(x.act_lo <= x.act_hi)) return "the bounds need act_lo <= act_hi";
  if (!(x.noise_clip >= 0.0f)) return "noise_clip must be >= 0";
  if (x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN && !x.noise) return "noise_mode GIVEN with a null noise";
  if (x.row_offset < 0) return "row_offset must be >= 0, got " + std::to_string(x.row_offset);
  return "";
}

}  // namespace

extern "C" {

int fleet_qtarget_create(int device, const FleetQTargetParams* p, const float* host_weights, fleet_qtarget_handle* out) {
  if (out) *out = nullptr;
  std::string why = validate(p);  // before the device is touched
  if (why.empty() && !host_weights) why = "null host_weights";
  if (why.empty() && !out) why = "null output handle";
  if (!why.empty()) {
    g_qtarget_error = "fleet_qtarget_create: " + why;
    return FLEET_ERR_INVALID;
  }
  FleetQTarget* h = new FleetQTarget();
  h->p = *p;
  h->p.tile_rows = kPolicyRows;
  h->floats = describe_layout(*p, &h->desc);
  h->lds_bytes = ((size_t)2 * kPolicyRows * h->desc.stride + (size_t)kPolicyRows * kPolicyChunk + (size_t)kPolicyRows * h->desc.act64) * sizeof(float);
  for (int net = 0; net < 1 + p->n_critics; ++net) h->n_tensors += 2 * head_of(*p, net).n_layers;
  std::vector<float> image;
  why = build_image(h, host_weights, &image);
  if (!why.empty()) {
    g_qtarget_error = "fleet_qtarget_create: " + why;
    delete h;
    return FLEET_ERR_INVALID;
  }
  int rc = handle_open(h, device, h->floats * sizeof(float), "target networks", &g_qtarget_error);
  if (rc == FLEET_OK) {
    // more than the 64 KiB a launch gets unasked; the attribute belongs to the kernel: every handle asks for the widest one's need
    constexpr int kMaxLds = (3 * kPolicyRows * FLEET_POLICY_MAX_WIDTH + kPolicyRows * kPolicyChunk) * (int)sizeof(float);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&qtarget_target), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds) != hipSuccess) {
      (void)hipGetLastError();
      g_qtarget_error = "hipFuncSetAttribute failed for the target kernel's " + std::to_string(kMaxLds) + " bytes of LDS";
      rc = FLEET_ERR_HIP;
    }
  }
  if (rc == FLEET_OK && (rc = upload(h, image)) != FLEET_OK) g_qtarget_error = h->error;
  if (rc != FLEET_OK) {
    fleet_qtarget_destroy(h);
    return rc;
  }
  *out = h;
  return FLEET_OK;
}

int fleet_qtarget_destroy(fleet_qtarget_handle h) {
  if (!h) return FLEET_OK;
  handle_close(h);
  delete h;
  return FLEET_OK;
}

const char* fleet_qtarget_last_error(fleet_qtarget_handle h) { return h ? h->error.c_str() : g_qtarget_error.c_str(); }

int fleet_qtarget_set_stream(fleet_qtarget_handle h, void* hip_stream) { return h ? handle_set_stream(h, hip_stream) : FLEET_ERR_INVALID; }

int fleet_qtarget_load_host(fleet_qtarget_handle h, const float* weights) {
  if (!h) return FLEET_ERR_INVALID;
  if (!weights) {
    h->error = "fleet_qtarget_load_host: null weights";
    return FLEET_ERR_INVALID;
  }
  std::vector<float> image;
  const std::string why = build_image(h, weights, &image);
  if (!why.empty()) {
    h->error = "fleet_qtarget_load_host: " + why;
    return FLEET_ERR_INVALID;
  }
  return upload(h, image);
}

int fleet_qtarget_load_dev(fleet_qtarget_handle h, const float* const* tensors, int count) {
  if (!h) return FLEET_ERR_INVALID;
  return relay<kRelayLoad>(h, "fleet_qtarget_load_dev", const_cast<float* const*>(tensors), count, 0.0f, 0.0f);  // (read only)
}

int fleet_qtarget_polyak_dev(fleet_qtarget_handle h, const float* const* tensors, int count, double tau) {
  if (!h) return FLEET_ERR_INVALID;
  if (!(tau >= 0.0 && tau <= 1.0)) {
    h->error = "fleet_qtarget_polyak_dev: tau must be in [0, 1], got " + std::to_string(tau);
    return FLEET_ERR_INVALID;
  }
  return relay<kRelayPolyak>(h, "fleet_qtarget_polyak_dev", const_cast<float* const*>(tensors), count, (float)tau, (float)(1.0 - tau));
}

int fleet_qtarget_export_dev(fleet_qtarget_handle h, float* const* tensors, int count) {
  if (!h) return FLEET_ERR_INVALID;
  return relay<kRelayExport>(h, "fleet_qtarget_export_dev", tensors, count, 0.0f, 0.0f);
}

int fleet_qtarget_target_dev(fleet_qtarget_handle h, const float* next_obs, const float* rewards, const float* dones, int B,
                             const FleetQTargetArgs* args) {
  const std::string why = check_target_args(next_obs, rewards, dones, B, args);
  if (!h) {
    g_qtarget_error = "fleet_qtarget_target_dev: " + (why.empty() ? std::string("null handle") : why);
    return FLEET_ERR_INVALID;
  }
  if (!why.empty()) {
    h->error = "fleet_qtarget_target_dev: " + why;
    return FLEET_ERR_INVALID;
  }
  const FleetQTargetArgs& x = *args;
  TargetArgs t{};
  t.desc = reinterpret_cast<const QTargetDesc*>(h->block);
  t.base = reinterpret_cast<const float*>(h->block);
  t.next_obs = next_obs, t.rewards = rewards, t.dones = dones, t.sigma = x.sigma;
  t.noise = x.noise, t.target_q = x.target_q, t.next_actions = x.next_actions, t.q = x.q;
  t.seed = x.seed, t.step = x.step, t.row_id0 = (uint32_t)x.row_offset;
  t.given = x.noise_mode == FLEET_EXPLORE_NOISE_GIVEN, t.B = B;
  t.gamma = x.gamma, t.noise_clip = x.noise_clip, t.lo = x.act_lo, t.hi = x.act_hi;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  const dim3 grid((unsigned)(((size_t)B + kPolicyRows - 1) / kPolicyRows)), block(kPolicyThreads);
  hipLaunchKernelGGL(qtarget_target, grid, block, h->lds_bytes, h->stream, t);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}

int fleet_qtarget_describe(fleet_qtarget_handle h, FleetQTargetParams* out) {
  if (!h || !out) return FLEET_ERR_INVALID;
  *out = h->p;
  return FLEET_OK;
}

}  // extern "C"
