// fleet_mlp.hip -- the weight image the policy and the target networks share (fleet_mlp.h): layout, host image, upload, and
//   mlp_relay  grid (64, tensors): load (torch's [out, in] -> the image), polyak (the same walk, t' = fmaf(tau, p, t * omt)) and
//              export (the image -> torch's layout).  Only real elements are visited: the padding stays what create made it.
// Launch boundaries are the only visibility mechanism; no atomics.  float32 throughout.
#include "fleet_mlp.h"

#include <hip/hip_runtime.h>

#include "fleet_norm.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

struct RelayArgs {
  float* tensor[kMlpMaxTensors];  // (read in the load and polyak modes, written in the export mode)
  const PolicyHeadDesc* nets;     // the span in the block
  int n_nets;
  float* base;
  float tau, omt;
};

// tensor blockIdx.y (W, b per layer, net after net): W[out][in] <-> Wt[in][out64], b <-> b
template <int kMode>
__global__ __launch_bounds__(256) void mlp_relay(RelayArgs a) {
  const PolicyHeadDesc* __restrict__ nets = a.nets;
  int t = blockIdx.y, net = 0;
  while (net < a.n_nets - 1 && t >= 2 * nets[net].n_layers) t -= 2 * nets[net++].n_layers;
  const PolicyLayer L = nets[net].layer[t >> 1];
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
    if (kMode == kMlpLoad) a.base[img] = ext[e];
    else if (kMode == kMlpExport) ext[e] = a.base[img];
    else a.base[img] = fmaf(a.tau, ext[e], a.base[img] * a.omt);
  }
}

// the packed weights -> the block's image (the record included); "" or why not
std::string build_image(const FleetMlpHandle* h, const float* weights, std::vector<float>* image) {
  image->assign(h->floats, 0.0f);
  memcpy(image->data(), h->record, h->record_bytes);
  const float* src = weights;
  for (int net = 0; net < h->n_nets; ++net)
    for (int l = 0; l < h->nets[net].n_layers; ++l) {
      const PolicyLayer& L = h->nets[net].layer[l];
      const size_t count = (size_t)L.in * L.out + L.out;
      for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(src[i]))
          return std::string(h->names->net[net]) + ", layer " + std::to_string(l) + ": " + (i < count - L.out ? "weight " : "bias ") +
                 std::to_string(i < count - L.out ? i : i - (count - L.out)) + " is not finite";
      for (int j = 0; j < L.out; ++j)
        for (int k = 0; k < L.in; ++k) (*image)[L.w_off + (size_t)k * L.out64 + j] = src[(size_t)j * L.in + k];
      src += (size_t)L.in * L.out;
      for (int j = 0; j < L.out; ++j) (*image)[L.b_off + j] = src[j];
      src += L.out;
    }
  return "";
}

int upload(FleetMlpHandle* h, const std::vector<float>& image) {
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  FLEET_HANDLE_TRY(h, hipMemcpyAsync(h->block, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
  FLEET_HANDLE_TRY(h, hipStreamSynchronize(h->stream));  // (the image is the caller's stack from here on)
  return FLEET_OK;
}

// more than the 64 KiB a launch gets unasked when the layers are wide; the attribute belongs to the kernel, not to the handle, so
// every handle asks for what the widest network needs
int set_lds_limits(std::initializer_list<MlpKernelLds> kernels, const char* noun, std::string* why) {
  int most = 0;
  bool set = true;
  for (const MlpKernelLds& k : kernels) {
    set = set && hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes) == hipSuccess;
    most = k.bytes > most ? k.bytes : most;
  }
  if (set) return FLEET_OK;
  (void)hipGetLastError();
  *why = std::string("hipFuncSetAttribute failed for the ") + noun + " kernel's " + std::to_string(most) + " bytes of LDS";
  return FLEET_ERR_HIP;
}

}  // namespace

// FleetPolicy (fleet_policy.hip) and FleetQTarget (fleet_qtarget.h) derive from FleetMlpHandle and from nothing else, and neither
// is polymorphic (mlp_image_is_first_base, asserted where each is defined): the image's handle is the first base, at the address
// the opaque handle holds.  The families are told apart by the size of their records.
FleetMlpHandle* mlp_borrow(void* owner, size_t record_bytes, const char* noun, std::string* why) {
  if (!owner) {
    *why = std::string("null ") + noun + " handle";
    return nullptr;
  }
  FleetMlpHandle* img = reinterpret_cast<FleetMlpHandle*>(owner);
  if (img->record_bytes == record_bytes) return img;
  *why = std::string("the handle is not a ") + noun + " handle";
  return nullptr;
}

int mlp_bind_norm(FleetHandleBase* h, int obs_dim, const char* noun, const char* entry, fleet_norm_handle norm, MlpNormStats* out, bool* norm_obs) {
  *norm_obs = false;
  if (!norm) return FLEET_OK;
  FleetNormView v{};
  FLEET_HANDLE_TRY(h, fleet_norm_begin_read(norm, h->stream, &v));
  if (v.D != obs_dim || v.device != h->device) {
    h->error = std::string(entry) + ": the normaliser has obs_dim " + std::to_string(v.D) + " on device " + std::to_string(v.device) +
               ", the " + noun + " " + std::to_string(obs_dim) + " on device " + std::to_string(h->device);
    return FLEET_ERR_INVALID;
  }
  out->mean = v.obs_mean, out->sd = v.obs_sd, out->clip = v.clip_obs;
  *norm_obs = v.norm_obs != 0;
  return FLEET_OK;
}

std::string mlp_validate_head(const FleetPolicyHead& H, const std::string& who) {
  if (H.n_layers < 1 || H.n_layers > FLEET_POLICY_MAX_LAYERS)
    return who + "n_layers must be in 1.." + std::to_string(FLEET_POLICY_MAX_LAYERS) + ", got " + std::to_string(H.n_layers);
  for (int l = 0; l < H.n_layers; ++l)
    if (H.width[l] < 1 || H.width[l] > FLEET_POLICY_MAX_WIDTH)
      return who + "width of layer " + std::to_string(l) + " must be in 1.." + std::to_string(FLEET_POLICY_MAX_WIDTH) + ", got " +
             std::to_string(H.width[l]);
  if (H.activation != FLEET_POLICY_ACT_TANH && H.activation != FLEET_POLICY_ACT_RELU) return who + "unknown activation";
  if (H.output != FLEET_POLICY_OUT_NONE && H.output != FLEET_POLICY_OUT_CLIP && H.output != FLEET_POLICY_OUT_TANH)
    return who + "unknown output transform";
  if (H.output == FLEET_POLICY_OUT_CLIP && !(H.lo <= H.hi)) return who + "clip bounds need lo <= hi";
  return "";
}

size_t mlp_describe_layout(const FleetPolicyHead* const* heads, const int* first_in, int n_nets, size_t record_bytes, PolicyHeadDesc* nets,
                           int32_t* stride) {
  *stride = 64;
  size_t off = mlp_round_up((int)record_bytes, 256) / 4;
  for (int net = 0; net < n_nets; ++net) {
    const FleetPolicyHead& H = *heads[net];
    PolicyHeadDesc& o = nets[net];
    o.n_layers = H.n_layers, o.activation = H.activation, o.output = H.output, o.lo = H.lo, o.hi = H.hi;
    for (int l = 0; l < H.n_layers; ++l) {
      PolicyLayer& L = o.layer[l];
      L.in = l ? H.width[l - 1] : first_in[net], L.out = H.width[l];
      L.in4 = mlp_round_up(L.in, 4), L.out64 = mlp_round_up(L.out, 64);
      L.w_off = (uint32_t)off;
      off += (size_t)L.in4 * L.out64;
      L.b_off = (uint32_t)off;
      off += (size_t)L.out64;
      if (l < H.n_layers - 1 && L.out64 > *stride) *stride = L.out64;
    }
  }
  // the offsets fit 32 bits: in floats, a record of at most 1 KiB, and per net at most FLEET_POLICY_MAX_LAYERS layers of at most
  // FLEET_POLICY_MAX_OBS_DIM x FLEET_POLICY_MAX_WIDTH weights and FLEET_POLICY_MAX_WIDTH biases
  constexpr uint64_t kLayerFloats = (uint64_t)FLEET_POLICY_MAX_OBS_DIM * FLEET_POLICY_MAX_WIDTH + FLEET_POLICY_MAX_WIDTH;
  static_assert(256 + kMlpMaxNets * FLEET_POLICY_MAX_LAYERS * kLayerFloats < (1ull << 32), "PolicyLayer's offsets are 32 bits");
  return off;
}

int mlp_open(FleetMlpHandle* h, int device, const float* weights, std::initializer_list<MlpKernelLds> kernels, std::string* why) {
  h->n_tensors = 0;
  for (int net = 0; net < h->n_nets; ++net) h->n_tensors += 2 * h->nets[net].n_layers;
  std::vector<float> image;
  const std::string bad = build_image(h, weights, &image);
  if (!bad.empty()) {
    *why = h->names->refusal + bad;
    return FLEET_ERR_INVALID;
  }
  int rc = handle_open(h, device, h->floats * sizeof(float), h->names->block, why);
  if (rc != FLEET_OK) return rc;
  if ((rc = set_lds_limits(kernels, h->names->kernel, why)) != FLEET_OK) return rc;
  if ((rc = upload(h, image)) != FLEET_OK) *why = h->error;
  return rc;
}

int mlp_user_open(FleetMlpUser* u, FleetMlpHandle* img, size_t bytes, const char* noun, std::initializer_list<MlpKernelLds> kernels,
                  const char* kernel, std::string* why) {
  u->img = img;
  if (hipSetDevice(img->device) != hipSuccess) {
    *why = "hipSetDevice failed";
    return FLEET_ERR_HIP;
  }
  if (const int rc = set_lds_limits(kernels, kernel, why); rc != FLEET_OK) return rc;
  void* q = nullptr;
  if (hipMalloc(&q, bytes) != hipSuccess) {
    (void)hipGetLastError();  // (the failure is reported here: it must not surface again from the caller's next HIP call)
    *why = std::string("hipMalloc of the ") + noun + "'s " + std::to_string(bytes) + " bytes failed";
    return FLEET_ERR_HIP;
  }
  u->block = static_cast<char*>(q);
  return FLEET_OK;
}

void mlp_user_close(FleetMlpUser* u) {
  if (u->block) (void)hipFree(u->block);
  u->block = nullptr;
}

int mlp_load_host(FleetMlpHandle* h, const char* entry, const float* weights) {
  if (!weights) {
    h->error = std::string(entry) + ": null weights";
    return FLEET_ERR_INVALID;
  }
  std::vector<float> image;
  const std::string why = build_image(h, weights, &image);
  if (!why.empty()) {
    h->error = std::string(entry) + ": " + why;
    return FLEET_ERR_INVALID;
  }
  return upload(h, image);
}

int mlp_launch_relay(FleetMlpHandle* h, int mode, const char* entry, float* const* tensors, int count, float tau, float omt) {
  return mlp_launch_relay_at(h, reinterpret_cast<float*>(h->block), mode, entry, tensors, count, tau, omt);
}

int mlp_launch_relay_at(FleetMlpHandle* h, float* base, int mode, const char* entry, float* const* tensors, int count, float tau, float omt) {
  if (!tensors || count != h->n_tensors) {
    h->error = std::string(entry) + ": expected " + std::to_string(h->n_tensors) + " tensors (W, b per layer), got " +
               (tensors ? std::to_string(count) : std::string("a null array"));
    return FLEET_ERR_INVALID;
  }
  RelayArgs a{};
  for (int i = 0; i < count; ++i) {
    if (!tensors[i]) {
      h->error = std::string(entry) + ": tensor " + std::to_string(i) + " is null";
      return FLEET_ERR_INVALID;
    }
    a.tensor[i] = tensors[i];
  }
  a.nets = reinterpret_cast<const PolicyHeadDesc*>(h->block + (reinterpret_cast<const char*>(h->nets) - static_cast<const char*>(h->record)));
  a.n_nets = h->n_nets;
  a.base = base;
  a.tau = tau, a.omt = omt;
  FLEET_HANDLE_TRY(h, hipSetDevice(h->device));
  const dim3 grid(64, count), block(256);
  if (mode == kMlpLoad) hipLaunchKernelGGL(mlp_relay<kMlpLoad>, grid, block, 0, h->stream, a);
  else if (mode == kMlpPolyak) hipLaunchKernelGGL(mlp_relay<kMlpPolyak>, grid, block, 0, h->stream, a);
  else hipLaunchKernelGGL(mlp_relay<kMlpExport>, grid, block, 0, h->stream, a);
  FLEET_HANDLE_TRY(h, hipGetLastError());
  return FLEET_OK;
}
