// fleet_mlp.h -- the weight image of a span of MLPs, which the policy (fleet_policy.hip) and the TD3 / DDPG target networks
// (fleet_qtarget.hip) keep in the same form: one device block that opens with the family's record, then per layer the weights as
// Wt[in4][out64] and the bias as b[out64], zero-padded (PolicyLayer, fleet_policy.h).  Everything about that image but the forward
// itself is here (fleet_mlp.hip): its layout, building it from packed host weights, the upload, the one kernel that walks its real
// elements (load, polyak, export) and the device half of *_create.  The families keep their records, their validation of their own
// parameter structs and their forward kernels; the shared code sees a record as its bytes and the span of nets in it.
// The handles that work ON such an image without owning one (fleet_ppo.hip, fleet_td3.hip, fleet_adam.hip) borrow it here too:
// FleetMlpUser, mlp_borrow, mlp_user_open, mlp_user_close.
#pragma once
#include <initializer_list>
#include <string>
#include <type_traits>

#include "fleet_handle.h"
#include "fleet_policy.h"

constexpr int kMlpMaxNets = 3;  // the larger family: actor, critic 0, critic 1
constexpr int kMlpMaxTensors = 2 * kMlpMaxNets * FLEET_POLICY_MAX_LAYERS;
static_assert(FLEET_POLICY_MAX_HEADS <= kMlpMaxNets, "the re-lay kernel's tensor array holds the larger family's");

// what a family is called in messages
struct MlpNames {
  const char* const* net;  // per net: "head 0", "critic 1"
  const char* block;       // "hipMalloc of the <block>'s ... bytes failed"
  const char* kernel;      // "hipFuncSetAttribute failed for the <kernel> kernel's ... bytes of LDS"
  const char* refusal;     // opens *_create's refusal of a weight that is not finite ("" or "fleet_qtarget_create: ")
};

// what both families' handles carry about the image; `record` is the family's record on the host, the first bytes of the block
struct FleetMlpHandle : FleetHandleBase {
  size_t floats = 0;  // of the block
  int n_tensors = 0;  // W, b per layer, net after net
  const void* record = nullptr;
  size_t record_bytes = 0;
  PolicyHeadDesc* nets = nullptr;  // the span of nets in *record
  int n_nets = 0;
  const MlpNames* names = nullptr;
};

// What mlp_borrow relies on, asserted by each family behind its handle's definition: the image's handle is the first base of T.
template <typename T>
constexpr bool mlp_image_is_first_base = std::is_base_of<FleetMlpHandle, T>::value && !std::is_polymorphic<T>::value;

// A handle that borrows an image: it launches on the image's device and stream, and the image's owner must outlive it.  It owns
// one device allocation (a scratch, an optimiser's state).
struct FleetMlpUser {
  FleetMlpHandle* img = nullptr;  // borrowed
  std::string error;              // *_last_error(handle)
  char* block = nullptr;          // owned

  float* floats() const { return reinterpret_cast<float*>(block); }
};

// The image behind an opaque fleet_policy_handle or fleet_qtarget_handle, when it is the family's whose record has `record_bytes`
// bytes; otherwise NULL, with "null <noun> handle" or "the handle is not a <noun> handle" in *why.
FleetMlpHandle* mlp_borrow(void* owner, size_t record_bytes, const char* noun, std::string* why);

// The normaliser's frozen statistics (when one is given) for a forward of h's `noun` ("policy") over obs_dim columns, its read opened
// on h's stream (the caller ends it behind the launch: fleet_norm_end_read); *norm_obs: whether it normalises observations at all.
// A normaliser of another shape or device is refused in h->error, `entry` in front.  Shared by fleet_policy.hip and fleet_sac.hip.
struct MlpNormStats {
  const double *mean, *sd;
  double clip;
};
int mlp_bind_norm(FleetHandleBase* h, int obs_dim, const char* noun, const char* entry, fleet_norm_handle norm, MlpNormStats* out, bool* norm_obs);

inline int mlp_round_up(int v, int m) { return (v + m - 1) / m * m; }

// what *_create refuses about one head, before the device is touched; `who` opens the message ("head 0: "); "" when it passes
std::string mlp_validate_head(const FleetPolicyHead& H, const std::string& who);

// heads[n] with a first layer over first_in[n] columns -> nets[n], laid out behind a record of record_bytes bytes; *stride: the widest
// hidden layer's out64 over the span (64 without one).  Returns the size of the block in floats.
size_t mlp_describe_layout(const FleetPolicyHead* const* heads, const int* first_in, int n_nets, size_t record_bytes, PolicyHeadDesc* nets,
                           int32_t* stride);

// The device half of *_create, after the family validated its parameters and filled h (floats, record, nets, names): the image of
// the packed `weights`, handle_open, the kernels' dynamic LDS limits, the upload.  A status other than FLEET_OK comes with the reason
// in *why, and the handle is then the caller's to destroy.
struct MlpKernelLds {
  const void* kernel;
  int bytes;  // hipFuncAttributeMaxDynamicSharedMemorySize
};
int mlp_open(FleetMlpHandle* h, int device, const float* weights, std::initializer_list<MlpKernelLds> kernels, std::string* why);

// The device half of a borrower's *_create, after it validated its parameters: the image's device, the kernels' dynamic LDS limits
// ("the <kernel> kernel's" in the message), `bytes` bytes of device memory (not initialised; "the <noun>'s").  A status other than
// FLEET_OK comes with the reason in *why, and the handle is then the caller's to destroy.
int mlp_user_open(FleetMlpUser* u, FleetMlpHandle* img, size_t bytes, const char* noun, std::initializer_list<MlpKernelLds> kernels,
                  const char* kernel, std::string* why);

// frees the block, which waits for the device: whatever still reads it is done.  The image is not touched.
void mlp_user_close(FleetMlpUser* u);

// *_load_host: new packed weights of the same shapes
int mlp_load_host(FleetMlpHandle* h, const char* entry, const float* weights);

// *_load_dev, *_polyak_dev, *_export_dev: one launch over `count` tensors in torch's layout (read; written by kMlpExport)
constexpr int kMlpLoad = 0, kMlpPolyak = 1, kMlpExport = 2;
int mlp_launch_relay(FleetMlpHandle* h, int mode, const char* entry, float* const* tensors, int count, float tau, float omt);
// ... the same launch over a COPY of the image at `base` (h's layout, h's stream): the evaluation's snapshot (fleet_eval.hip)
int mlp_launch_relay_at(FleetMlpHandle* h, float* base, int mode, const char* entry, float* const* tensors, int count, float tau, float omt);
