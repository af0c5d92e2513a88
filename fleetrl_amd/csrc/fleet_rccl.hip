// fleet_rccl.hip -- the RCCL binding and its four entries: the unique id, a communicator's create and destroy, and the all-gather
// of the handle's last-episode statistics on the handle's stream.
#include <dlfcn.h>

#include <cstring>
#include <functional>
#include <mutex>

#include "fleet_batch.h"

namespace {

// RCCL, bound at run time: a process that never gathers across GPUs does not need librccl, and a process that has PyTorch in
// it gets the copy PyTorch has already mapped (same soname) instead of a second one.  The handful of NCCL-API declarations the
// binding needs are restated here (their ABI is fixed: rccl/rccl.h `ncclUniqueId` = 128 opaque bytes, `ncclSuccess` = 0,
// `ncclDouble` = 8), so that building this library does not need RCCL's headers either.
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[FLEET_RCCL_UNIQUE_ID_BYTES]; } ncclUniqueId;
typedef int ncclResult_t;
typedef int ncclDataType_t;
constexpr ncclResult_t ncclSuccess = 0;
constexpr ncclDataType_t ncclDouble = 8;
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string why;
};
void rccl_bind(RcclApi& api);
RcclApi& rccl() {  // bound once, whichever thread asks first
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, rccl_bind, std::ref(api));
  return api;
}
void rccl_bind(RcclApi& api) {
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) {
    api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (api.lib) break;
  }
  if (!api.lib) {
    const char* e = dlerror();
    api.why = std::string("librccl not found: ") + (e ? e : "");
    return;
  }
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.lib, "ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.lib, "ncclCommInitRank"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.lib, "ncclCommDestroy"));
  api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(api.lib, "ncclAllGather"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.lib, "ncclGetErrorString"));
  if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather) api.why = "librccl lacks an expected symbol";
}

}  // namespace

extern "C" {

int fleet_rccl_unique_id(void* id128) {
  if (!id128) return FLEET_ERR_INVALID;
  RcclApi& r = rccl();
  if (!r.why.empty()) { fleet_set_create_error(r.why); return FLEET_ERR_HIP; }
  static_assert(sizeof(ncclUniqueId) == FLEET_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  if (r.GetUniqueId(&id) != ncclSuccess) { fleet_set_create_error("ncclGetUniqueId failed"); return FLEET_ERR_HIP; }
  memcpy(id128, &id, sizeof id);
  return FLEET_OK;
}

int fleet_rccl_comm_create(int device, int world_size, int rank, const void* id128, void** comm) {
  if (!id128 || !comm || world_size < 1 || rank < 0 || rank >= world_size) return FLEET_ERR_INVALID;
  RcclApi& r = rccl();
  if (!r.why.empty()) { fleet_set_create_error(r.why); return FLEET_ERR_HIP; }
  if (hipSetDevice(device) != hipSuccess) { fleet_set_create_error("hipSetDevice failed"); return FLEET_ERR_HIP; }
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  ncclComm_t c = nullptr;
  const ncclResult_t rc = r.CommInitRank(&c, world_size, id, rank);
  if (rc != ncclSuccess) {
    fleet_set_create_error(std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(rc) : "failed"));
    return FLEET_ERR_HIP;
  }
  *comm = c;
  return FLEET_OK;
}

int fleet_rccl_comm_destroy(void* comm) {
  if (!comm) return FLEET_OK;
  RcclApi& r = rccl();
  if (!r.why.empty()) return FLEET_ERR_HIP;
  return r.CommDestroy(static_cast<ncclComm_t>(comm)) == ncclSuccess ? FLEET_OK : FLEET_ERR_HIP;
}

int fleet_gather_episode_stats_rccl(fleet_handle h, void* comm, int world_size, double* out_dev) {
  FLEET_ENTER(h);
  if (!h || !comm || world_size < 1 || !out_dev) {
    if (h) h->error = "fleet_gather_episode_stats_rccl: bad argument";
    return FLEET_ERR_INVALID;
  }
  RcclApi& r = rccl();
  if (!r.why.empty()) { h->error = r.why; return FLEET_ERR_HIP; }
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t E = (size_t)h->d.E;
  // [2, E] float64 in the handle's staging block: returns, then lengths (exact in float64)
  double* send = static_cast<double*>(h->st_field);
  HIP_TRY(h, fleet_launch_gather_field(h->d, FLEET_F_LAST_EP_RETURN, send, h->stream));
  HIP_TRY(h, fleet_launch_gather_field(h->d, FLEET_F_LAST_EP_LEN_F64, send + E, h->stream));
  const ncclResult_t rc = r.AllGather(send, out_dev, 2 * E, ncclDouble, static_cast<ncclComm_t>(comm), h->stream);
  if (rc != ncclSuccess) {
    h->error = std::string("ncclAllGather: ") + (r.GetErrorString ? r.GetErrorString(rc) : "failed");
    return FLEET_ERR_HIP;
  }
  return FLEET_OK;
}

}  // extern "C"
