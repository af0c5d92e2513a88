// fleet_state.h -- env state in the caller's hands (fleet_state.hip): the blob layout, the fingerprint that decides whether a state
// fits a handle, whole-handle save / load as one copy per section, and the fork kernel that copies chosen envs within a handle or
// between two.  Called by the fleet_state_* / fleet_fork_envs entry points (fleet_capi.hip; the handle: fleet_batch.h).  What "the state" is:
// fleet_device.h, beside FleetDev.  DESIGN.md "Env state in the caller's hands".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "fleet_device.h"

// What the state code needs of a handle.
struct FleetStateRefs {
  const FleetParams* p;
  const FleetDev* d;
  FleetCold* cold_host;       // host mirror of *d->cold: the per-handle items live here
  FleetCold* cold_dev;
  int32_t** dev_sched;        // the handle's start-schedule allocation (hipMalloc / hipFree, or nullptr)
  uint64_t table_hash;
  hipStream_t stream;
  FleetStateHeader* pin_hdr;  // pinned staging for one header (rewritten only after the stream has drained)
  std::string* error;
};

uint64_t fleet_state_hash_tables(const FleetParams& p, const FleetTables& t);
void fleet_state_fingerprint(const FleetParams& p, const FleetDev& d, uint64_t table_hash, FleetStateFingerprint* fp);
// nullptr when equal, else the name of the first field that differs
const char* fleet_state_fingerprint_diff(const FleetStateFingerprint& a, const FleetStateFingerprint& b);
uint64_t fleet_state_blob_bytes(const FleetStateRefs& r);
// host = the blob is host memory (the call returns when the copies have landed); else device memory, asynchronous on r.stream
int fleet_state_save(const FleetStateRefs& r, void* blob, uint64_t bytes, bool host);
// validates the header first; restores the sections and the per-handle items; synchronises r.stream
int fleet_state_load(const FleetStateRefs& r, const void* blob, uint64_t bytes, bool host);
// What a fork keeps on its destination handle between calls: the device copy of the index pairs and its pinned staging (both grown
// to `cap` pairs, never shrunk) and the event that orders the kernel against the source's stream.
struct FleetForkScratch {
  int2* idx_dev = nullptr;
  int2* idx_pin = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
};
void fleet_state_fork_release(FleetForkScratch* k);
// argument checks (FLEET_ERR_INVALID, nothing launched), then the index upload out of the pinned staging and the kernel on dst.stream,
// nothing waited for; between two records of the event when src launches on another stream.  The caller has drained dst.stream since
// the last fork (it reads the error word back), so the staging is free to be rewritten.
int fleet_state_fork(const FleetStateRefs& dst, const FleetStateRefs& src, bool same_handle, const int32_t* dst_idx,
                     const int32_t* src_idx, int n, FleetForkScratch* k);
