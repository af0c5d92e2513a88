// fleet_batch.h -- the env handle itself (`fleet_handle` of include/fleet_hip.h) and what the host files that serve it share:
// fleet_capi.hip (the handle proper), fleet_tables.hip (what fleet_create prepares), fleet_hostpath.hip (the host-pointer entries),
// fleet_tape.hip (replays and timing), fleet_rccl.hip.  Private to the library, host code only.  What belongs here: the struct, the
// layout of its small block, the entry and error macros, the allocation helpers, and the declarations of the few functions that
// cross those files.  What does not: anything only one of them uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <tuple>
#include <vector>

#include "fleet_device.h"
#include "fleet_direct.h"
#include "fleet_state.h"

// What a prepared replay of an action tape depends on (a captured graph, the argument blocks of a direct run): reused while equal.
struct TapeKey {
  const void* tape = nullptr;
  int len = 0, dtype = 0;
  float* obs = nullptr;
  float* term = nullptr;
  double* reward = nullptr;
  uint8_t* done = nullptr;
  int mode = 0;
  uint64_t gen = 0;
  bool operator==(const TapeKey& o) const {
    return std::tie(tape, len, dtype, obs, term, reward, done, mode, gen) ==
           std::tie(o.tape, o.len, o.dtype, o.obs, o.term, o.reward, o.done, o.mode, o.gen);
  }
};

// The host step's small block: {reward f64[E], finished-episode returns f64[E], count i32, error word u32, idx i32[E], lengths
// i32[E], done u8[E]} in ONE device block = one transfer, with a pinned host mirror.  The accessors take the base of either copy.
struct FleetSmallBlock {
  size_t E = 0, bytes = 0;
  void set(int num_envs) { E = (size_t)num_envs; bytes = 25 * E + 8; }
  double* reward(char* base) const { return reinterpret_cast<double*>(base); }
  double* ep_return(char* base) const { return reinterpret_cast<double*>(base + 8 * E); }
  int32_t* count(char* base) const { return reinterpret_cast<int32_t*>(base + 16 * E); }
  uint32_t* err_word(char* base) const { return reinterpret_cast<uint32_t*>(base + 16 * E + 4); }  // FleetDev::err_any
  int32_t* idx(char* base) const { return reinterpret_cast<int32_t*>(base + 16 * E + 8); }
  int32_t* ep_len(char* base) const { return reinterpret_cast<int32_t*>(base + 20 * E + 8); }
  uint8_t* done(char* base) const { return reinterpret_cast<uint8_t*>(base + 24 * E + 8); }
};

struct FleetEnvBatch {
  FleetParams p{};
  FleetDev d{};
  int device = 0;
  hipStream_t stream = nullptr;      // the stream launches go to: the handle's own one, or an adopted one (fleet_set_stream)
  hipStream_t own_stream = nullptr;  // created with the handle, destroyed with it; never handed out of the library's control
  std::string error;
  std::vector<void*> allocs;
  // staging for the *_host entry points
  void* st_actions = nullptr;
  float* st_obs = nullptr;
  float* st_term = nullptr;
  double* st_reward = nullptr;  // (in st_small)
  uint8_t* st_done = nullptr;   // (in st_small)
  uint8_t* st_mask = nullptr;
  // host path: the small block and the compacted terminal rows; pinned host mirrors (PCIe at full rate, no pageable staging by
  // the runtime)
  FleetSmallBlock small;
  char* st_small = nullptr;
  float* st_term_compact = nullptr;
  char* pin_small = nullptr;
  void* pin_actions = nullptr;
  float* pin_term = nullptr;
  // observations to a pageable destination: pinned landing buffer (allocated at the first such step) + one event per piece
  char* pin_obs = nullptr;
  static constexpr int kObsPieces = 3;  // every transfer on the link costs ~15 us of its own: 8 pieces halve the link rate (measured)
  hipEvent_t obs_piece_ev[kObsPieces] = {};
  bool host_step_has_episodes = false;
  uint32_t last_step_err = 0;  // OR of the device error bits as of the last fleet_step_host
  double* st_dist = nullptr;
  int32_t* dev_sched = nullptr;
  FleetCold cold_host{};
  FleetCold* cold_dev = nullptr;
  FleetDev* self_dev = nullptr;
  void* st_field = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  std::vector<hipEvent_t> region_events;  // fleet_time_regions_begin / _read
  // cached tape graph
  hipGraphExec_t graph_exec = nullptr;
  TapeKey graph_key;
  // direct AQL submission of tape runs (fleet_direct.hip; FLEET_LAUNCH_DIRECT): the handle's own HSA queue, what its prepared
  // argument blocks describe, the spans of the timed runs waited for so far
  FleetDirect* direct = nullptr;
  TapeKey dq_key;
  bool dq_timed = false;  // runs carry dispatch timestamps on their first and last packets: fleet_direct_submit
  std::vector<double> dq_spans_us;
  bool direct_state_only = true;  // fleet_set_direct_state_only: dead launches of a run take the state-only twin where there is one
  // Every call that changes what a launch's argument block embeds (the handle's streams, its start schedule, its policy parameters:
  // anything a later version may move into FleetDev) bumps the generation: argument blocks prepared before it are never reused.
  uint64_t gen = 1;
  // fleet_lp_plan_dev: the planner's device scratch, kept for the next call (grows, never shrinks)
  void* lp_scratch = nullptr;
  size_t lp_scratch_bytes = 0;
  // fleet_log_summary_dev: the block partials of the log reduction (fleet_logsum.h), allocated by the first call
  void* logsum_scratch = nullptr;
  // env state (fleet_state.hip): the hash of the table contents the handle was created from (half of its fingerprint), pinned
  // staging for a blob header, what a fork keeps between calls (index pairs on the device and their pinned staging, an event)
  uint64_t table_hash = 0;
  FleetStateHeader* pin_state_hdr = nullptr;
  FleetForkScratch fork;
};

// A run submitted to the handle's own queue is not on its HIP stream: every entry point that touches the handle waits for it first.
inline int direct_drain(FleetEnvBatch* h) {
  if (!h || !h->direct) return FLEET_OK;
  return fleet_direct_wait(h->direct, &h->dq_spans_us, &h->error);
}
#define FLEET_ENTER(h)                          \
  do {                                          \
    const int _rc = direct_drain(h);            \
    if (_rc != FLEET_OK) return _rc;            \
  } while (0)

#define HIP_TRY(b, expr)                                                                         \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      (b)->error = std::string(#expr) + ": " + hipGetErrorString(_e);                            \
      return FLEET_ERR_HIP;                                                                      \
    }                                                                                            \
  } while (0)

template <typename T>
int dev_alloc(FleetEnvBatch* b, T** out, size_t count, bool zero = true) {
  void* ptr = nullptr;
  const size_t bytes = (count ? count : 1) * sizeof(T);
  HIP_TRY(b, hipMalloc(&ptr, bytes));
  b->allocs.push_back(ptr);
  if (zero) HIP_TRY(b, hipMemsetAsync(ptr, 0, bytes, b->stream));
  *out = static_cast<T*>(ptr);
  return FLEET_OK;
}

template <typename T>
int dev_upload(FleetEnvBatch* b, const T** out, const T* host, size_t count) {
  T* ptr = nullptr;
  int rc = dev_alloc(b, &ptr, count, false);
  if (rc) return rc;
  HIP_TRY(b, hipMemcpyAsync(ptr, host, count * sizeof(T), hipMemcpyHostToDevice, b->stream));
  *out = ptr;
  return FLEET_OK;
}

inline void drop_graph(FleetEnvBatch* b) {
  if (b->graph_exec) {
    (void)hipGraphExecDestroy(b->graph_exec);
    b->graph_exec = nullptr;
  }
}

inline bool act_dtype_ok(int act_dtype) { return act_dtype == FLEET_ACT_F32 || act_dtype == FLEET_ACT_F64; }

// ---- what crosses the files -------------------------------------------------------------------------------------------------------
void fleet_set_create_error(const std::string& why);  // fleet_capi.hip: what fleet_last_error(NULL) returns
// fleet_tables.hip: nullptr or why fleet_create refuses; the observation width; everything of a new handle that touches the device
const char* fleet_validate(const FleetParams* p, const FleetTables* t);
int fleet_obs_dim_of(const FleetParams* p);
int fleet_create_impl(const FleetParams* p, const FleetTables* t, int device, FleetEnvBatch* b);
