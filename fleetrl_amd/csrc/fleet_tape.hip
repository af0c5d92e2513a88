// fleet_tape.hip -- replays of an action tape and their timing: eager launches, the cached hipGraph, runs on the library's own
// queues (what makes one ready, where it is placed, how a grid is split), the description of a step instance, the placement guard's
// test hook, timed regions, per-launch timing and the handle's timer.
#include <string>
#include <vector>

#include "fleet_batch.h"

namespace {

// A tape: `tape_len` rows of [E, N] actions in the action dtype, replayed cyclically
size_t tape_row_bytes(const FleetDev& d, int act_dtype) { return (size_t)d.E * d.N * (act_dtype == FLEET_ACT_F64 ? 8 : 4); }
const void* tape_row(const FleetDev& d, const void* tape, int tape_len, int act_dtype, int i) {
  return static_cast<const char*>(tape) + (size_t)(i % tape_len) * tape_row_bytes(d, act_dtype);
}

// A batch of more wavefronts than are resident at once (256 CUs x 4 SIMDs x 5 of this kernel = 5120) runs on the library's own queues
// as two ranges of workgroups, one per queue (FLEET_LAUNCH_DIRECT); one wavefront per env or less only (the wider groups were not
// measured to gain)
#ifndef FLEET_DIRECT_SPLIT_WAVES
#define FLEET_DIRECT_SPLIT_WAVES 6144
#endif
constexpr size_t kDirectSplitWaves = FLEET_DIRECT_SPLIT_WAVES;

}  // namespace

extern "C" {

// What every submission to the library's own queues has in common: the queue exists (opened at the first use: code object, source
// hash, placement probe), the launch's argument blocks describe exactly these buffers on the handle as it is now, and everything the
// HIP stream was given before has completed.  `tape`: tape_len rows of actions (a closed-loop step: one row).
static int direct_ready(fleet_handle h, const void* tape, int tape_len, int act_dtype, float* obs, double* reward, uint8_t* done,
                        float* terminal_obs, int mode) {
  if (h->stream != h->own_stream) {
    // a run is not ordered on a HIP stream: ops queued on a borrowed stream (torch's) after the call would read its outputs too early
    // and nothing could tell them.  The handle's own stream is never handed to anybody else's ops.
    h->error = "launches through the library's own queue are not ordered on a borrowed HIP stream: fleet_use_own_stream first "
               "(the call itself waits for the stream's earlier work; fleet_wait_step / fleet_synchronize order what follows)";
    return FLEET_ERR_INVALID;
  }
  const TapeKey key{tape, tape_len, act_dtype, obs, terminal_obs, reward, done, mode, h->gen};
  if (!h->direct || !(h->dq_key == key)) {
    // (the launches in flight read the argument blocks that are about to be replaced)
    int rc = h->direct ? fleet_direct_wait(h->direct, &h->dq_spans_us, &h->error) : FLEET_OK;
    if (rc != FLEET_OK) return rc;
    if (!h->direct) {
      rc = fleet_direct_open(h->device, &h->direct, &h->error);
      if (rc != FLEET_OK) return rc;
    }
    FleetStepLaunch L;
    const hipError_t e = fleet_describe_step(h->d, tape, act_dtype, obs, reward, done, terminal_obs, &L);
    if (e != hipSuccess) {
      h->error = "direct submission serves single-step launches only (no real_time, no data log)";
      return FLEET_ERR_INVALID;
    }
    const bool split = mode == FLEET_LAUNCH_DIRECT && h->d.N <= 64 && (size_t)L.grid * (L.block / 64) >= kDirectSplitWaves;
    h->dq_key = TapeKey{};  // whatever happens below, the old key describes nothing any more
    rc = fleet_direct_prepare(h->direct, L, tape, tape_len, tape_row_bytes(h->d, act_dtype), split, h->direct_state_only, &h->error);
    if (rc != FLEET_OK) return rc;
    h->dq_key = key;
  }
  // what the stream was given before (a reset, a copy of actions ...) has completed before the first packet is written
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLEET_OK;
}

int fleet_run_tape_dev(fleet_handle h, int steps, const void* tape, int tape_len, int act_dtype, float* obs,
                       double* reward, uint8_t* done, int use_graph) {
  if (!h || steps < 0 || !tape || tape_len < 1 || !obs || !reward || !done || !act_dtype_ok(act_dtype)) {
    if (h) h->error = "fleet_run_tape_dev: bad argument";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  if (use_graph == FLEET_LAUNCH_DIRECT || use_graph == FLEET_LAUNCH_DIRECT_ONE_QUEUE) {
    // the library's own AQL packets: the launches of the run keep their state in the dies' L2s (fleet_direct.hip), the last one
    // writes it back.  Asynchronous like the other forms; not on the HIP stream -- the next call on the handle waits for the run.
    if (steps == 0) return FLEET_OK;
    const int rc = direct_ready(h, tape, tape_len, act_dtype, obs, reward, done, nullptr, use_graph);
    if (rc != FLEET_OK) return rc;
    return fleet_direct_submit(h->direct, steps, h->dq_timed, &h->error);
  }
  FLEET_ENTER(h);
  int i = 0;
  // the captured graph holds a whole number of tape cycles and at least 64 launches, however short the tape (a short tape must not
  // turn the replay into many short graphs: every hipGraphLaunch costs the host ~10 us)
  const int glen = tape_len * ((64 + tape_len - 1) / tape_len);
  if (use_graph && steps >= glen) {
    // (no generation: the graph reads everything else through device memory, and a change of stream drops it)
    const TapeKey key{tape, tape_len, act_dtype, obs, nullptr, reward, done, FLEET_LAUNCH_GRAPH, 0};
    if (!h->graph_exec || !(h->graph_key == key)) {
      drop_graph(h);
      hipGraph_t graph = nullptr;
      // capture is not allowed on the legacy null stream (what torch's default stream is): record on the handle's own
      // stream then; the graph itself is launched on the stream in use
      hipStream_t cap = h->stream ? h->stream : h->own_stream;
      HIP_TRY(h, hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
      for (int k = 0; k < glen; ++k) {
        hipError_t e = fleet_launch_step(h->d, tape_row(h->d, tape, tape_len, act_dtype, k), act_dtype, 1, obs, reward, done, nullptr,
                                         nullptr, cap);
        if (e != hipSuccess) {
          (void)hipStreamEndCapture(cap, &graph);
          if (graph) (void)hipGraphDestroy(graph);
          h->error = std::string("capture: ") + hipGetErrorString(e);
          return FLEET_ERR_HIP;
        }
      }
      HIP_TRY(h, hipStreamEndCapture(cap, &graph));
      hipError_t e = hipGraphInstantiate(&h->graph_exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (e != hipSuccess) {
        h->graph_exec = nullptr;
        h->error = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
        return FLEET_ERR_HIP;
      }
      (void)hipGraphUpload(h->graph_exec, h->stream);  // best effort: the first replay does not pay for the upload
      h->graph_key = key;
    }
    for (; i + glen <= steps; i += glen) HIP_TRY(h, hipGraphLaunch(h->graph_exec, h->stream));
  }
  for (; i < steps; ++i)
    HIP_TRY(h, fleet_launch_step(h->d, tape_row(h->d, tape, tape_len, act_dtype, i), act_dtype, 1, obs, reward, done, nullptr, nullptr,
                                 h->stream));
  return FLEET_OK;
}

int fleet_direct_queues(fleet_handle h) {
  if (!h) return FLEET_ERR_INVALID;
  return h->direct ? fleet_direct_parts(h->direct) : 0;
}

int fleet_direct_placement(fleet_handle h, int32_t map8[8], int32_t* num_xcc, int32_t* any_grid) {
  if (!h || !map8) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  if (!h->direct) {
    const int rc = fleet_direct_open(h->device, &h->direct, &h->error);
    if (rc != FLEET_OK) return rc;
  }
  int m[8], nx = 0, ag = 0;
  const int rc = fleet_direct_probed(h->direct, m, &nx, &ag);
  for (int j = 0; j < 8; ++j) map8[j] = m[j];
  if (num_xcc) *num_xcc = nx;
  if (any_grid) *any_grid = ag;
  return rc;
}

int fleet_direct_split_plan(uint32_t grid_workgroups, int split, uint32_t part_grid[2]) {
  if (!part_grid) return FLEET_ERR_INVALID;
  unsigned pg[2];
  const int parts = fleet_direct_plan(grid_workgroups, split != 0, pg);
  part_grid[0] = pg[0];
  part_grid[1] = pg[1];
  return parts;
}

// What the launch planner reads of a described launch (fleet_step_instance, fleet_step_has_state_only): the arguments checked in ONE
// place, then a FleetDev with only those fields filled in.  false: an argument out of range.
static bool described_launch(int num_envs, int num_cars, int deg_mode, int real_time, int log_data, int act_mode, int K, FleetDev* d) {
  if (num_envs < 1 || num_cars < 1 || num_cars > 65535 || deg_mode < FLEET_DEG_NONE || deg_mode > FLEET_DEG_RAINFLOW ||
      act_mode < FLEET_ACT_F32 || act_mode > FLEET_ACT_POLICY_NIGHT || K < 1)
    return false;
  static int32_t log_on;  // the selection only asks whether the log exists
  *d = FleetDev{};
  d->E = num_envs;
  d->N = num_cars;
  d->deg_mode = deg_mode;
  d->real_time = real_time != 0;
  d->log_pos = log_data ? &log_on : nullptr;
  return true;
}

int fleet_step_instance(int num_envs, int num_cars, int deg_mode, int real_time, int log_data, int act_mode, int K,
                        int has_done_count, char* name, size_t name_bytes, uint32_t* grid) {
  FleetDev d;
  if (!name || name_bytes < 1 || !grid || !described_launch(num_envs, num_cars, deg_mode, real_time, log_data, act_mode, K, &d))
    return FLEET_ERR_INVALID;
  unsigned g = 0;
  const int n = fleet_describe_step_instance(d, act_mode, K, has_done_count != 0, name, name_bytes, &g);
  *grid = g;
  return (n < 0 || (size_t)n >= name_bytes) ? FLEET_ERR_INVALID : FLEET_OK;
}

int fleet_set_direct_state_only(fleet_handle h, int on) {
  if (!h) return FLEET_ERR_INVALID;
  FLEET_ENTER(h);
  if (h->direct_state_only != (on != 0)) {
    h->direct_state_only = (on != 0);
    h->gen += 1;  // the prepared argument blocks go with a choice of kernel objects: rebuilt at the next run
  }
  return FLEET_OK;
}

int fleet_direct_packet_counts(fleet_handle h, uint64_t* live, uint64_t* state_only) {
  if (!h) return FLEET_ERR_INVALID;
  fleet_direct_packets(h->direct, live, state_only);
  return FLEET_OK;
}

int fleet_step_has_state_only(int num_envs, int num_cars, int deg_mode, int real_time, int log_data, int act_mode, int K,
                              int has_done_count, int32_t* has_twin) {
  FleetDev d;
  if (!has_twin || !described_launch(num_envs, num_cars, deg_mode, real_time, log_data, act_mode, K, &d)) return FLEET_ERR_INVALID;
  *has_twin = fleet_step_has_twin(d, act_mode, K, has_done_count != 0) ? 1 : 0;
  return FLEET_OK;
}

int fleet_debug_direct_fault(fleet_handle h, int kind, int tape_row) {
  if (!h || !h->direct) {
    if (h) h->error = "fleet_debug_direct_fault: no prepared run (run one through the library's own queue first)";
    return FLEET_ERR_INVALID;
  }
  FLEET_ENTER(h);
  return fleet_direct_fault(h->direct, kind, tape_row, &h->error);
}

int fleet_time_regions_begin(fleet_handle h, int regions, int steps, const void* tape, int tape_len, int act_dtype, float* obs,
                              double* reward, uint8_t* done, int use_graph) {
  if (!h || regions < 1 || regions > 256) return FLEET_ERR_INVALID;
  FLEET_ENTER(h);
  HIP_TRY(h, hipSetDevice(h->device));
  if (use_graph == FLEET_LAUNCH_DIRECT || use_graph == FLEET_LAUNCH_DIRECT_ONE_QUEUE) {  // the runs' own dispatch timestamps: start of the first launch -> end of the last
    h->dq_spans_us.clear();
    h->dq_timed = true;
    int rc = FLEET_OK;
    for (int r = 0; r < regions && rc == FLEET_OK; ++r) rc = fleet_run_tape_dev(h, steps, tape, tape_len, act_dtype, obs, reward, done, use_graph);
    h->dq_timed = false;
    return rc;
  }
  for (auto& e : h->region_events)
    if (e) (void)hipEventDestroy(e);
  h->region_events.assign(2 * (size_t)regions, nullptr);
  for (auto& e : h->region_events) HIP_TRY(h, hipEventCreate(&e));
  for (int r = 0; r < regions; ++r) {
    HIP_TRY(h, hipEventRecord(h->region_events[2 * r], h->stream));
    const int rc = fleet_run_tape_dev(h, steps, tape, tape_len, act_dtype, obs, reward, done, use_graph);
    if (rc != FLEET_OK) return rc;
    HIP_TRY(h, hipEventRecord(h->region_events[2 * r + 1], h->stream));
  }
  return FLEET_OK;
}

int fleet_time_regions_read(fleet_handle h, float* region_ms) {
  FLEET_ENTER(h);
  if (h && region_ms && h->region_events.empty() && !h->dq_spans_us.empty()) {  // (FLEET_ENTER has waited for the runs)
    bool ok = true;
    for (size_t r = 0; r < h->dq_spans_us.size(); ++r) {
      region_ms[r] = (float)(h->dq_spans_us[r] * 1e-3);
      ok = ok && h->dq_spans_us[r] >= 0.0;  // -1: a packet without dispatch timestamps (a queue whose profiling could not be enabled)
    }
    h->dq_spans_us.clear();
    if (!ok) {
      h->error = "fleet_time_regions_read: a run carries no dispatch timestamps";
      return FLEET_ERR_HIP;
    }
    return FLEET_OK;
  }
  if (!h || !region_ms || h->region_events.empty()) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipEventSynchronize(h->region_events.back()));
  for (size_t r = 0; r < h->region_events.size() / 2; ++r)
    HIP_TRY(h, hipEventElapsedTime(&region_ms[r], h->region_events[2 * r], h->region_events[2 * r + 1]));
  for (auto& e : h->region_events)
    if (e) (void)hipEventDestroy(e);
  h->region_events.clear();
  return FLEET_OK;
}

int fleet_time_steps_dev(fleet_handle h, int steps, const void* tape, int tape_len, int act_dtype, float* obs,
                         double* reward, uint8_t* done, float* per_launch_ms) {
  FLEET_ENTER(h);
  if (!h || steps < 1 || !tape || tape_len < 1 || !obs || !reward || !done || !per_launch_ms || !act_dtype_ok(act_dtype)) {
    if (h) h->error = "fleet_time_steps_dev: bad argument";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<hipEvent_t> ev(2 * (size_t)steps, nullptr);
  int rc = FLEET_OK;
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) rc = FLEET_ERR_HIP;
  if (rc == FLEET_OK) {
    for (int i = 0; i < steps && rc == FLEET_OK; ++i) {
      if (hipEventRecord(ev[2 * i], h->stream) != hipSuccess) rc = FLEET_ERR_HIP;
      if (fleet_launch_step(h->d, tape_row(h->d, tape, tape_len, act_dtype, i), act_dtype, 1, obs, reward, done, nullptr, nullptr,
                            h->stream) != hipSuccess)
        rc = FLEET_ERR_HIP;
      if (hipEventRecord(ev[2 * i + 1], h->stream) != hipSuccess) rc = FLEET_ERR_HIP;
    }
    if (hipStreamSynchronize(h->stream) != hipSuccess) rc = FLEET_ERR_HIP;
    for (int i = 0; i < steps && rc == FLEET_OK; ++i)
      if (hipEventElapsedTime(&per_launch_ms[i], ev[2 * i], ev[2 * i + 1]) != hipSuccess) rc = FLEET_ERR_HIP;
  }
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  if (rc != FLEET_OK) h->error = "fleet_time_steps_dev: a HIP call failed";
  return rc;
}

int fleet_timer_start(fleet_handle h) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipEventRecord(h->ev_start, h->stream));
  return FLEET_OK;
}

int fleet_timer_stop(fleet_handle h, float* elapsed_ms) {
  FLEET_ENTER(h);
  if (!h || !elapsed_ms) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipEventRecord(h->ev_stop, h->stream));
  HIP_TRY(h, hipEventSynchronize(h->ev_stop));
  HIP_TRY(h, hipEventElapsedTime(elapsed_ms, h->ev_start, h->ev_stop));
  return FLEET_OK;
}

int fleet_timer_mark(fleet_handle h) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipEventRecord(h->ev_stop, h->stream));
  return FLEET_OK;
}

int fleet_timer_read(fleet_handle h, float* elapsed_ms) {
  FLEET_ENTER(h);
  if (!h || !elapsed_ms) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipEventSynchronize(h->ev_stop));
  HIP_TRY(h, hipEventElapsedTime(elapsed_ms, h->ev_start, h->ev_stop));
  return FLEET_OK;
}

}  // extern "C"
