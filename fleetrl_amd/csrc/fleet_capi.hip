// fleet_capi.hip -- the env handle proper of the C ABI declared in include/fleet_hip.h (libfleet_hip.so): create and destroy,
// streams, the setters of the cold block, the *_dev steps, getters, the data log, error reporting, the state entries, the self-tests.
// The struct and what the host files share: fleet_batch.h.  What fleet_create prepares: fleet_tables.hip.  The entries that take host
// pointers: fleet_hostpath.hip.  Tape replays and timing: fleet_tape.hip.  RCCL: fleet_rccl.hip.
// There is no CPU path in this library: without a HIP device fleet_create fails with FLEET_ERR_NODEVICE.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "fleet_batch.h"
#include "fleet_logsum.h"
#include "fleet_lp.h"

static thread_local std::string g_create_error;

// Name the first env that carries device error bits (the reference raises at the offending line: fleet_environment.py:610,
// rainflow_sei_degradation.py:164-167,179-180,209-210; running off the table is a KeyError of its `db.loc[...]`).
static const char* deverr_names(uint32_t bits, char* buf, size_t n) {
  snprintf(buf, n, "%s%s%s%s%s%s%s",
           (bits & FLEET_DEVERR_PLACEMENT) ? " placement: a workgroup of a run on the library's own queue ran on another die than probed, the run's results are void;" : "",
           (bits & FLEET_DEVERR_INTERNAL) ? " internal: inconsistent launch arguments;" : "",
           (bits & FLEET_DEVERR_OBS_FORMAT) ? " observation format not recognized;" : "",
           (bits & FLEET_DEVERR_NEG_LIFE) ? " life degradation is negative;" : "",
           (bits & FLEET_DEVERR_SOH_MISMATCH) ? " degradation calculation is not correct;" : "",
           (bits & FLEET_DEVERR_DOD_RANGE) ? " DoD too large;" : "",
           (bits & FLEET_DEVERR_TABLE_END) ? " the episode runs past the last table row;" : "");
  return buf;
}

void fleet_set_create_error(const std::string& why) { g_create_error = why; }

// Every change of the cold block: argument blocks prepared before it are never reused (gen), the stream has drained before `edit`
// changes the host mirror, and the mirror goes to the device in one copy (the block lives in device memory, so captured graphs stay
// valid).  A status other than FLEET_OK from `edit` ends the call there.
template <typename Edit>
static int push_cold(fleet_handle h, Edit edit) {
  h->gen += 1;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const int rc = edit();
  if (rc != FLEET_OK) return rc;
  HIP_TRY(h, hipMemcpy(h->cold_dev, &h->cold_host, sizeof(FleetCold), hipMemcpyHostToDevice));
  return FLEET_OK;
}

extern "C" {

int fleet_obs_dim(const FleetParams* p) {
  if (!p || p->num_cars < 1) return -1;
  return fleet_obs_dim_of(p);
}

int fleet_create(const FleetParams* p, const FleetTables* t, int device, fleet_handle* out) {
  if (out) *out = nullptr;
  if (const char* why = fleet_validate(p, t)) {
    g_create_error = why;
    return FLEET_ERR_INVALID;
  }
  if (!out) {
    g_create_error = "null output handle";
    return FLEET_ERR_INVALID;
  }
  FleetEnvBatch* b = new FleetEnvBatch();
  int rc = fleet_create_impl(p, t, device, b);
  if (rc != FLEET_OK) {
    g_create_error = b->error;
    fleet_destroy(b);
    return rc;
  }
  *out = b;
  return FLEET_OK;
}

int fleet_destroy(fleet_handle h) {
  if (!h) return FLEET_OK;
  (void)hipSetDevice(h->device);
  if (h->direct) fleet_direct_close(h->direct);  // waits for a run in flight
  h->direct = nullptr;
  (void)hipStreamSynchronize(h->stream);
  drop_graph(h);
  for (void* ptr : h->allocs) (void)hipFree(ptr);
  for (void* ptr : {(void*)h->pin_small, h->pin_actions, (void*)h->pin_term, (void*)h->pin_obs})
    if (ptr) (void)hipHostFree(ptr);
  for (auto& e : h->obs_piece_ev)
    if (e) (void)hipEventDestroy(e);
  if (h->dev_sched) (void)hipFree(h->dev_sched);
  if (h->lp_scratch) (void)hipFree(h->lp_scratch);
  if (h->logsum_scratch) (void)hipFree(h->logsum_scratch);
  fleet_state_fork_release(&h->fork);
  if (h->pin_state_hdr) (void)hipHostFree(h->pin_state_hdr);
  for (auto& e : h->region_events)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_start) (void)hipEventDestroy(h->ev_start);
  if (h->ev_stop) (void)hipEventDestroy(h->ev_stop);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return FLEET_OK;
}

const char* fleet_last_error(fleet_handle h) { return h ? h->error.c_str() : g_create_error.c_str(); }

int fleet_set_stream(fleet_handle h, void* hip_stream) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  h->gen += 1;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // what was enqueued on the stream in use so far is finished before the switch
  drop_graph(h);
  // the handle's own stream is kept (fleet_set_stream(h, fleet_own_stream) or a later fleet_use_own_stream goes back to it);
  // an adopted stream is only borrowed: the caller keeps it alive while the handle uses it
  h->stream = static_cast<hipStream_t>(hip_stream);
  return FLEET_OK;
}

int fleet_use_own_stream(fleet_handle h) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  h->gen += 1;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  drop_graph(h);
  h->stream = h->own_stream;
  return FLEET_OK;
}

int fleet_synchronize(fleet_handle h) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLEET_OK;
}

int fleet_stream_query(fleet_handle h) {
  if (!h) return FLEET_ERR_INVALID;
  if (h->direct && fleet_direct_busy(h->direct)) return -1;
  const hipError_t e = hipStreamQuery(h->stream);
  if (e == hipSuccess) return FLEET_OK;
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();
    return -1;
  }
  h->error = std::string("hipStreamQuery: ") + hipGetErrorString(e);
  return FLEET_ERR_HIP;
}

int fleet_set_start_schedule(fleet_handle h, const int32_t* starts, int n_episodes) {
  FLEET_ENTER(h);
  if (!h || n_episodes < 0 || (n_episodes > 0 && !starts)) return FLEET_ERR_INVALID;
  return push_cold(h, [&]() -> int {
    if (h->dev_sched) {
      (void)hipFree(h->dev_sched);
      h->dev_sched = nullptr;
    }
    h->cold_host.sched = nullptr;
    h->cold_host.sched_n = 0;
    if (n_episodes > 0) {
      const size_t n = (size_t)n_episodes * h->d.E;
      for (size_t i = 0; i < n; ++i)
        if (starts[i] < 0 || starts[i] > h->d.T - 1) {
          h->error = "start row outside the table";
          return FLEET_ERR_INVALID;
        }
      HIP_TRY(h, hipMalloc((void**)&h->dev_sched, n * sizeof(int32_t)));
      HIP_TRY(h, hipMemcpy(h->dev_sched, starts, n * sizeof(int32_t), hipMemcpyHostToDevice));
      h->cold_host.sched = h->dev_sched;
      h->cold_host.sched_n = n_episodes;
    }
    return FLEET_OK;
  });
}

int fleet_reset_dev(fleet_handle h, const uint8_t* mask, float* obs) {
  FLEET_ENTER(h);
  if (!h || !obs) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, fleet_launch_reset(h->d, mask, obs, h->stream));
  return FLEET_OK;
}

int fleet_step_dev(fleet_handle h, const void* actions, int act_dtype, float* obs, double* reward, uint8_t* done,
                   float* terminal_obs) {
  FLEET_ENTER(h);
  if (!h || !actions || !obs || !reward || !done || !act_dtype_ok(act_dtype)) {
    if (h) h->error = "fleet_step_dev: null buffer or bad action dtype";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, fleet_launch_step(h->d, actions, act_dtype, 1, obs, reward, done, terminal_obs, nullptr, h->stream));
  return FLEET_OK;
}

int fleet_step_many_dev(fleet_handle h, int K, const void* actions, int act_dtype, float* obs, double* reward_sum,
                        int32_t* done_count) {
  FLEET_ENTER(h);
  if (!h || K < 1 || !actions || !obs || !reward_sum || !act_dtype_ok(act_dtype)) {
    if (h) h->error = "fleet_step_many_dev: bad argument";
    return FLEET_ERR_INVALID;
  }
  if (!h->d.auto_reset) {
    h->error = "fleet_step_many_dev needs auto_reset = 1";
    return FLEET_ERR_INVALID;
  }
  if (h->d.real_time) {
    h->error = "fleet_step_many_dev is not available with real_time = 1 (each launch already spans a variable number of rows)";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  // K == 1 without done_count is the single-step kernel (it writes the per-step reward = the sum of one, and the done flag
  // to the staging buffer); with done_count the launcher takes the multi-step kernel, which counts episode ends
  HIP_TRY(h, fleet_launch_step(h->d, actions, act_dtype, K, obs, reward_sum, h->st_done, nullptr, done_count, h->stream));
  return FLEET_OK;
}

int fleet_lp_plan_dev(fleet_handle h, int H, void* actions, int act_dtype, double* soc_plan, double* bound, double* plan_cost,
                      int32_t* status) {
  FLEET_ENTER(h);
  if (!h || H < 1 || !actions || !bound || !plan_cost || !status || !act_dtype_ok(act_dtype)) {
    if (h) h->error = "fleet_lp_plan_dev: bad argument";
    return FLEET_ERR_INVALID;
  }
  if (h->d.real_time) {
    h->error = "fleet_lp_plan_dev is not available with real_time = 1 (the model has a fixed step)";
    return FLEET_ERR_INVALID;
  }
  const size_t lanes = (size_t)h->d.E * h->d.N;
  if ((size_t)H > (size_t)INT32_MAX / 16 || fleet_lp_scratch_bytes(1, H) > ((size_t)1 << 40) / lanes) {
    h->error = "fleet_lp_plan_dev: horizon too long for this batch";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  // the plan is replayed on the episode it was made for: every env must have H rows left in its running episode
  std::vector<EnvRec> env(h->d.E);
  HIP_TRY(h, hipMemcpyAsync(env.data(), h->d.env, env.size() * sizeof(EnvRec), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int e = 0; e < h->d.E; ++e) {
    const int t = env[e].h.t, t_end = env[e].h.t_end;
    const bool done = ((uint32_t)env[e].start_done >> 31) != 0u;
    if (done || t < 0 || (int64_t)t + H > (int64_t)t_end || (int64_t)t + H > (int64_t)h->d.T) {
      h->error = "fleet_lp_plan_dev: env " + std::to_string(e) + " at row " + std::to_string(t) + " has " +
                 std::to_string(done ? 0 : std::max(0, std::min(t_end, h->d.T) - t)) + " rows left in its episode, fewer than H = " +
                 std::to_string(H);
      return FLEET_ERR_INVALID;
    }
  }
  const size_t need = fleet_lp_scratch_bytes(lanes, H);
  if (need > h->lp_scratch_bytes) {
    if (h->lp_scratch) HIP_TRY(h, hipFree(h->lp_scratch));
    h->lp_scratch = nullptr;
    h->lp_scratch_bytes = 0;
    HIP_TRY(h, hipMalloc(&h->lp_scratch, need));
    h->lp_scratch_bytes = need;
  }
  FleetLpArgs a{};
  a.H = H;
  a.act_dtype = act_dtype;
  a.actions = actions;
  a.soc_plan = soc_plan;
  a.bound = bound;
  a.plan_cost = plan_cost;
  a.status = status;
  a.scratch = static_cast<double*>(h->lp_scratch);
  HIP_TRY(h, fleet_launch_lp_plan(h->d, a, h->stream));
  return FLEET_OK;
}

int fleet_set_night_policy(fleet_handle h, int charging_hour, int charging_minute, int max_hours) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  // charging_hour may be 24 (the reference's own edge when the window would open exactly at midnight: never opens)
  if (charging_hour < 0 || charging_hour > 24 || charging_minute < 0 || charging_minute > 59 || max_hours < 0 ||
      max_hours > 24 * 365) {
    h->error = "fleet_set_night_policy: argument out of range";
    return FLEET_ERR_INVALID;
  }
  return push_cold(h, [&]() -> int {
    h->cold_host.night_hour = charging_hour;
    h->cold_host.night_minute = charging_minute;
    h->cold_host.night_limit_s = 3600 * max_hours;
    std::vector<int32_t> idle((size_t)h->d.E, FLEET_NIGHT_IDLE);
    HIP_TRY(h, hipMemcpy(h->cold_host.night_start, idle.data(), idle.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return FLEET_OK;
  });
}

int fleet_set_rainflow_count_all(fleet_handle h, int on) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  return push_cold(h, [&]() -> int {
    h->cold_host.rf_count_all = on ? 1 : 0;
    return FLEET_OK;
  });
}

int fleet_rollout_policy_dev(fleet_handle h, int policy, int K, float* obs, double* reward_sum, int32_t* done_count) {
  FLEET_ENTER(h);
  if (!h || K < 1 || !obs || !reward_sum ||
      (policy != FLEET_ACT_POLICY_UNCONTROLLED && policy != FLEET_ACT_POLICY_DISTRIBUTED && policy != FLEET_ACT_POLICY_NIGHT)) {
    if (h) h->error = "fleet_rollout_policy_dev: bad argument";
    return FLEET_ERR_INVALID;
  }
  if (policy == FLEET_ACT_POLICY_NIGHT && h->cold_host.night_hour < 0) {
    h->error = "fleet_rollout_policy_dev: FLEET_ACT_POLICY_NIGHT needs fleet_set_night_policy first";
    return FLEET_ERR_INVALID;
  }
  if (!h->d.auto_reset) {
    h->error = "fleet_rollout_policy_dev needs auto_reset = 1";
    return FLEET_ERR_INVALID;
  }
  if (h->d.real_time) {
    h->error = "fleet_rollout_policy_dev is not available with real_time = 1";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  // K >= 1 always takes the multi-step kernel (policies are only compiled into it); done_count may be NULL
  HIP_TRY(h, fleet_launch_step(h->d, nullptr, policy, K, obs, reward_sum, h->st_done, nullptr, done_count, h->stream));
  return FLEET_OK;
}

static size_t field_bytes(const FleetDev& d, int field) {
  const size_t E = d.E, EN = (size_t)d.E * d.N;
  size_t bytes = 0;
  switch (field) {
    case FLEET_F_SOC: case FLEET_F_SOH: case FLEET_F_SOC_DEG: case FLEET_F_TARGET_SOC: case FLEET_F_FD_CYC:
    case FLEET_F_FD_CAL: case FLEET_F_SEI_L: bytes = EN * 8; break;
    case FLEET_F_HOURS_LEFT: case FLEET_F_RF_LEN: case FLEET_F_RF_CYCLES: case FLEET_F_RF_STACK: bytes = EN * 4; break;
    case FLEET_F_CASHFLOW: case FLEET_F_EP_RETURN: case FLEET_F_LAST_EP_RETURN: case FLEET_F_PENALTY_RECORD:
    case FLEET_F_LAST_EP_LEN_F64:
    bytes = E * 8; break;
    case FLEET_F_TIME_IDX: case FLEET_F_START_IDX: case FLEET_F_EP_LEN: case FLEET_F_LAST_EP_LEN: case FLEET_F_ERROR_BITS:
    case FLEET_F_EPISODES: case FLEET_F_RF_UNTIL: bytes = E * 4; break;
    case FLEET_F_DONE: bytes = E; break;
    default: break;
  }
  return bytes;
}

int fleet_get_dev(fleet_handle h, int field, void* out_dev) {
  FLEET_ENTER(h);
  if (!h || !out_dev) return FLEET_ERR_INVALID;
  if (!field_bytes(h->d, field)) {
    h->error = "fleet_get_dev: unknown field";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, fleet_launch_gather_field(h->d, field, out_dev, h->stream));
  return FLEET_OK;
}

int fleet_get(fleet_handle h, int field, void* out) {
  FLEET_ENTER(h);
  if (!h || !out) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  const size_t bytes = field_bytes(h->d, field);
  if (!bytes) {
    h->error = "fleet_get: unknown field";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, fleet_launch_gather_field(h->d, field, h->st_field, h->stream));
  HIP_TRY(h, hipMemcpyAsync(out, h->st_field, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLEET_OK;
}

int fleet_get_dist_factor(fleet_handle h, double* out) {
  FLEET_ENTER(h);
  if (!h || !out) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, fleet_launch_dist_factor(h->d, h->st_dist, h->stream));
  HIP_TRY(h, hipMemcpyAsync(out, h->st_dist, (size_t)h->d.E * h->d.N * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLEET_OK;
}

int fleet_log_capacity(fleet_handle h) { return (h && h->d.log_pos) ? h->d.log_cap : 0; }

int fleet_log_dropped(fleet_handle h, int64_t* rows) {
  FLEET_ENTER(h);
  if (!h || !rows || !h->d.log_pos) {
    if (h) h->error = "fleet_log_dropped: the data log is off or a null pointer";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<int32_t> pos((size_t)h->d.E);
  HIP_TRY(h, hipMemcpyAsync(pos.data(), h->d.log_pos, pos.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  int64_t n = 0;
  for (int32_t p : pos) n += p > h->d.log_cap ? p - h->d.log_cap : 0;
  *rows = n;
  return FLEET_OK;
}

int fleet_log_read(fleet_handle h, int32_t* pos, int32_t* row, double* env, double* ev, float* obs) {
  FLEET_ENTER(h);
  if (!h || !h->d.log_pos) {
    if (h) h->error = "fleet_log_read: the data log is off (FleetParams.log_data = 0)";
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  const FleetDev& d = h->d;
  const size_t rows = (size_t)d.log_cap * d.E;
  if (pos) HIP_TRY(h, hipMemcpyAsync(pos, d.log_pos, (size_t)d.E * 4, hipMemcpyDeviceToHost, h->stream));
  if (row) HIP_TRY(h, hipMemcpyAsync(row, d.log_row, rows * 4, hipMemcpyDeviceToHost, h->stream));
  if (env) HIP_TRY(h, hipMemcpyAsync(env, d.log_env, rows * 4 * 8, hipMemcpyDeviceToHost, h->stream));
  if (ev) HIP_TRY(h, hipMemcpyAsync(ev, d.log_ev, rows * 4 * d.N * 8, hipMemcpyDeviceToHost, h->stream));
  if (obs) HIP_TRY(h, hipMemcpyAsync(obs, d.log_obs, rows * (size_t)d.obs_dim * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return FLEET_OK;
}

int fleet_log_clear(fleet_handle h) {
  FLEET_ENTER(h);
  if (!h || !h->d.log_pos) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->d.log_pos, 0, (size_t)h->d.E * 4, h->stream));
  return FLEET_OK;
}

int fleet_log_summary_dev(fleet_handle h, const FleetLogSummaryArgs* args, size_t args_size) {
  FLEET_ENTER(h);  // a run on the library's own queue is not on the stream: waited for, as fleet_log_read does
  if (!h) return FLEET_ERR_INVALID;
  const FleetDev& d = h->d;
  const char* why = nullptr;
  if (!d.log_pos) why = "the data log is off (FleetParams.log_data = 0)";
  else if (!args || args_size != sizeof(FleetLogSummaryArgs)) why = "null args or args_size is not sizeof(FleetLogSummaryArgs)";
  else if (!args->scal) why = "null scal";
  else if (args->drop_last < 0) why = "drop_last < 0";
  else if (args->hist && (args->bins < 1 || args->bins > kLogsumMaxBins)) why = "bins outside 1..256";
  else if (!(args->hi > args->lo)) why = "hi <= lo or a NaN bound";
  else if (args->hist_ev < -1 || args->hist_ev >= d.N) why = "hist_ev outside -1..N-1";
  const int step_s = h->cold_host.step_s;
  if (!why && (args->prof_sum || args->prof_cnt)) {
    if (d.tab_finish) why = "prof_*: an irregular time grid has no time-of-day slots";
    else if (step_s < 60 || step_s % 60 || 1440 % (step_s / 60)) why = "prof_*: the step is no whole divisor of a day in minutes";
  }
  if (!why && (d.log_cap + kLogsumRows - 1) / kLogsumRows > 65535) why = "log_capacity above 64 * 65535 rows";
  if (why) {
    h->error = std::string("fleet_log_summary_dev: ") + why;
    return FLEET_ERR_INVALID;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  if (!h->logsum_scratch) HIP_TRY(h, hipMalloc(&h->logsum_scratch, fleet_logsum_scratch_bytes(d.E, d.N, d.log_cap)));
  FleetLogsumArgs a{};
  a.drop_last = args->drop_last;
  a.bins = args->hist ? args->bins : 1;
  a.hist_ev = args->hist_ev;
  a.calc_deg = d.deg_mode != FLEET_DEG_NONE;
  a.minutes_per_step = (args->prof_sum || args->prof_cnt) ? step_s / 60 : 0;
  a.lo = args->lo;
  a.hi = args->hi;
  a.price_multiplier = h->p.price_multiplier;
  a.tab_hm = h->cold_host.tab_hm;
  a.scal = args->scal;
  a.deg_sum = args->deg_sum;
  a.soh_last = args->soh_last;
  a.prof_sum = args->prof_sum;
  a.prof_cnt = args->prof_cnt;
  a.hist = args->hist;
  a.scratch = h->logsum_scratch;
  HIP_TRY(h, fleet_launch_log_summary(d, a, h->stream));
  return FLEET_OK;
}

int fleet_get_stream(fleet_handle h, void** hip_stream) {
  FLEET_ENTER(h);
  if (!h || !hip_stream) return FLEET_ERR_INVALID;
  *hip_stream = static_cast<void*>(h->stream);
  return FLEET_OK;
}

int fleet_check_errors(fleet_handle h) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  std::vector<uint32_t> e(h->d.E);
  int rc = fleet_get(h, FLEET_F_ERROR_BITS, e.data());
  if (rc) return rc;
  for (int i = 0; i < h->d.E; ++i)
    if (e[i]) {
      std::vector<int32_t> t(h->d.E);
      (void)fleet_get(h, FLEET_F_TIME_IDX, t.data());
      char names[400], buf[640];
      snprintf(buf, sizeof buf, "device error bits 0x%x on env %d at table row %d of %d:%s (FLEET_DEVERR_* in fleet_hip.h)", e[i], i, t[i],
               h->d.T, deverr_names(e[i], names, sizeof names));
      h->error = buf;
      return FLEET_ERR_STATE;
    }
  return FLEET_OK;
}

// ---- env state: save, load, fork (fleet_state.hip does the work; here: what belongs to the handle) -------------------------------
static FleetStateRefs state_refs(fleet_handle h) {
  return FleetStateRefs{&h->p, &h->d, &h->cold_host, h->cold_dev, &h->dev_sched, h->table_hash, h->stream, h->pin_state_hdr, &h->error};
}

// The handle's error word, read back (drains the stream): a handle with device error bits raised is neither saved nor forked.
static int state_clean(fleet_handle h, const char* who) {
  uint32_t any = 0;
  HIP_TRY(h, hipMemcpyAsync(&any, h->d.err_any, sizeof any, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (any) {
    char names[400], buf[640];
    snprintf(buf, sizeof buf, "%s: the handle has device error bits raised (0x%x:%s) and its state is not saved or forked", who, any,
             deverr_names(any, names, sizeof names));
    h->error = buf;
    return FLEET_ERR_STATE;
  }
  return FLEET_OK;
}

static int state_save(fleet_handle h, void* blob, uint64_t bytes, bool host) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  if (!h->pin_state_hdr) HIP_TRY(h, hipHostMalloc((void**)&h->pin_state_hdr, sizeof(FleetStateHeader), hipHostMallocDefault));
  const int rc = state_clean(h, host ? "fleet_state_save_host" : "fleet_state_save_dev");
  if (rc != FLEET_OK) return rc;
  return fleet_state_save(state_refs(h), blob, bytes, host);
}

static int state_load(fleet_handle h, const void* blob, uint64_t bytes, bool host) {
  FLEET_ENTER(h);
  if (!h) return FLEET_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  const int rc = fleet_state_load(state_refs(h), blob, bytes, host);
  if (rc != FLEET_OK) return rc;
  // the start schedule and the policy parameters may have changed: nothing prepared before is reused (FleetEnvBatch::gen); what the host
  // path remembers of its last step belongs to the state that has just been replaced
  h->gen += 1;
  h->host_step_has_episodes = false;
  h->last_step_err = 0;
  return FLEET_OK;
}

int fleet_state_bytes(fleet_handle h, uint64_t* bytes) {
  if (!h || !bytes) return FLEET_ERR_INVALID;
  *bytes = fleet_state_blob_bytes(state_refs(h));
  return FLEET_OK;
}
int fleet_state_save_dev(fleet_handle h, void* blob_dev, uint64_t bytes) { return state_save(h, blob_dev, bytes, false); }
int fleet_state_save_host(fleet_handle h, void* blob_host, uint64_t bytes) { return state_save(h, blob_host, bytes, true); }
int fleet_state_load_dev(fleet_handle h, const void* blob_dev, uint64_t bytes) { return state_load(h, blob_dev, bytes, false); }
int fleet_state_load_host(fleet_handle h, const void* blob_host, uint64_t bytes) { return state_load(h, blob_host, bytes, true); }

int fleet_fork_envs(fleet_handle dst, fleet_handle src, const int32_t* dst_idx_host, const int32_t* src_idx_host, int n) {
  FLEET_ENTER(dst);
  if (!dst || !src) return FLEET_ERR_INVALID;
  if (src != dst) {
    const int rc = direct_drain(src);
    if (rc != FLEET_OK) {
      dst->error = "fleet_fork_envs: the source handle: " + src->error;
      return rc;
    }
  }
  if (dst->device != src->device) {
    dst->error = "fleet_fork_envs: the two handles are on different devices";
    return FLEET_ERR_INVALID;
  }
  if (dst->d.log_pos || src->d.log_pos) {
    dst->error = "fleet_fork_envs: a handle with the data log on is not forked (log_data = 1)";
    return FLEET_ERR_UNSUPPORTED;
  }
  HIP_TRY(dst, hipSetDevice(dst->device));
  int rc = state_clean(dst, "fleet_fork_envs");
  if (rc != FLEET_OK) return rc;
  if (src != dst && (rc = state_clean(src, "fleet_fork_envs")) != FLEET_OK) {
    dst->error = src->error;
    return rc;
  }
  return fleet_state_fork(state_refs(dst), state_refs(src), src == dst, dst_idx_host, src_idx_host, n, &dst->fork);
}

}  // extern "C"

// Both self-tests: `words` 64-bit result words on `device`, cleared, filled by `launch`, read back into `out`.
static int selftest_run(int device, uint64_t n, uint64_t seed, void* out, size_t words,
                        hipError_t (*launch)(unsigned long long, unsigned long long, unsigned long long*, hipStream_t)) {
  if (!out || n == 0) return FLEET_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FLEET_ERR_NODEVICE;
  if (device < 0 || device >= ndev) return FLEET_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return FLEET_ERR_HIP;
  unsigned long long* dev = nullptr;
  unsigned long long host[2] = {0, 0};
  const size_t bytes = words * sizeof host[0];
  if (hipMalloc(&dev, bytes) != hipSuccess) return FLEET_ERR_HIP;
  int rc = FLEET_OK;
  if (hipMemset(dev, 0, bytes) != hipSuccess || launch(n, seed, dev, nullptr) != hipSuccess ||
      hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    rc = FLEET_ERR_HIP;
  (void)hipFree(dev);
  memcpy(out, host, bytes);
  return rc;
}

int fleet_selftest_stress(int device, uint64_t n_samples, uint64_t seed, double* max_rel_err) {
  return selftest_run(device, n_samples, seed, max_rel_err, 1, fleet_launch_selftest_stress);
}

int fleet_selftest_division(int device, uint64_t n_pairs, uint64_t seed, uint64_t* mismatches) {
  return selftest_run(device, n_pairs, seed, mismatches, 2, fleet_launch_selftest_division);
}
