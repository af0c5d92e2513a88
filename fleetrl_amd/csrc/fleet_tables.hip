// fleet_tables.hip -- what fleet_create prepares: the checks on the caller's parameters and tables, the observation width, the
// tables re-packed into the rows the kernels read (physics, segments, observation tails), and fleet_create_impl, which uploads them
// and allocates the env state and the staging of the host entries.  Apart from those uploads: pure host arithmetic.
#include <cmath>
#include <cstring>

#include "fleet_batch.h"

int fleet_obs_dim_of(const FleetParams* p) {
  const int N = p->num_cars, L = p->price_lookahead, B = p->bl_pv_lookahead;
  int dim = 2 * N + (L + 1) * 2;
  if (p->include_building && p->include_pv)
    dim += 2 * (B + 1);
  else if (p->include_building || p->include_pv)
    dim += B + 1;
  if (p->aux) {
    dim += 5 * N + 1 + 6;
    if (p->include_building) dim += 3;
  }
  return dim;
}

const char* fleet_validate(const FleetParams* p, const FleetTables* t) {
  if (!p || !t) return "null params/tables";
  if (p->abi_version != FLEET_ABI_VERSION) return "abi_version mismatch";
  if (p->struct_bytes != (int)sizeof(FleetParams)) return "FleetParams size mismatch";
  if (p->num_envs < 1 || p->num_cars < 1 || p->table_rows < 2) return "num_envs/num_cars/table_rows out of range";
  if (p->num_cars > 65535) return "num_cars: at most 65535 EVs per env";  // (the step kernel's packed argument, fleet_kernels.hip `p_N`; filled by step_args, fleet_step_plan.h)
  if (p->episode_steps < 1 || p->steps_per_hour < 1) return "episode_steps/steps_per_hour out of range";
  if (p->episode_steps >= FLEET_MAX_EPISODE_STEPS) return "episode_steps exceeds 2^29 - 1 (the env head's sample count is 29 bits wide)";
  if (p->price_lookahead < 0 || p->bl_pv_lookahead < 0) return "negative look-ahead";
  if (p->deg_mode < FLEET_DEG_NONE || p->deg_mode > FLEET_DEG_RAINFLOW) return "unknown deg_mode";
  if (p->deg_mode == FLEET_DEG_RAINFLOW && p->init_soh != 1.0)
    return "rainflow/SEI degradation needs init_soh == 1.0 (the reference's used-battery branch is ill-defined, quirk Q4)";
  // the rainflow stack size travels in a 26-bit field of the hot record (fleet_device.h HOT_PACK)
  if (p->deg_mode == FLEET_DEG_RAINFLOW && p->episode_steps > FLEET_MAX_STACK_ROWS - 3)
    return "rainflow/SEI degradation: episode_steps exceeds 67 million (the packed rainflow stack size is 26 bits wide)";
  // ... and the kernels address an EV's rainflow row as (its env's rows) + a 32-bit byte offset
  if (p->deg_mode == FLEET_DEG_RAINFLOW && (uint64_t)p->num_cars * ((uint64_t)p->episode_steps + 24) * 8ull >= (1ull << 32))
    return "rainflow/SEI degradation: num_cars x episode_steps too large (the rainflow rows of one env exceed 4 GiB)";
  if (p->table_rows >= 0x3FFFFFFF) return "table_rows exceeds 2^30 - 1 (segment ends are 30 bits wide)";
  if (t->finish_row)
    for (int r = 0; r < p->table_rows; ++r) {
      if (t->finish_row[r] >= p->table_rows) return "finish_row entry outside the table";
      if (p->deg_mode == FLEET_DEG_RAINFLOW && t->finish_row[r] - r > FLEET_MAX_STACK_ROWS - 3)
        return "rainflow/SEI degradation: an episode spans more than 67 million rows (the packed rainflow stack size is 26 bits wide)";
    }
  if (t->lookahead_row)
    for (size_t k = 0; k < (size_t)p->table_rows * (size_t)t->lookahead_cols; ++k)
      if (t->lookahead_row[k] >= p->table_rows) return "lookahead_row entry outside the table";
  if (p->normalize && p->include_pv && !p->include_building)
    return "normalize with pv but without building load crashes in the reference (quirk Q4); unsupported";
  if ((t->dt_row != nullptr) != (t->finish_row != nullptr) || (t->dt_row && (!t->lookahead_row || t->lookahead_cols < 1)))
    return "irregular-grid tables must be given together (dt_row, finish_row, lookahead_row)";
  if (t->dt_row && !p->real_time) return "an irregular time grid needs real_time = 1";
  if (t->lookahead_row && (t->lookahead_cols < p->price_lookahead || t->lookahead_cols < p->bl_pv_lookahead))
    return "lookahead_cols smaller than a look-ahead";
  if (p->log_capacity < 0) return "negative log_capacity";
  if (t->pick_rows && t->n_pick_rows < 1) return "empty pick_rows";
  if (p->start_lo < 0 || p->start_hi < p->start_lo || p->start_hi > (t->pick_rows ? t->n_pick_rows : p->table_rows) - 1)
    return "start range outside the table";
  if (t->pick_rows)
    for (int i = 0; i < t->n_pick_rows; ++i)
      if (t->pick_rows[i] < 0 || t->pick_rows[i] > p->table_rows - 1) return "pick_rows entry outside the table";
  if (!t->there || !t->time_left || !t->soc_on_return || !t->delu || !t->tariff || !t->prc || !t->trc || !t->load ||
      !t->pv || !t->hour || !t->minute || !t->month || !t->weekday)
    return "a required table pointer is null";
  return nullptr;
}

// hourly look-ahead row: `resample("H").first()` of the slice starting at t (observer_bl_pv.py:50-80):
// bucket 0 = row t, bucket k>=1 = first row of clock hour floor_hour(t)+k.
static inline int lookahead_row(const FleetParams& p, const FleetTables& tb, int t, int k) {
  if (k == 0) return t;
  if (tb.lookahead_row) {  // irregular grid: tabulated by date on the host
    const int r = tb.lookahead_row[(size_t)t * tb.lookahead_cols + (k - 1)];
    return r < 0 ? p.table_rows - 1 : r;
  }
  int r = ((t + p.hour_phase) / p.steps_per_hour + k) * p.steps_per_hour - p.hour_phase;
  return r > p.table_rows - 1 ? p.table_rows - 1 : r;
}

// Env-level observation blocks are a pure function of the table row: assemble (and normalise) them once, in
// float64 with the reference's operation order, and store the float32 words the reference would emit.
//   block A: price[L+1] | tariff[L+1] | building_load[B+1]* | pv[B+1]*      (observer_bl_pv.py:50-80)
//   block B: evse | grid_cap† | avail_grid_cap† | possible_avg_action† | month/week/hour sin,cos  (:92-107)
static void build_tail_rows(const FleetParams& p, const FleetTables& t, int tail_a, int tail_b, int stride, std::vector<float>& out) {
  const int T = p.table_rows, L = p.price_lookahead, B = p.bl_pv_lookahead, N = p.num_cars;
  const bool norm = p.normalize != 0;
  out.assign((size_t)T * stride, 0.0f);
  const double two_pi = 2 * M_PI;
  for (int r = 0; r < T; ++r) {
    float* o = out.data() + (size_t)r * stride;
    int k0 = 0;
    for (int k = 0; k <= L; ++k) {
      double v = (t.delu[lookahead_row(p, t, r, k)] + p.fixed_markup) * p.variable_multiplier;
      if (norm) v = (v - p.min_price) / (p.max_price - p.min_price);
      o[k0++] = (float)v;
    }
    for (int k = 0; k <= L; ++k) {
      double v = t.tariff[lookahead_row(p, t, r, k)] * (1 - p.feed_in_deduction);
      if (norm) v = (v - p.min_tariff) / (p.max_tariff - p.min_tariff);
      o[k0++] = (float)v;
    }
    double load0 = 0.0, pv0 = 0.0;
    if (p.include_building) {
      load0 = t.load[r];
      for (int k = 0; k <= B; ++k) {
        double v = t.load[lookahead_row(p, t, r, k)];
        if (norm) v = v / p.max_building;
        o[k0++] = (float)v;
      }
    }
    if (p.include_pv) {
      pv0 = t.pv[r];
      for (int k = 0; k <= B; ++k) {
        double v = t.pv[lookahead_row(p, t, r, k)];
        if (norm) v = v / p.max_pv;
        o[k0++] = (float)v;
      }
    }
    if (!p.aux) continue;
    o[k0++] = (float)(norm ? p.evse_power / p.max_evse : p.evse_power);
    if (p.include_building) {
      const double grid_cap = p.grid_connection;
      const double avail = grid_cap - load0 + pv0;
      const double q = avail / (N * p.evse_power);
      const double pavg = q < 1 ? q : 1;
      o[k0++] = (float)(norm ? grid_cap / p.max_grid : grid_cap);
      o[k0++] = (float)(norm ? avail / p.max_grid : avail);
      o[k0++] = (float)pavg;
    }
    if (t.time_feat) {
      for (int k = 0; k < 6; ++k) o[k0++] = t.time_feat[(size_t)r * 6 + k];
    } else {
      o[k0++] = (float)std::sin(two_pi * t.month[r] / 12);
      o[k0++] = (float)std::cos(two_pi * t.month[r] / 12);
      o[k0++] = (float)std::sin(two_pi * t.weekday[r] / 7);
      o[k0++] = (float)std::cos(two_pi * t.weekday[r] / 7);
      o[k0++] = (float)std::sin(two_pi * t.hour[r] / 24);
      o[k0++] = (float)std::cos(two_pi * t.hour[r] / 24);
    }
    (void)tail_a; (void)tail_b;
  }
}

// Physics rows: only combinations the reference itself evaluates on per-time scalars, same float64 operations
// in the same order, so the stored doubles are bit-identical to what the reference computes per step.
static void build_phys_rows(const FleetParams& p, const FleetTables& t, std::vector<PhysRow>& phys, std::vector<uint8_t>& flags) {
  const int T = p.table_rows, N = p.num_cars;
  phys.resize(T);
  flags.resize(T);
  const double spot_offset = p.fixed_markup / 1000;  // ev_charger.py:34
  for (int r = 0; r < T; ++r) {
    PhysRow& q = phys[r];
    q.k_cost = (t.delu[r] / 1000.0 + spot_offset) * p.variable_multiplier;  // (current_spot + spot_offset) * spot_multiplier :145-149
    q.k_rev = -1 * p.discharging_eff * t.tariff[r] / 1000 * (1 - p.feed_in_deduction);  // :196-199 without the energy factor
    q.k_charge = -1 * p.price_multiplier * t.prc[r] / 1000;       // :154-155
    q.k_discharge = -1 * p.price_multiplier * t.trc[r] / 1000;    // :204-205
    q.load = p.include_building ? t.load[r] : 0.0;
    q.pv = p.include_pv ? t.pv[r] : 0.0;
    // connected_cars = max(sum(There[t]), 1) is a function of the time row alone (:138-140), so
    // current_pv_energy / connected_cars (:134,142) can be tabulated with the reference's own two operations
    long connected = 0;
    for (int c = 0; c < N; ++c) connected += t.there[(size_t)r * N + c];
    if (connected < 1) connected = 1;
    const double pv_energy = p.include_pv ? t.pv[r] * (t.dt_row ? t.dt_row[r] : p.dt) : 0.0;
    q.pv_share = pv_energy / (double)connected;
    q.pad = 0;
    q.dt = t.dt_row ? t.dt_row[r] : p.dt;
    uint8_t f = 0;
    if (t.hour[r] == 14 && t.minute[r] == 45) f |= FLEET_TFLAG_DEG;
    if (t.hour[r] > 11 && t.hour[r] < 15) f |= FLEET_TFLAG_LUNCH;
    flags[r] = f;
  }
  for (int r = 0; r < T; ++r) phys[r].flags_next = flags[r + 1 < T ? r + 1 : T - 1];
}

// Per-(t, EV) schedule records in run-length form (struct SegRec in fleet_device.h): consecutive rows of an EV with the same
// There, the same SOC_on_return (bit for bit) and a time_left that counts down to the same departure row form a segment and
// share one record.  Whether a row's float32 time_left is what the kernels derive from the departure row is checked here
// with the kernels' own expression (seg_tl); a row where it is not -- an irregular time grid, a hand-made table -- becomes
// a one-row segment that carries its time_left verbatim.
static void build_seg_rows(const FleetParams& p, const FleetTables& t, std::vector<SegRec>& seg) {
  const int T = p.table_rows, N = p.num_cars;
  seg.resize((size_t)T * N);
  std::vector<uint8_t> raw((size_t)T);
  std::vector<uint32_t> dep((size_t)T);
  for (int c = 0; c < N; ++c) {
    for (int r = 0; r < T; ++r) {
      const float tl = t.time_left[(size_t)r * N + c];
      raw[r] = 0;
      dep[r] = 0;  // time_left == 0: no departure ahead
      if (tl != 0.0f) {
        const double k = (double)tl / p.dt;
        const long long kk = std::llround(k);
        SegRec probe;
        probe.sor = 0.0;
        probe.tlx = (uint32_t)(r + kk);
        probe.se = 0;
        if (!t.dt_row && kk >= 1 && (long long)r + kk < 0x3FFFFFFFll && seg_tl(probe, r, p.dt) == tl)
          dep[r] = (uint32_t)(r + kk);
        else
          raw[r] = 1;
      }
    }
    uint32_t end = (uint32_t)T;
    for (int r = T - 1; r >= 0; --r) {
      const size_t k = (size_t)r * N + c;
      if (r < T - 1) {
        const size_t k1 = k + N;
        uint64_t s0, s1;
        memcpy(&s0, &t.soc_on_return[k], 8);
        memcpy(&s1, &t.soc_on_return[k1], 8);
        const bool same = !raw[r] && !raw[r + 1] && t.there[k] == t.there[k1] && s0 == s1 && dep[r] == dep[r + 1];
        if (!same) end = (uint32_t)(r + 1);
      }
      SegRec& x = seg[k];
      x.sor = t.soc_on_return[k];
      if (raw[r]) {
        memcpy(&x.tlx, &t.time_left[k], 4);
      } else {
        x.tlx = dep[r];
      }
      x.se = end | (raw[r] ? SEG_RAW : 0u) | (t.there[k] ? 0x80000000u : 0u);
    }
  }
}

int fleet_create_impl(const FleetParams* p, const FleetTables* t, int device, FleetEnvBatch* b) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    b->error = "no HIP device visible; libfleet_hip has no CPU fallback";
    return FLEET_ERR_NODEVICE;
  }
  if (device < 0 || device >= ndev) {
    b->error = "device index out of range";
    return FLEET_ERR_INVALID;
  }
  b->p = *p;
  b->device = device;
  b->table_hash = fleet_state_hash_tables(*p, *t);
  HIP_TRY(b, hipSetDevice(device));
  HIP_TRY(b, hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking));
  b->stream = b->own_stream;
  HIP_TRY(b, hipEventCreate(&b->ev_start));
  HIP_TRY(b, hipEventCreate(&b->ev_stop));

  FleetDev& d = b->d;
  const int E = p->num_envs, N = p->num_cars, T = p->table_rows, L = p->price_lookahead, B = p->bl_pv_lookahead;
  d.E = E; d.N = N; d.T = T;
  d.obs_dim = fleet_obs_dim_of(p);
  d.episode_steps = p->episode_steps;
  // rows of the rainflow stack workspace: pushes <= logged samples; on an irregular grid an episode spans as many rows as its
  // finish row says, not episode_steps
  int max_rows = p->episode_steps;
  if (t->finish_row)
    for (int r = 0; r < T; ++r)
      if (t->finish_row[r] - r > max_rows) max_rows = t->finish_row[r] - r;
  d.stack_cap = max_rows + 3;
  d.tail_a_len = 2 * (L + 1) + (p->include_building ? B + 1 : 0) + (p->include_pv ? B + 1 : 0);
  d.tail_b_len = p->aux ? (1 + (p->include_building ? 3 : 0) + 6) : 0;
  d.tail_stride = ((d.tail_a_len + d.tail_b_len + 3) / 4) * 4;
  d.aux = p->aux; d.normalize = p->normalize; d.is_caretaker = p->is_caretaker; d.deg_mode = p->deg_mode;
  d.auto_reset = p->auto_reset;
  d.real_time = p->real_time ? 1 : 0;
  d.carry_run = (N <= fleet_max_evs_per_lane_group()) ? 1 : 0;
  d.dt = p->dt; d.evse_power = p->evse_power;
  d.p_avail = p->obc_max_power < p->evse_power ? p->obc_max_power : p->evse_power;  // min([obc, evse]) ev_charger.py:95
  d.init_cap = p->init_battery_cap; d.grid_connection = p->grid_connection;
  d.eta_c = p->charging_eff; d.eta_d = p->discharging_eff;
  // stress_temp (rainflow_sei_degradation.py:72-73) is a constant of the batch
  d.stress_temp = std::exp(6.93E-2 * (p->temperature - 25.0) * ((25.0 + 273.15) / (p->temperature + 273.15)));
  d.penalty_invalid = p->penalty_invalid_action; d.penalty_oc = p->penalty_overcharging; d.clip_oc = p->clip_overcharging;
  d.penalty_overload = p->penalty_overloading; d.fully_charged_reward = p->fully_charged_reward;
  d.target_soc = p->target_soc; d.target_soc_lunch = p->target_soc_lunch; d.eps = p->eps;
  d.max_time_left = p->max_time_left;
  // auxiliary observation slots: divisions by constants become multiplications by the correctly rounded quotient / reciprocal
  d.hn_scale = p->batt_cap_nominal / (p->evse_power * p->charging_eff);
  d.inv_eta_c = 1.0 / p->charging_eff;

  FleetCold& cd = b->cold_host;
  cd.min_laxity = p->min_laxity; cd.def_soc = p->def_soc; cd.init_soh = p->init_soh; cd.temperature = p->temperature;
  cd.dt = p->dt; cd.batt_cap_nominal = p->batt_cap_nominal; cd.hn_denominator = p->evse_power * p->charging_eff;
  cd.max_soc = p->max_soc; cd.max_hours_needed = p->max_hours_needed; cd.max_laxity = p->max_laxity;
  cd.inv_max_soc = p->normalize ? 1.0 / p->max_soc : 1.0;
  cd.inv_max_hours_needed = p->normalize ? 1.0 / p->max_hours_needed : 1.0;
  cd.inv_max_laxity = p->normalize ? 1.0 / p->max_laxity : 1.0;
  cd.seed = p->seed; cd.picker_mode = p->picker_mode; cd.start_lo = p->start_lo; cd.start_hi = p->start_hi;
  cd.env_id_offset = p->env_id_offset; cd.sched_n = 0; cd.normalize = p->normalize; cd.sched = nullptr;

  // ---- tables ---------------------------------------------------------------------------------------
  int rc;
  {
    std::vector<PhysRow> phys;
    std::vector<uint8_t> flags;
    build_phys_rows(*p, *t, phys, flags);
    std::vector<float> tail;
    build_tail_rows(*p, *t, d.tail_a_len, d.tail_b_len, d.tail_stride, tail);
    std::vector<SegRec> seg;
    build_seg_rows(*p, *t, seg);
    if ((rc = dev_upload(b, &d.seg, seg.data(), seg.size()))) return rc;
    if ((rc = dev_upload(b, &d.tab_phys, phys.data(), phys.size()))) return rc;
    if ((rc = dev_upload(b, &d.tab_flags, flags.data(), flags.size()))) return rc;
    // the last degradation row at or before every row: where an episode's rainflow count may stop (EnvRec::rf_until)
    std::vector<int32_t> last_deg((size_t)T);
    int32_t last = -1;
    for (int r = 0; r < T; ++r) {
      if (flags[r] & FLEET_TFLAG_DEG) last = r;
      last_deg[r] = last;
    }
    if ((rc = dev_upload(b, &cd.tab_last_deg, last_deg.data(), last_deg.size()))) return rc;
    if ((rc = dev_upload(b, &d.tab_tail, tail.data(), tail.size()))) return rc;
    HIP_TRY(b, hipStreamSynchronize(b->stream));  // host vectors go out of scope here
  }
  {
    // night-charging policy (benchmarking/night_charging.py:81-98): clock of every table row + per-env window state
    std::vector<uint16_t> hm((size_t)T);
    for (int i = 0; i < T; ++i)
      hm[i] = (uint16_t)((t->hour[i] << 8) | t->minute[i] | ((t->second && t->second[i]) ? 0x8000 : 0));  // bit 15: off the minute
    if ((rc = dev_upload(b, &cd.tab_hm, hm.data(), hm.size()))) return rc;
    std::vector<int32_t> idle((size_t)E, FLEET_NIGHT_IDLE);
    if ((rc = dev_alloc(b, &cd.night_start, (size_t)E, false))) return rc;
    HIP_TRY(b, hipMemcpyAsync(cd.night_start, idle.data(), idle.size() * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
    cd.night_hour = -1; cd.night_minute = 0; cd.night_limit_s = 0;
    if ((rc = dev_alloc(b, &cd.last_len, (size_t)E))) return rc;  // (zeroed)
    cd.rf_count_all = 0;
    cd.step_s = (int)std::llround(p->dt * 3600.0);
    HIP_TRY(b, hipStreamSynchronize(b->stream));
  }
  if (t->pick_rows)
    if ((rc = dev_upload(b, &cd.pick_rows, t->pick_rows, (size_t)t->n_pick_rows))) return rc;
  if (t->finish_row) {  // irregular time grid (real_time): episode-end row by date (the per-row step length is in PhysRow)
    if ((rc = dev_upload(b, &d.tab_finish, t->finish_row, (size_t)T))) return rc;
    HIP_TRY(b, hipStreamSynchronize(b->stream));
  }
  if ((rc = dev_alloc(b, &b->cold_dev, 1))) return rc;
  HIP_TRY(b, hipMemcpyAsync(b->cold_dev, &cd, sizeof(FleetCold), hipMemcpyHostToDevice, b->stream));
  d.cold = b->cold_dev;

  // ---- state ----------------------------------------------------------------------------------------
  const size_t EN = (size_t)E * N;
  if ((rc = dev_alloc(b, &d.hot, EN))) return rc;
  if ((rc = dev_alloc(b, &d.run, EN))) return rc;
  if ((rc = dev_alloc(b, &d.soh, EN))) return rc;
  if ((rc = dev_alloc(b, &d.soc_deg, EN))) return rc;
  if ((rc = dev_alloc(b, &d.sei, EN))) return rc;
  if (p->log_data) {  // device-side data log: ring of log_capacity rows per env (default: two episodes incl. their reset rows)
    d.log_cap = p->log_capacity > 0 ? p->log_capacity : 2 * (p->episode_steps + 1);
    const size_t rows = (size_t)d.log_cap * E;
    if ((rc = dev_alloc(b, &d.log_pos, (size_t)E))) return rc;
    if ((rc = dev_alloc(b, &d.log_row, rows))) return rc;
    if ((rc = dev_alloc(b, &d.log_env, rows * 4))) return rc;
    if ((rc = dev_alloc(b, &d.log_ev, rows * 4 * N))) return rc;
    if ((rc = dev_alloc(b, &d.log_obs, rows * (size_t)d.obs_dim))) return rc;
  }
  if ((rc = dev_alloc(b, &d.env, E))) return rc;
  if (p->deg_mode == FLEET_DEG_RAINFLOW) {
    d.rf_row_stride = ((RF_HDR_WORDS + d.stack_cap + 15) / 16) * 16;  // RfHdr + stack, rounded to whole 128-byte lines
    // the kernels address an EV's row as (the env's rows, a scalar base) + a 32-bit byte offset
    if ((uint64_t)N * (uint64_t)d.rf_row_stride * 8ull >= (1ull << 32)) {
      b->error = "num_cars x episode length: the rainflow rows of one env exceed 4 GiB";
      return FLEET_ERR_INVALID;
    }
    if ((rc = dev_alloc(b, &d.rf_rows, EN * (size_t)d.rf_row_stride, false))) return rc;
    // headers: rainflow_length = 1 (rainflow_sei_degradation.py:57), everything else 0
    RfHdr h0;
    memset(&h0, 0, sizeof h0);
    h0.rf_len = 1;
    std::vector<RfHdr> hdrs(EN, h0);
    HIP_TRY(b, hipMemcpy2DAsync(d.rf_rows, (size_t)d.rf_row_stride * 8, hdrs.data(), sizeof(RfHdr), sizeof(RfHdr), EN,
                                hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
  }
  {
    // persistent degradation state (RainflowSeiDegradation.__init__, rainflow_sei_degradation.py:24-66), the initial
    // SoH and the (cleared) sticky target flags (fleet_environment.py:263)
    std::vector<double> soh(EN, p->init_soh);  // the hot records themselves are zero (no sticky target flag yet)
    std::vector<SeiRec> sei(EN);
    for (auto& q : sei) { q.fd_cyc = 0; q.fd_cal = 0; q.sei_soh = p->init_soh; q.sei_l = 1.0 - p->init_soh; }
    HIP_TRY(b, hipMemcpyAsync(d.soh, soh.data(), EN * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipMemcpyAsync(d.sei, sei.data(), EN * sizeof(SeiRec), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
  }
  if ((rc = dev_alloc(b, &b->self_dev, 1))) return rc;
  d.self = b->self_dev;
  // ---- staging for host entry points -------------------------------------------------------------------------------
  const size_t OD = (size_t)E * d.obs_dim;
  if ((rc = dev_alloc(b, (char**)&b->st_actions, EN * 8))) return rc;
  if ((rc = dev_alloc(b, &b->st_obs, OD))) return rc;
  if ((rc = dev_alloc(b, &b->st_term, OD))) return rc;
  b->small.set(E);
  if ((rc = dev_alloc(b, &b->st_small, b->small.bytes))) return rc;
  b->st_reward = b->small.reward(b->st_small);
  b->st_done = b->small.done(b->st_small);
  d.err_any = b->small.err_word(b->st_small);
  if ((rc = dev_alloc(b, &b->st_term_compact, OD))) return rc;
  HIP_TRY(b, hipHostMalloc((void**)&b->pin_small, b->small.bytes, hipHostMallocDefault));
  HIP_TRY(b, hipHostMalloc(&b->pin_actions, EN * 8, hipHostMallocDefault));
  HIP_TRY(b, hipHostMalloc((void**)&b->pin_term, OD * sizeof(float), hipHostMallocDefault));
  if ((rc = dev_alloc(b, &b->st_mask, E))) return rc;
  if ((rc = dev_alloc(b, &b->st_dist, EN))) return rc;
  if ((rc = dev_alloc(b, (char**)&b->st_field, (EN > 2 * (size_t)E ? EN : 2 * (size_t)E) * 8))) return rc;  // a field, or the [2, E] gather block
  // device-resident copy of the (now complete) argument block for the out-of-line rare paths (reset, daily degradation)
  HIP_TRY(b, hipMemcpyAsync(b->self_dev, &d, sizeof(FleetDev), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(b, hipStreamSynchronize(b->stream));
  return FLEET_OK;
}
