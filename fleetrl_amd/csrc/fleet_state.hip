// fleet_state.hip -- save, restore and fork env state on the device (declared in fleet_state.h; C ABI: include/fleet_hip.h
// "env state").  The blob is a FleetStateHeader followed by plain copies of the state arrays at 256-byte-aligned offsets: save and
// load are one asynchronous copy per section and need no kernel.  The fork moves chosen envs with fleet_fork_kernel.
#include "fleet_state.h"

#include <cstring>
#include <vector>

void fleet_set_create_error(const std::string& why);  // fleet_capi.hip (declared in fleet_batch.h too): what fleet_last_error(NULL) returns

namespace {

#define ST_TRY(r, expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      *(r).error = std::string(#expr) + ": " + hipGetErrorString(_e);          \
      return FLEET_ERR_HIP;                                                    \
    }                                                                          \
  } while (0)

constexpr uint64_t align_up(uint64_t x) { return (x + FLEET_STATE_ALIGN - 1) / FLEET_STATE_ALIGN * FLEET_STATE_ALIGN; }

int obs_dim_of(const FleetParams& p) {  // (fleet_obs_dim)
  return fleet_obs_dim(&p);
}

// Offsets and sizes of every section from the few numbers that fix them.
void layout_fill(int E, int N, int obs_dim, int deg_mode, int stack_cap, int log_cap, FleetStateLayout* L) {
  memset(L, 0, sizeof *L);
  L->struct_bytes = (int32_t)sizeof *L;
  L->alignment = FLEET_STATE_ALIGN;
  L->header_bytes = align_up(sizeof(FleetStateHeader));
  L->num_envs = E;
  L->num_cars = N;
  L->obs_dim = obs_dim;
  const bool rf = deg_mode == FLEET_DEG_RAINFLOW;
  L->stack_cap = rf ? stack_cap : 0;
  L->rf_row_stride = rf ? ((RF_HDR_WORDS + stack_cap + 15) / 16) * 16 : 0;
  L->log_cap = log_cap;
  const uint64_t EN = (uint64_t)E * N, rows = (uint64_t)log_cap * E;
  uint64_t bytes[FLEET_STATE_SECTIONS] = {};
  bytes[FLEET_SEC_HOT] = EN * sizeof(Hot);
  bytes[FLEET_SEC_RUN] = EN * sizeof(SegRec);
  bytes[FLEET_SEC_SOH] = EN * 8;
  bytes[FLEET_SEC_SOC_DEG] = EN * 8;
  bytes[FLEET_SEC_SEI] = EN * sizeof(SeiRec);
  bytes[FLEET_SEC_ENV] = (uint64_t)E * sizeof(EnvRec);
  bytes[FLEET_SEC_NIGHT_START] = (uint64_t)E * 4;
  bytes[FLEET_SEC_LAST_LEN] = (uint64_t)E * 4;
  bytes[FLEET_SEC_RF_ROWS] = rf ? EN * (uint64_t)L->rf_row_stride * 8 : 0;
  if (log_cap > 0) {
    bytes[FLEET_SEC_LOG_POS] = (uint64_t)E * 4;
    bytes[FLEET_SEC_LOG_ROW] = rows * 4;
    bytes[FLEET_SEC_LOG_ENV] = rows * 4 * 8;
    bytes[FLEET_SEC_LOG_EV] = rows * 4 * N * 8;
    bytes[FLEET_SEC_LOG_OBS] = rows * (uint64_t)obs_dim * 4;
  }
  uint64_t off = L->header_bytes;
  for (int s = 0; s < FLEET_STATE_SECTIONS; ++s) {
    if (!bytes[s]) continue;
    L->sec[s].offset = off;
    L->sec[s].bytes = bytes[s];
    off = align_up(off + bytes[s]);
  }
  L->total_bytes = off;
}

void layout_of(const FleetStateRefs& r, FleetStateLayout* L) {
  const FleetDev& d = *r.d;
  layout_fill(d.E, d.N, d.obs_dim, d.deg_mode, d.stack_cap, d.log_pos ? d.log_cap : 0, L);
}

// the device array of a section
void* section_ptr(const FleetStateRefs& r, int s) {
  const FleetDev& d = *r.d;
  switch (s) {
    case FLEET_SEC_HOT: return d.hot;
    case FLEET_SEC_RUN: return d.run;
    case FLEET_SEC_SOH: return d.soh;
    case FLEET_SEC_SOC_DEG: return d.soc_deg;
    case FLEET_SEC_SEI: return d.sei;
    case FLEET_SEC_ENV: return d.env;
    case FLEET_SEC_NIGHT_START: return r.cold_host->night_start;
    case FLEET_SEC_LAST_LEN: return r.cold_host->last_len;
    case FLEET_SEC_RF_ROWS: return d.rf_rows;
    case FLEET_SEC_LOG_POS: return d.log_pos;
    case FLEET_SEC_LOG_ROW: return d.log_row;
    case FLEET_SEC_LOG_ENV: return d.log_env;
    case FLEET_SEC_LOG_EV: return d.log_ev;
    case FLEET_SEC_LOG_OBS: return d.log_obs;
    case FLEET_SEC_SCHED: return *r.dev_sched;
    default: return nullptr;
  }
}

// the header of a blob of this handle as it is now
void header_of(const FleetStateRefs& r, FleetStateHeader* h) {
  FleetStateLayout L;
  layout_of(r, &L);
  memset(h, 0, sizeof *h);
  h->magic = FLEET_STATE_MAGIC;
  h->abi_version = FLEET_ABI_VERSION;
  h->header_bytes = (int32_t)sizeof *h;
  fleet_state_fingerprint(*r.p, *r.d, r.table_hash, &h->fp);
  h->num_envs = r.d->E;
  h->env_id_offset = r.cold_host->env_id_offset;
  h->obs_dim = r.d->obs_dim;
  h->night_hour = r.cold_host->night_hour;
  h->night_minute = r.cold_host->night_minute;
  h->night_limit_s = r.cold_host->night_limit_s;
  h->rf_count_all = r.cold_host->rf_count_all;
  h->sched_n = r.cold_host->sched_n;
  memcpy(h->sec, L.sec, sizeof h->sec);
  h->total_bytes = L.total_bytes;
  if (h->sched_n > 0) {
    h->sec[FLEET_SEC_SCHED].offset = L.total_bytes;
    h->sec[FLEET_SEC_SCHED].bytes = (uint64_t)h->sched_n * r.d->E * 4;
    h->total_bytes = align_up(L.total_bytes + h->sec[FLEET_SEC_SCHED].bytes);
  }
}

// magic, version, E and fingerprint of a header against what a handle (or a set of parameters) has; nullptr: fits
const char* header_mismatch(const FleetStateHeader& h, uint64_t bytes, int E, const FleetStateFingerprint& fp, bool full_fp) {
  if (bytes < sizeof(FleetStateHeader)) return "the blob is shorter than a header";
  if (h.magic != FLEET_STATE_MAGIC) return "magic: not a fleet state blob";
  if (h.abi_version != FLEET_ABI_VERSION) return "abi_version: the blob was written by another version of the library";
  if (h.header_bytes != (int32_t)sizeof(FleetStateHeader)) return "header_bytes";
  if (h.num_envs != E) return "num_envs: a state is loaded into a handle of the same number of envs";
  FleetStateFingerprint a = h.fp;
  if (!full_fp) {  // from parameters alone the tables' own episode spans (irregular grids) are not known
    a.stack_cap = fp.stack_cap;
    a.rf_row_stride = fp.rf_row_stride;
  }
  if (const char* f = fleet_state_fingerprint_diff(a, fp)) return f;
  if (h.total_bytes > bytes) return "the blob is shorter than its header says";
  return nullptr;
}

}  // namespace

uint64_t fleet_state_hash_tables(const FleetParams& p, const FleetTables& t) {
  // eight bytes at a time: multiply, fold.  Not cryptographic: it tells two data sets apart, nothing else.
  uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)p.table_rows << 32) ^ (uint64_t)p.num_cars;
  auto mix = [&h](const void* ptr, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(ptr);
    if (!b) {
      h = (h ^ 0xA5A5A5A5ull) * 0xD6E8FEB86659FD93ull;
      return;
    }
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t w;
      memcpy(&w, b + i, 8);
      h = (h ^ w) * 0xD6E8FEB86659FD93ull;
      h ^= h >> 32;
    }
    uint64_t w = 0;
    memcpy(&w, b + i, n - i);
    h = (h ^ w ^ ((uint64_t)n << 56)) * 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
  };
  // Hashed: `there` and every per-row array in full; of the two wide per-(row, EV) arrays, time_left and soc_on_return -- 21 of the
  // 25 MB at T = 35 040, N = 50, where hashing everything cost 11 % of fleet_create -- every 16th row and the last one.  Two data sets
  // that differ ONLY in time_left / soc_on_return values of rows in between, with the same plug-in pattern, hash alike.
  const size_t T = (size_t)p.table_rows, N = (size_t)p.num_cars, TN = T * N;
  mix(t.there, TN);
  for (size_t r = 0; r < T; r += (r + 16 < T || r + 1 == T) ? 16 : T - 1 - r) {
    mix(t.time_left + r * N, N * 4);
    mix(t.soc_on_return + r * N, N * 8);
  }
  for (const double* a : {t.delu, t.tariff, t.prc, t.trc, t.load, t.pv}) mix(a, T * 8);
  for (const uint8_t* a : {t.hour, t.minute, t.month, t.weekday}) mix(a, T);
  mix(t.time_feat, T * 6 * 4);
  mix(t.dt_row, T * 8);
  mix(t.finish_row, T * 4);
  mix(t.lookahead_row, t.lookahead_row ? T * (size_t)t.lookahead_cols * 4 : 0);
  mix(t.second, T);
  mix(t.pick_rows, t.pick_rows ? (size_t)t.n_pick_rows * 4 : 0);
  return h;
}

void fleet_state_fingerprint(const FleetParams& p, const FleetDev& d, uint64_t table_hash, FleetStateFingerprint* fp) {
  memset(fp, 0, sizeof *fp);
  fp->num_cars = p.num_cars;
  fp->table_rows = p.table_rows;
  fp->episode_steps = p.episode_steps;
  fp->deg_mode = p.deg_mode;
  fp->real_time = p.real_time ? 1 : 0;
  fp->price_lookahead = p.price_lookahead;
  fp->bl_pv_lookahead = p.bl_pv_lookahead;
  fp->include_building = p.include_building ? 1 : 0;
  fp->include_pv = p.include_pv ? 1 : 0;
  fp->aux = p.aux ? 1 : 0;
  fp->normalize = p.normalize ? 1 : 0;
  const bool rf = p.deg_mode == FLEET_DEG_RAINFLOW;
  fp->stack_cap = rf ? d.stack_cap : 0;
  fp->rf_row_stride = rf ? d.rf_row_stride : 0;
  fp->log_cap = d.log_cap;
  fp->picker_mode = p.picker_mode;
  fp->seed = p.seed;
  fp->dt = p.dt;
  fp->table_hash = table_hash;
}

const char* fleet_state_fingerprint_diff(const FleetStateFingerprint& a, const FleetStateFingerprint& b) {
#define FP_FIELD(f) \
  if (memcmp(&a.f, &b.f, sizeof a.f) != 0) return "fingerprint: " #f " differs"
  FP_FIELD(num_cars);
  FP_FIELD(table_rows);
  FP_FIELD(episode_steps);
  FP_FIELD(deg_mode);
  FP_FIELD(real_time);
  FP_FIELD(price_lookahead);
  FP_FIELD(bl_pv_lookahead);
  FP_FIELD(include_building);
  FP_FIELD(include_pv);
  FP_FIELD(aux);
  FP_FIELD(normalize);
  FP_FIELD(stack_cap);
  FP_FIELD(rf_row_stride);
  FP_FIELD(log_cap);
  FP_FIELD(picker_mode);
  FP_FIELD(seed);
  FP_FIELD(dt);
  FP_FIELD(table_hash);
#undef FP_FIELD
  return nullptr;
}

uint64_t fleet_state_blob_bytes(const FleetStateRefs& r) {
  FleetStateHeader h;
  header_of(r, &h);
  return h.total_bytes;
}

int fleet_state_save(const FleetStateRefs& r, void* blob, uint64_t bytes, bool host) {
  FleetStateHeader hdr;
  header_of(r, &hdr);
  if (!blob || bytes < hdr.total_bytes) {
    *r.error = "fleet_state_save: the buffer holds " + std::to_string(bytes) + " bytes, the state needs " +
               std::to_string(hdr.total_bytes) + " (fleet_state_bytes)";
    return FLEET_ERR_INVALID;
  }
  if (!host && (reinterpret_cast<uintptr_t>(blob) % 16) != 0) {
    *r.error = "fleet_state_save_dev: the blob must be 16-byte aligned";
    return FLEET_ERR_INVALID;
  }
  char* out = static_cast<char*>(blob);
  // the bytes between two sections are zero, so that two saves of one state are the same bytes
  auto zero = [&](uint64_t lo, uint64_t hi) -> hipError_t {
    if (hi <= lo) return hipSuccess;
    if (host) {
      memset(out + lo, 0, hi - lo);
      return hipSuccess;
    }
    return hipMemsetAsync(out + lo, 0, hi - lo, r.stream);
  };
  if (host) {
    memcpy(out, &hdr, sizeof hdr);
  } else {
    *r.pin_hdr = hdr;  // (the caller has drained the stream: the last save's copy out of this buffer is done)
    ST_TRY(r, hipMemcpyAsync(out, r.pin_hdr, sizeof hdr, hipMemcpyHostToDevice, r.stream));
  }
  uint64_t end = sizeof hdr;
  for (int s = 0; s < FLEET_STATE_SECTIONS; ++s) {
    if (!hdr.sec[s].bytes) continue;
    ST_TRY(r, zero(end, hdr.sec[s].offset));
    ST_TRY(r, hipMemcpyAsync(out + hdr.sec[s].offset, section_ptr(r, s), hdr.sec[s].bytes,
                             host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, r.stream));
    end = hdr.sec[s].offset + hdr.sec[s].bytes;
  }
  ST_TRY(r, zero(end, hdr.total_bytes));
  if (host) ST_TRY(r, hipStreamSynchronize(r.stream));
  return FLEET_OK;
}

int fleet_state_load(const FleetStateRefs& r, const void* blob, uint64_t bytes, bool host) {
  if (!blob || bytes < sizeof(FleetStateHeader)) {
    *r.error = "fleet_state_load: the blob is shorter than a header";
    return FLEET_ERR_INVALID;
  }
  const char* in = static_cast<const char*>(blob);
  FleetStateHeader hdr;
  if (host) {
    memcpy(&hdr, in, sizeof hdr);
  } else {
    ST_TRY(r, hipMemcpyAsync(&hdr, in, sizeof hdr, hipMemcpyDeviceToHost, r.stream));
    ST_TRY(r, hipStreamSynchronize(r.stream));
  }
  // ---- everything is checked before the handle's state is touched ----
  FleetStateFingerprint fp;
  fleet_state_fingerprint(*r.p, *r.d, r.table_hash, &fp);
  if (const char* why = header_mismatch(hdr, bytes, r.d->E, fp, true)) {
    *r.error = std::string("fleet_state_load: ") + why;
    return FLEET_ERR_INVALID;
  }
  FleetStateLayout L;
  layout_of(r, &L);
  for (int s = 0; s < FLEET_STATE_SECTIONS; ++s)
    if (s != FLEET_SEC_SCHED && (hdr.sec[s].offset != L.sec[s].offset || hdr.sec[s].bytes != L.sec[s].bytes)) {
      *r.error = "fleet_state_load: section " + std::to_string(s) + " of the blob is not where this handle's layout has it";
      return FLEET_ERR_INVALID;
    }
  const FleetStateSection sc = hdr.sec[FLEET_SEC_SCHED];
  const uint64_t sched_bytes = hdr.sched_n > 0 ? (uint64_t)hdr.sched_n * r.d->E * 4 : 0;
  if (hdr.sched_n < 0 || sc.bytes != sched_bytes || (sched_bytes && (sc.offset != L.total_bytes || sc.offset + sc.bytes > bytes))) {
    *r.error = "fleet_state_load: the start-schedule section does not match sched_n";
    return FLEET_ERR_INVALID;
  }
  if (hdr.night_hour > 24 || hdr.night_minute < 0 || hdr.night_minute > 59 || hdr.night_limit_s < 0) {
    *r.error = "fleet_state_load: night-policy parameters out of range";
    return FLEET_ERR_INVALID;
  }
  std::vector<int32_t> sched(sched_bytes / 4);
  if (sched_bytes) {  // start rows index the tables: checked like fleet_set_start_schedule checks them
    if (host) {
      memcpy(sched.data(), in + sc.offset, sched_bytes);
    } else {
      ST_TRY(r, hipMemcpyAsync(sched.data(), in + sc.offset, sched_bytes, hipMemcpyDeviceToHost, r.stream));
      ST_TRY(r, hipStreamSynchronize(r.stream));
    }
    for (int32_t row : sched)
      if (row < 0 || row > r.d->T - 1) {
        *r.error = "fleet_state_load: a start row of the blob's schedule lies outside the table";
        return FLEET_ERR_INVALID;
      }
  }
  // ---- restore ----
  ST_TRY(r, hipStreamSynchronize(r.stream));  // (the old schedule may still be read by a reset in flight)
  if (*r.dev_sched) {
    (void)hipFree(*r.dev_sched);
    *r.dev_sched = nullptr;
  }
  r.cold_host->sched = nullptr;
  r.cold_host->sched_n = 0;
  if (sched_bytes) {
    ST_TRY(r, hipMalloc((void**)r.dev_sched, sched_bytes));
    ST_TRY(r, hipMemcpy(*r.dev_sched, sched.data(), sched_bytes, hipMemcpyHostToDevice));
    r.cold_host->sched = *r.dev_sched;
    r.cold_host->sched_n = hdr.sched_n;
  }
  r.cold_host->night_hour = hdr.night_hour;
  r.cold_host->night_minute = hdr.night_minute;
  r.cold_host->night_limit_s = hdr.night_limit_s;
  r.cold_host->rf_count_all = hdr.rf_count_all ? 1 : 0;
  ST_TRY(r, hipMemcpy(r.cold_dev, r.cold_host, sizeof(FleetCold), hipMemcpyHostToDevice));
  for (int s = 0; s < FLEET_STATE_SECTIONS; ++s) {
    if (s == FLEET_SEC_SCHED || !hdr.sec[s].bytes) continue;
    ST_TRY(r, hipMemcpyAsync(section_ptr(r, s), in + hdr.sec[s].offset, hdr.sec[s].bytes,
                             host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, r.stream));
  }
  // a saved state has no device error bits (save refuses otherwise): the handle's own word follows its env records
  ST_TRY(r, hipMemsetAsync(r.d->err_any, 0, sizeof(uint32_t), r.stream));
  ST_TRY(r, hipStreamSynchronize(r.stream));
  return FLEET_OK;
}

// ---- fork -----------------------------------------------------------------------------------------------------------------
namespace {

struct ForkSide {
  Hot* hot;
  SegRec* run;
  double* soh;
  double* soc_deg;
  SeiRec* sei;
  EnvRec* env;
  int32_t* night_start;
  int32_t* last_len;
  double* rf_rows;
};
struct ForkArgs {
  ForkSide dst, src;
  const int2* pairs;  // x: destination env, y: source env
  int n, N;
  int g_shift;        // lanes per group = 1 << g_shift
  int chunks;         // groups per pair: ceil(N / G)
  int rf_row_stride;  // doubles, 0 without rainflow rows
};

// One lane group of G lanes per (pair, range of G EVs), like the step kernel's G mapping: lane l of the group holds EV c0 + l, so the
// dense records of an env are read and written by adjacent lanes (whole cache lines).  Per lane: Hot, SegRec and the two halves of
// SeiRec as 16-byte loads / stores, soh and soc_deg as 8-byte ones (a row of an odd N starts on an 8-byte boundary only, and source
// and destination rows need not share their parity), and the LIVE part of the EV's rainflow row: the 48-byte header and the
// HOT_TAIL(bits) - 1 stack words below the top entry (the top is RfHdr::s2) of the SOURCE, in 16-byte pieces -- the row is 128-byte
// aligned and its stack starts 48 bytes in.  Words of the destination row beyond that keep their old contents: nothing reads above
// the stack size the hot record carries.  The group's first lane of the pair's first range copies the 64-byte EnvRec, night_start and
// last_len.  Plain stores: the next step of the destination reads all of it.  No atomics, no LDS, no barrier.
__global__ __launch_bounds__(256) void fleet_fork_kernel(const ForkArgs a) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;
  const unsigned group = gid >> a.g_shift, lane = gid & ((1u << a.g_shift) - 1u);
  const unsigned pair = group / (unsigned)a.chunks;
  if (pair >= (unsigned)a.n) return;
  const int c = (int)((group - pair * (unsigned)a.chunks) << a.g_shift) + (int)lane;
  const int2 pr = a.pairs[pair];
  if (c == 0) {
    const uint4* se = reinterpret_cast<const uint4*>(a.src.env + pr.y);
    uint4* de = reinterpret_cast<uint4*>(a.dst.env + pr.x);
    const uint4 e0 = se[0], e1 = se[1], e2 = se[2], e3 = se[3];
    const int32_t ns = a.src.night_start[pr.y], ll = a.src.last_len[pr.y];
    de[0] = e0; de[1] = e1; de[2] = e2; de[3] = e3;
    a.dst.night_start[pr.x] = ns;
    a.dst.last_len[pr.x] = ll;
  }
  if (c >= a.N) return;
  const size_t s = (size_t)pr.y * a.N + c, d = (size_t)pr.x * a.N + c;
  const uint4 hot = reinterpret_cast<const uint4*>(a.src.hot)[s];
  const uint4 run = reinterpret_cast<const uint4*>(a.src.run)[s];
  const uint4 sei0 = reinterpret_cast<const uint4*>(a.src.sei)[2 * s], sei1 = reinterpret_cast<const uint4*>(a.src.sei)[2 * s + 1];
  const double soh = a.src.soh[s], soc_deg = a.src.soc_deg[s];
  reinterpret_cast<uint4*>(a.dst.hot)[d] = hot;
  reinterpret_cast<uint4*>(a.dst.run)[d] = run;
  reinterpret_cast<uint4*>(a.dst.sei)[2 * d] = sei0;
  reinterpret_cast<uint4*>(a.dst.sei)[2 * d + 1] = sei1;
  a.dst.soh[d] = soh;
  a.dst.soc_deg[d] = soc_deg;
  if (a.rf_row_stride) {
    const uint4* sr = reinterpret_cast<const uint4*>(a.src.rf_rows + s * (size_t)a.rf_row_stride);
    uint4* dr = reinterpret_cast<uint4*>(a.dst.rf_rows + d * (size_t)a.rf_row_stride);
    int words = HOT_TAIL(hot.w) - 1;  // Hot::bits is the record's fourth word
    const int room = a.rf_row_stride - RF_HDR_WORDS;  // (even: a 16-byte piece never leaves the row)
    words = words < 0 ? 0 : (words > room ? room : words);
    const int pieces = RF_HDR_WORDS / 2 + (words + 1) / 2;
    for (int k = 0; k < pieces; ++k) dr[k] = sr[k];
  }
}

ForkSide side_of(const FleetStateRefs& r) {
  const FleetDev& d = *r.d;
  return ForkSide{d.hot, d.run, d.soh, d.soc_deg, d.sei, d.env, r.cold_host->night_start, r.cold_host->last_len, d.rf_rows};
}

}  // namespace

void fleet_state_fork_release(FleetForkScratch* k) {
  if (k->idx_dev) (void)hipFree(k->idx_dev);
  if (k->idx_pin) (void)hipHostFree(k->idx_pin);
  if (k->ev) (void)hipEventDestroy(k->ev);
  *k = FleetForkScratch{};
}

int fleet_state_fork(const FleetStateRefs& dst, const FleetStateRefs& src, bool same_handle, const int32_t* dst_idx,
                     const int32_t* src_idx, int n, FleetForkScratch* k) {
  std::string& err = *dst.error;
  if (n < 0 || (n > 0 && (!dst_idx || !src_idx))) {
    err = "fleet_fork_envs: null index array or negative count";
    return FLEET_ERR_INVALID;
  }
  FleetStateFingerprint fd, fs;
  fleet_state_fingerprint(*dst.p, *dst.d, dst.table_hash, &fd);
  fleet_state_fingerprint(*src.p, *src.d, src.table_hash, &fs);
  if (const char* why = fleet_state_fingerprint_diff(fs, fd)) {
    err = std::string("fleet_fork_envs: the two handles do not hold the same kind of state: ") + why;
    return FLEET_ERR_INVALID;
  }
  const int Ed = dst.d->E, Es = src.d->E;
  std::vector<uint8_t> is_dst((size_t)Ed, 0);
  for (int i = 0; i < n; ++i) {
    if (dst_idx[i] < 0 || dst_idx[i] >= Ed || src_idx[i] < 0 || src_idx[i] >= Es) {
      err = "fleet_fork_envs: pair " + std::to_string(i) + ": env index out of range";
      return FLEET_ERR_INVALID;
    }
    if (is_dst[dst_idx[i]]) {
      err = "fleet_fork_envs: env " + std::to_string(dst_idx[i]) + " appears twice among the destinations";
      return FLEET_ERR_INVALID;
    }
    is_dst[dst_idx[i]] = 1;
  }
  if (same_handle)
    for (int i = 0; i < n; ++i)
      if (is_dst[src_idx[i]]) {
        err = "fleet_fork_envs: env " + std::to_string(src_idx[i]) + " is both a source and a destination of a fork within one handle";
        return FLEET_ERR_INVALID;
      }
  if (n == 0) return FLEET_OK;
  const int N = dst.d->N;
  int g_shift = 0;
  while ((1 << g_shift) < N && g_shift < 6) ++g_shift;
  const int chunks = (N + (1 << g_shift) - 1) >> g_shift;
  const uint64_t threads = ((uint64_t)n * chunks) << g_shift;
  const uint64_t blocks = (threads + 255) / 256;
  if (blocks > 0x7FFFFFFFull) {
    err = "fleet_fork_envs: too many pairs for one launch";
    return FLEET_ERR_INVALID;
  }
  if ((size_t)n > k->cap) {
    if (k->idx_dev) ST_TRY(dst, hipFree(k->idx_dev));
    if (k->idx_pin) ST_TRY(dst, hipHostFree(k->idx_pin));
    k->idx_dev = k->idx_pin = nullptr;
    k->cap = 0;
    ST_TRY(dst, hipMalloc((void**)&k->idx_dev, (size_t)n * sizeof(int2)));
    ST_TRY(dst, hipHostMalloc((void**)&k->idx_pin, (size_t)n * sizeof(int2), hipHostMallocDefault));
    k->cap = (size_t)n;
  }
  for (int i = 0; i < n; ++i) k->idx_pin[i] = make_int2(dst_idx[i], src_idx[i]);
  // what src's stream holds (its last step) is finished before the kernel reads src, and src's next step waits for the kernel
  const bool two_streams = src.stream != dst.stream;
  if (two_streams) {
    if (!k->ev) ST_TRY(dst, hipEventCreateWithFlags(&k->ev, hipEventDisableTiming));
    ST_TRY(dst, hipEventRecord(k->ev, src.stream));
    ST_TRY(dst, hipStreamWaitEvent(dst.stream, k->ev, 0));
  }
  // one small upload: the pairs, out of pinned memory, so nothing is waited for
  hipError_t e = hipMemcpyAsync(k->idx_dev, k->idx_pin, (size_t)n * sizeof(int2), hipMemcpyHostToDevice, dst.stream);
  if (e == hipSuccess) {
    ForkArgs a{};
    a.dst = side_of(dst);
    a.src = side_of(src);
    a.pairs = k->idx_dev;
    a.n = n;
    a.N = N;
    a.g_shift = g_shift;
    a.chunks = chunks;
    a.rf_row_stride = dst.d->deg_mode == FLEET_DEG_RAINFLOW ? dst.d->rf_row_stride : 0;
    hipLaunchKernelGGL(fleet_fork_kernel, dim3((unsigned)blocks), dim3(256), 0, dst.stream, a);
    e = hipGetLastError();
  }
  if (two_streams) {  // (a wait takes the event as it was recorded when the wait was issued: one event serves both directions)
    if (e == hipSuccess) e = hipEventRecord(k->ev, dst.stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(src.stream, k->ev, 0);
  }
  ST_TRY(dst, e);
  return FLEET_OK;
}

extern "C" {

int fleet_state_layout(const FleetParams* p, FleetStateLayout* out) {
  if (!p || !out || p->num_envs < 1 || p->num_cars < 1 || p->episode_steps < 1 || p->log_capacity < 0 ||
      p->deg_mode < FLEET_DEG_NONE || p->deg_mode > FLEET_DEG_RAINFLOW) {
    fleet_set_create_error("fleet_state_layout: null pointer or parameters out of range");
    return FLEET_ERR_INVALID;
  }
  const int log_cap = p->log_data ? (p->log_capacity > 0 ? p->log_capacity : 2 * (p->episode_steps + 1)) : 0;
  layout_fill(p->num_envs, p->num_cars, obs_dim_of(*p), p->deg_mode, p->episode_steps + 3, log_cap, out);
  return FLEET_OK;
}

int fleet_state_table_hash(const FleetParams* p, const FleetTables* t, uint64_t* hash) {
  if (!p || !t || !hash || p->table_rows < 1 || p->num_cars < 1 || !t->there || !t->time_left || !t->soc_on_return || !t->delu ||
      !t->tariff || !t->prc || !t->trc || !t->load || !t->pv || !t->hour || !t->minute || !t->month || !t->weekday) {
    fleet_set_create_error("fleet_state_table_hash: null pointer");
    return FLEET_ERR_INVALID;
  }
  *hash = fleet_state_hash_tables(*p, *t);
  return FLEET_OK;
}

int fleet_state_check(const FleetParams* p, uint64_t table_hash, const void* blob_header_host, uint64_t bytes) {
  if (!p || !blob_header_host) {
    fleet_set_create_error("fleet_state_check: null pointer");
    return FLEET_ERR_INVALID;
  }
  if (bytes < sizeof(FleetStateHeader)) {
    fleet_set_create_error("fleet_state_check: the blob is shorter than a header");
    return FLEET_ERR_INVALID;
  }
  FleetStateHeader hdr;
  memcpy(&hdr, blob_header_host, sizeof hdr);
  FleetStateLayout L;
  if (fleet_state_layout(p, &L) != FLEET_OK) return FLEET_ERR_INVALID;
  FleetDev d{};
  d.stack_cap = L.stack_cap;
  d.rf_row_stride = L.rf_row_stride;
  d.log_cap = L.log_cap;
  FleetStateFingerprint fp;
  fleet_state_fingerprint(*p, d, table_hash, &fp);
  if (const char* why = header_mismatch(hdr, bytes, p->num_envs, fp, false)) {
    fleet_set_create_error(std::string("fleet_state_check: ") + why);
    return FLEET_ERR_INVALID;
  }
  return FLEET_OK;
}

}  // extern "C"
