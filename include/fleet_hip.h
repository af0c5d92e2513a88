/*
 * fleet_hip.h -- C ABI of the MI355X-native batched FleetRL step ("libfleet_hip.so").
 *
 * Drop-in boundary.  The reference has no native code; what this ABI replaces is the
 * Python object protocol of `fleetrl.fleet_env.fleet_environment.FleetEnv`
 *   __init__  /root/reference/fleetrl/fleet_env/fleet_environment.py:76-328
 *   reset     :330-434
 *   step      :436-702
 *   getters   :741-799
 * batched over `num_envs` independent environments (what SB3's SubprocVecEnv does with one OS process per
 * env).  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - every entry point returns an int status (FLEET_OK = 0); nothing throws, nothing aborts;
 *     `fleet_last_error(h)` returns a human-readable message for the last non-zero status.
 *   - plain pointers and sizes only; buffers are caller-owned.  `*_host` entry points take host
 *     pointers and are synchronous; `*_dev` entry points take device pointers (e.g. torch-ROCm tensor
 *     data_ptr()) and are asynchronous on the handle's HIP stream.
 *   - one handle = one device + one stream; calls on one handle must be serialised by the caller.
 *   - layouts are row-major:  actions [E,N], obs [E,obs_dim] f32, reward [E] f64, done [E] u8.
 */
#ifndef FLEET_HIP_H
#define FLEET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLEET_ABI_VERSION 11
/* marks an exported entry (the entries added with PPO's early stopping are declared with it) */
#define FLEET_API __attribute__((visibility("default")))

/* status codes */
#define FLEET_OK 0
#define FLEET_ERR_INVALID 1   /* bad argument / unsupported configuration (SURVEY.md Q4 matrix)            */
#define FLEET_ERR_HIP 2       /* a HIP runtime call failed                                               */
#define FLEET_ERR_STATE 3     /* device-side error word set (impossible state, rainflow stack overflow)  */
#define FLEET_ERR_NODEVICE 4  /* no HIP device: this library has no CPU fallback by design              */
#define FLEET_ERR_UNSUPPORTED 5 /* the platform does not offer what the requested launch mode relies on (FLEET_LAUNCH_DIRECT:
                                 no HSA agent at the HIP device's PCI address, a workgroup -> die placement that is not stable);
                                 use another mode                                                         */

/* FleetParams.deg_mode -- which battery-degradation model runs on the daily 14:45 step                   */
#define FLEET_DEG_NONE 0      /* calculate_degradation = False                                           */
#define FLEET_DEG_LINEAR 1    /* EmpiricalDegradation  (utils/battery_degradation/empirical_degradation.py:29-99), quirk Q1 */
#define FLEET_DEG_RAINFLOW 2  /* RainflowSeiDegradation (rainflow_sei_degradation.py:91-212)            */

/* FleetParams.picker_mode -- episode start row (utils/time_picker/)                                      */
#define FLEET_PICK_STATIC 0   /* always start_lo                                                         */
#define FLEET_PICK_RANDOM 1   /* uniform integer in [start_lo, start_hi], counter-based Philox4x32-10   */
#define FLEET_PICK_EVAL 2     /* same sampler, caller passes the validation range                       */

/* action element type */
#define FLEET_ACT_F32 0
#define FLEET_ACT_F64 1
/* built-in open-loop policies (fleet_rollout_policy_dev): the action rules of the reference's benchmark harnesses */
#define FLEET_ACT_POLICY_UNCONTROLLED 2 /* all ones           (benchmarking/uncontrolled_charging.py:51-54) */
#define FLEET_ACT_POLICY_DISTRIBUTED 3  /* clip(get_dist_factor(), 0, 1) (benchmarking/distributed_charging.py:50-54) */
#define FLEET_ACT_POLICY_NIGHT 4        /* time-window rule, stateful per env (benchmarking/night_charging.py:81-98);
                                           configure with fleet_set_night_policy first */

/* device-side error bits (per env, OR-ed into one word; see fleet_get(FLEET_F_ERROR_BITS))               */
#define FLEET_DEVERR_OBS_FORMAT 1u     /* the reference's `raise TypeError("Observation format not recognized")` :610 */
#define FLEET_DEVERR_NEG_LIFE 2u       /* "Life degradation is negative" rainflow_sei_degradation.py:179-180         */
#define FLEET_DEVERR_SOH_MISMATCH 4u   /* "Degradation calculation is not correct" :209-210                         */
#define FLEET_DEVERR_DOD_RANGE 8u      /* "DoD too large" :164-167                                                   */
#define FLEET_DEVERR_TABLE_END 16u     /* episode ran past the last table row                                        */
#define FLEET_DEVERR_INTERNAL 32u      /* a kernel found its launch arguments inconsistent (a build problem, not a data one) */
#define FLEET_DEVERR_PLACEMENT 64u     /* a launch of a run on the library's own queue (FLEET_LAUNCH_DIRECT ...) found one of its
                                          workgroups on another die than the library's probe of that queue says: the run's state
                                          may be stale, its results are void (a platform problem, not a data one)                */

/*
 * Scalars of one env group (all envs of a handle share tables and parameters).
 * Field meaning follows the reference's config classes; see fleetrl_amd/config.py for how each is
 * derived from the reference's config dict.
 */
typedef struct FleetParams {
  int32_t abi_version;      /* FLEET_ABI_VERSION */
  int32_t struct_bytes;     /* sizeof(FleetParams) as seen by the caller */
  int32_t num_envs;         /* E */
  int32_t num_cars;         /* N  (db["ID"].max()+1, fleet_environment.py:260) */
  int32_t table_rows;       /* T */
  int32_t episode_steps;    /* episode_length[h] * steps_per_hour; finish = start + episode_steps (:355).  Rainflow mode:
                               < 2^26 - 3, and num_cars * (episode_steps + 24) * 8 bytes < 4 GiB */
  int32_t price_lookahead;  /* L  (time_config.py:14) */
  int32_t bl_pv_lookahead;  /* B  (time_config.py:15) */
  int32_t steps_per_hour;   /* 60 / minutes */
  int32_t hour_phase;       /* table row 0 lies `hour_phase` steps after a full clock hour (0 for shipped data) */
  int32_t include_building; /* flags, fleet_environment.py:139-145 */
  int32_t include_pv;
  int32_t aux;
  int32_t normalize;        /* normalize_in_env -> OracleNormalization, else UnitNormalization */
  int32_t is_caretaker;     /* CompanyType.Caretaker: lunch-break target SOC (:536-554) */
  int32_t deg_mode;         /* FLEET_DEG_* */
  int32_t picker_mode;      /* FLEET_PICK_* */
  int32_t start_lo;         /* inclusive */
  int32_t start_hi;         /* inclusive */
  int32_t auto_reset;       /* 1: VecEnv semantics (done envs are reset inside the step, terminal obs reported)
                               0: gymnasium.Env semantics (obs of a done env is its terminal obs).  An env may be
                               stepped past its finish row until reset: done stays 1 (episode.done is sticky,
                               fleet_environment.py:627-628, :702), the SOC log keeps growing and its 14:45 rows
                               evaluate the degradation model, the data log writes nothing (:679).  The rainflow
                               stack workspace holds episode_steps + 3 entries: a run past done whose stack outgrows
                               it sets FLEET_DEVERR_TABLE_END in that step instead of returning a wrong result */
  int32_t env_id_offset;    /* global index of env 0 of this handle (multi-GPU sharding keeps RNG streams env-stable) */
  int32_t log_data;         /* 1: device-side data log -- every row the reference's DataLogger would get
                               (utils/data_logger/data_logger.py:21-68; call sites fleet_environment.py:420-432, 659-690) is
                               written to a per-env ring by the kernels, in every mode (single step, K steps per launch,
                               policy rollouts, resets); read with fleet_log_read.  0: nothing is logged */
  int32_t real_time;        /* 1: event-skipping step (fleet_environment.py:453,692-699, event_manager.py:16-31): the same
                               action is applied row after row until a relevant event (departure, arrival, penalty,
                               overload, episode end, clock minute 15); irregular time grids need FleetTables.dt_row etc. */
  int32_t log_capacity;     /* rows per env of the data-log ring; 0 = 2 * (episode_steps + 1).  Older rows are overwritten */
  uint64_t seed;            /* Philox key for the random/eval picker */

  double dt;                /* hours per step (time_config.py:24) */
  double evse_power;        /* load_calculation.evse_max_power */
  double obc_max_power;     /* ev_config.obc_max_power; possible_power = min(obc, evse) (ev_charger.py:95) */
  double batt_cap_nominal;  /* load_calculation.batt_cap, used by the aux observations only (observer_*.py:88) */
  double init_battery_cap;  /* ev_config.init_battery_cap */
  double grid_connection;   /* load_calculation.grid_connection */
  double charging_eff;
  double discharging_eff;
  double fixed_markup;      /* EUR/MWh (obs) ; spot_offset = fixed_markup/1000 (ev_charger.py:34) */
  double variable_multiplier;
  double feed_in_deduction;
  double price_multiplier;  /* already scaled by max_batt_cap/init_cap (:194-195) and zeroed by ignore_price_reward */
  double penalty_invalid_action;
  double penalty_overcharging;
  double clip_overcharging;
  double penalty_overloading;
  double fully_charged_reward;
  double target_soc;
  double target_soc_lunch;
  double eps;               /* 0.005 (:230) */
  double def_soc;
  double min_laxity;
  double init_soh;
  double temperature;
  /* OracleNormalization.__init__ constants (oracle_normalization.py:34-54); ignored unless `normalize` */
  double max_time_left;
  double max_price, min_price;
  double max_tariff, min_tariff;
  double max_building;
  double max_pv;
  double max_soc;
  double max_hours_needed;
  double max_laxity;
  double max_evse;
  double max_grid;
} FleetParams;

/* Pre-staged tables (HOST pointers; fleet_create uploads / re-packs them).  Row t, EV c -> [t*N + c].     */
typedef struct FleetTables {
  const uint8_t* there;         /* [T,N]  db["There"]                          */
  const float* time_left;       /* [T,N]  db["time_left"], multiples of dt     */
  const double* soc_on_return;  /* [T,N]  db["SOC_on_return"]                  */
  const double* delu;           /* [T]    EUR/MWh                              */
  const double* tariff;         /* [T]                                         */
  const double* prc;            /* [T]    price_reward_curve                   */
  const double* trc;            /* [T]    tariff_reward_curve                  */
  const double* load;           /* [T]    kW (zeros if !include_building)      */
  const double* pv;             /* [T]    kW (zeros if !include_pv)            */
  const uint8_t* hour;          /* [T]                                         */
  const uint8_t* minute;        /* [T]                                         */
  const uint8_t* month;         /* [T]  1..12                                  */
  const uint8_t* weekday;       /* [T]  Monday = 0                             */
  const float* time_feat;       /* [T,6] month/week/hour sin,cos as float32, or NULL (library computes with libm) */
  /* Irregular time grids (real_time only; all NULL / 0 for a regular grid, where the library derives them from
   * FleetParams.dt / steps_per_hour / hour_phase).  The reference reads the step length off the data
   * (`get_next_dt`, fleet_environment.py:994-1022), ends the episode on the row whose date equals start + episode_length
   * (:355, :627) and takes the hourly look-ahead values from the first row of each clock hour
   * (`resample("H").first()`, observer_bl_pv.py:53-79). */
  const double* dt_row;         /* [T]  hours from row t to row t+1 (last row: any positive value)                   */
  const int32_t* finish_row;    /* [T]  row whose date is date[t] + episode_length hours, or -1 (the episode never ends) */
  const int32_t* lookahead_row; /* [T,lookahead_cols]  column k-1: first row of clock hour floor_hour(date[t]) + k, k >= 1;
                                   -1: no such row                                                                     */
  int32_t lookahead_cols;       /* >= max(price_lookahead, bl_pv_lookahead)                                           */
  int32_t reserved0;
  const uint8_t* second;        /* [T]  seconds of the row's clock time (the clock-minute-15 event needs second == 0) */
  /* Candidate start rows of the random / eval time pickers, or NULL (= every row of [start_lo, start_hi]).  The
   * reference draws from a `date_range` at the model frequency (random_time_picker.py:25-28), which on an irregular
   * grid is a subset of the rows; with this list FleetParams.start_lo / start_hi index INTO it. */
  const int32_t* pick_rows;     /* [n_pick_rows] ascending row numbers */
  int32_t n_pick_rows;
  int32_t reserved1;
} FleetTables;

typedef struct FleetEnvBatch* fleet_handle;

/* fields for fleet_get (all copied to a HOST buffer) */
#define FLEET_F_SOC 0            /* f64 [E,N] */
#define FLEET_F_HOURS_LEFT 1     /* f32 [E,N] */
#define FLEET_F_SOH 2            /* f64 [E,N] */
#define FLEET_F_SOC_DEG 3        /* f64 [E,N] */
#define FLEET_F_TARGET_SOC 4     /* f64 [E,N] */
#define FLEET_F_TIME_IDX 5       /* i32 [E]   */
#define FLEET_F_START_IDX 6      /* i32 [E]   */
#define FLEET_F_CASHFLOW 7       /* f64 [E]   last step's cashflow (episode.current_charging_expense) */
#define FLEET_F_EP_RETURN 8      /* f64 [E]   running episode return (episode.cumulative_reward)      */
#define FLEET_F_EP_LEN 9         /* i32 [E]   */
#define FLEET_F_LAST_EP_RETURN 10 /* f64 [E]  return of the last finished episode */
#define FLEET_F_LAST_EP_LEN 11   /* i32 [E]   */
#define FLEET_F_RF_LEN 12        /* i32 [E,N] sei_deg.rainflow_length */
#define FLEET_F_FD_CYC 13        /* f64 [E,N] */
#define FLEET_F_FD_CAL 14        /* f64 [E,N] */
#define FLEET_F_SEI_L 15         /* f64 [E,N] */
#define FLEET_F_ERROR_BITS 16    /* u32 [E]   */
#define FLEET_F_DONE 17          /* u8  [E]   episode.done */
#define FLEET_F_EPISODES 18      /* i32 [E]   finished-episode counter */
#define FLEET_F_PENALTY_RECORD 19 /* f64 [E]  episode.penalty_record */
#define FLEET_F_LAST_EP_LEN_F64 20 /* f64 [E] length of the last finished episode as float64 (fleet_get_dev / the RCCL gather) */
#define FLEET_F_RF_CYCLES 21     /* i32 [E,N] rainflow cycles closed so far in the running episode (0 without rainflow degradation) */
#define FLEET_F_RF_STACK 22      /* i32 [E,N] reversal points on the EV's rainflow stack (bench.py derives the share of EV-steps that
                                    push a reversal point / close a cycle from the two: the workload's invariants)               */
#define FLEET_F_RF_UNTIL 23      /* i32 [E]   the last table row of the running episode on which the degradation model is evaluated
                                    (-1: none; INT32_MAX after fleet_set_rainflow_count_all or with auto_reset = 0): SOC samples logged after it are not
                                    counted, see fleet_set_rainflow_count_all                                                   */

/* ---- lifetime ------------------------------------------------------------------------------------- */
int fleet_obs_dim(const FleetParams* p);  /* detect_dim_and_bounds, fleet_environment.py:854-949; <0 on invalid flags */
int fleet_create(const FleetParams* p, const FleetTables* t, int device, fleet_handle* out);
int fleet_destroy(fleet_handle h);
const char* fleet_last_error(fleet_handle h);  /* h may be NULL: error of the last failed fleet_create */
/* Launch on an external hipStream_t from now on (e.g. torch's current stream, so that launches are ordered with the torch ops
 * around them).  The stream is borrowed: the caller keeps it alive while the handle uses it.  The handle's own stream is
 * kept; fleet_use_own_stream goes back to it.  Both synchronise the stream in use so far and drop a cached tape graph. */
int fleet_set_stream(fleet_handle h, void* hip_stream);
int fleet_use_own_stream(fleet_handle h);
int fleet_get_stream(fleet_handle h, void** hip_stream); /* the hipStream_t the handle launches on (to order another stream
                                                            against it with events) */
int fleet_synchronize(fleet_handle h);
/* non-blocking: FLEET_OK when everything enqueued on the handle's stream has finished, -1 while it has not (hipStreamQuery) */
int fleet_stream_query(fleet_handle h);

/* Inject episode start rows (parity tests / `set_start_time`): `starts` is HOST [n_episodes,E]; episode k of
 * env e starts at starts[(k % n_episodes)*E + e].  n_episodes = 0 clears the schedule (picker resumes). */
int fleet_set_start_schedule(fleet_handle h, const int32_t* starts, int n_episodes);

/* ---- reset / step, device pointers, asynchronous on the handle's stream --------------------------------
 * mask: u8 [E] or NULL (= all).  obs: f32 [E,obs_dim] (rows of unmasked envs are left untouched).        */
int fleet_reset_dev(fleet_handle h, const uint8_t* mask, float* obs);
int fleet_step_dev(fleet_handle h, const void* actions, int act_dtype, float* obs, double* reward,
                   uint8_t* done, float* terminal_obs /* [E,obs_dim] or NULL */);
/* K consecutive steps in ONE launch for open-loop rollouts (actions known up front): actions [K,E,N];
 * obs = observation after the last step, reward_sum[E] = sum of the K rewards, done_count[E] (or NULL) = number of
 * episode ends among them.  auto_reset must be 1. */
int fleet_step_many_dev(fleet_handle h, int K, const void* actions, int act_dtype, float* obs,
                        double* reward_sum, int32_t* done_count);

/* K consecutive steps in ONE launch with a built-in policy (FLEET_ACT_POLICY_*) evaluated on the device instead of an
 * action tape: the reference's `benchmarking/` harnesses without a host round trip per step.  Outputs as
 * fleet_step_many_dev.  auto_reset must be 1. */
int fleet_rollout_policy_dev(fleet_handle h, int policy, int K, float* obs, double* reward_sum, int32_t* done_count);
/* Parameters of FLEET_ACT_POLICY_NIGHT, as the reference's harness derives them before its loop
 * (benchmarking/night_charging.py:50-73): charging starts when `charging_hour <= hour && charging_minute <= minute`
 * of the env's current row (the reference's own, non-lexicographic test), runs until more than `max_hours`
 * (= int(max_time_needed)) have passed since it started, and on a caretaker fleet the rows of hours 11..14 use the
 * distributed rule instead.  Each env keeps its own "charging since" state, which -- like the reference's loop
 * variable -- survives episode resets; this call clears it.  Not callable while a captured graph is replaying. */
int fleet_set_night_policy(fleet_handle h, int charging_hour, int charging_minute, int max_hours);
/* With auto_reset = 1 the rainflow count stops at the episode's last degradation row.  The reference appends one SOC sample per
 * EV and step to LogDataDeg (fleet_environment.py:655) and runs rainflow.extract_cycles on that log only on the 14:45 rows (:665,
 * rainflow_sei_degradation.py:132); reset() clears the log (:338-339).  What is logged between an episode's last 14:45 row and
 * its end is therefore never read by anybody when the env is reset at its finish -- with 48 h episodes a quarter of all samples
 * -- and the kernels, which count while they log, stop counting there (FLEET_F_RF_UNTIL; state of health, fd_cyc,
 * rainflow_length, observations, rewards: exactly as with the full count, tests/test_rf_tail_gpu.py).  With auto_reset = 0 an
 * env may be stepped past its finish row, and the reference's later 14:45 rows read those samples: the count never stops then
 * (FLEET_F_RF_UNTIL = INT32_MAX, tests/test_past_done_gpu.py).  `on` != 0 keeps the count running to the end of every episode
 * from each env's next reset on (FLEET_F_RF_CYCLES / FLEET_F_RF_STACK then describe the whole series: diagnostics, the
 * adversarial count tests).  Default: off.  Not callable while a captured graph is replaying. */
int fleet_set_rainflow_count_all(fleet_handle h, int on);

/* ---- linear-optimisation benchmark (benchmarking/linear_optimization.py:55-247) ------------------------
 * The reference's perfect-foresight plan, one exact solve per (env, EV): H rows from every env's current row (its live state:
 * time row, SOC of the EVs that are plugged in).  actions [H,E,N] (FLEET_ACT_F32 / FLEET_ACT_F64) is the tape to replay with
 * fleet_step_dev / fleet_step_many_dev from this very state; soc_plan [H+1,E,N] (or NULL) the planned SOC of every row (0 while
 * an EV is away); bound [E] the optimum of the LP relaxation (a lower bound on the reference's MILP), plan_cost [E] the MILP
 * objective of the tape (gap = plan_cost - bound >= 0), both in EUR and summed over the env's EVs; status [E,N] the FLEET_LP_*
 * bits.  Every env must have at least H rows left in its running episode (else FLEET_ERR_INVALID and nothing is launched), so
 * that the replay never auto-resets in the middle of the plan.  Reads the env state synchronously (one small copy), then runs
 * asynchronously on the handle's stream; device pointers.  Not available with real_time = 1.  Two calls on the same state give
 * bit-identical outputs. */
#define FLEET_LP_UNREACHABLE 1   /* a parking session cannot reach target_soc by its departure row: its target was lowered to the
                                    highest reachable SOC (full power on every row)                                          */
#define FLEET_LP_NEG_RETURN 2    /* a SOC_on_return (or a starting SOC) below 0 was clamped to 0                            */
#define FLEET_LP_ABOVE_TARGET 4  /* a starting SOC or SOC_on_return above target_soc was clamped to target_soc               */
#define FLEET_LP_GRID_NEGATIVE 8 /* a row of the horizon has load - pv > grid_connection: its grid limit was taken as 0       */
int fleet_lp_plan_dev(fleet_handle h, int H, void* actions, int act_dtype, double* soc_plan, double* bound, double* plan_cost,
                      int32_t* status);

/* ---- reset / step, host pointers, synchronous ------------------------------------------------------------ */
int fleet_reset_host(fleet_handle h, const uint8_t* mask, float* obs);
/* terminal_obs (or NULL): rows of envs that finished in this step are written; all other rows are left untouched.
 * `obs` / `actions` may be any host memory: buffers from fleet_host_alloc (pinned) are transferred to / from directly; a
 * pageable `obs` receives the observations in pieces through a pinned buffer of the handle, each piece copied to it while
 * the next ones are still on the link. */
int fleet_step_host(fleet_handle h, const void* actions, int act_dtype, float* obs, double* reward,
                    uint8_t* done, float* terminal_obs);

/* The episodes that ended in the last fleet_step_host call (the one with a terminal_obs buffer): their env indices in
 * ascending order, returns (episode.cumulative_reward) and lengths -- what SB3's Monitor wrapper would put into
 * info["episode"].  The pointers refer to the handle's own host buffer and stay valid until the next step. */
int fleet_last_step_episodes(fleet_handle h, int32_t* n, const int32_t** env_idx, const double** ep_return, const int32_t** ep_len);

/* Pinned (page-locked) host memory for the *_host entry points: observations / actions in such buffers cross PCIe straight
 * out of / into them at the full link rate; any other host pointer is staged through the handle's own pinned mirrors (one
 * extra memcpy).  Independent of any handle; free with fleet_host_free. */
int fleet_host_alloc(size_t bytes, void** out);
int fleet_host_free(void* p);

/* ---- state access ------------------------------------------------------------------------------------- */
int fleet_get(fleet_handle h, int field, void* out_host);
/* same, into a DEVICE buffer and asynchronous on the handle's stream (e.g. the episode returns that a multi-GPU run
 * all-gathers for logging, without a host round trip) */
int fleet_get_dev(fleet_handle h, int field, void* out_dev);
/* `FleetEnv.get_dist_factor` (:782-799): hours_needed / (hours_left + 0.001) from a fresh observation, f64 [E,N] */
int fleet_get_dist_factor(fleet_handle h, double* out_host);
/* ---- multi-GPU logging gather ---------------------------------------------------------------------
 * Envs are independent: one process per GPU, each with a handle for its own contiguous env range (FleetParams.env_id_offset),
 * nothing exchanged on the data path.  The one collective is the gather of the finished episodes' returns / lengths for
 * logging -- ONE RCCL all-gather over xGMI, enqueued on the handle's stream, no PyTorch in the process needed (the Python
 * package does the same through torch.distributed, fleetrl_amd/distributed.py).  librccl is opened at run time.
 *   fleet_rccl_unique_id       rank 0 makes the 128-byte id; the caller's launcher hands it to the other ranks (file, env, MPI ...)
 *   fleet_rccl_comm_create     every rank: ncclCommInitRank on `device`; *comm is an ncclComm_t
 *   fleet_gather_episode_stats_rccl   out_dev: DEVICE f64 [world_size, 2, E]: per rank, last_ep_return[E] then last_ep_len[E]
 *                              (as float64) of that rank's envs; every rank must have the same E.  Asynchronous on the
 *                              handle's stream (fleet_synchronize before reading). */
#define FLEET_RCCL_UNIQUE_ID_BYTES 128
int fleet_rccl_unique_id(void* id128);
int fleet_rccl_comm_create(int device, int world_size, int rank, const void* id128, void** comm);
int fleet_rccl_comm_destroy(void* comm);
int fleet_gather_episode_stats_rccl(fleet_handle h, void* comm, int world_size, double* out_dev);

/* ---- device-side data log (FleetParams.log_data = 1) ---------------------------------------------------------------
 * What `FleetEnv.get_log()` (:741-748) returns is rebuilt from this ring: row k of env e (k counted since creation or the
 * last fleet_log_clear; the ring holds the last `capacity` of them, row k in slot k % capacity) is
 *   row [slot,E]      i32  table row of episode.time; bit 31 set: the row reset() writes (zeros + observation + SoH)
 *   env [slot,E,4]    f64  reward, cashflow, overload_amount [kW], cum_soc_missing     (Penalties = reward - cashflow *
 *                          price_multiplier and the absolute values are the caller's, :659-661)
 *   ev  [slot,E,4,N]  f64  action, (dis)charging energy per EV [kWh] (ev_charger.py:114,174), degradation, SoH
 *   obs [slot,E,obs_dim] f32  the observation logged with the row
 * The step that ends an episode is not logged (:679); with auto-reset the next row is the reset row of the next episode.
 * With real_time = 1 every table row the skipping loop passes gets its row, like in the reference (:677-690). */
int fleet_log_capacity(fleet_handle h);  /* rows per env; 0 when the log is off */
/* rows the ring has already overwritten, summed over the envs (sum of max(pos - capacity, 0)): what a caller that wants every
 * row -- like the reference's unbounded DataLogger -- has lost; size FleetParams.log_capacity so that this stays 0 */
int fleet_log_dropped(fleet_handle h, int64_t* rows);
/* copy the ring to HOST buffers (any of them may be NULL); pos [E] = rows written so far per env; synchronous */
int fleet_log_read(fleet_handle h, int32_t* pos, int32_t* row, double* env, double* ev, float* obs);
int fleet_log_clear(fleet_handle h);     /* forget all rows (asynchronous on the handle's stream) */

/* The ring reduced to the numbers of the reference's evaluation (agent_eval/basic_evaluation.py `BasicEvaluation.compare`,
 * `plot_action_dist`) ON THE DEVICE, so that a few kilobytes per env come back instead of the ring (entry added under
 * FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays).  DESIGN.md "The data log, summarised on the
 * device"; tests/logsum_model.py restates it.
 *
 * Window of env e: pos = rows written so far, k0 = max(0, pos - capacity), k1 = max(k0, pos - drop_last); the kept rows
 * k0 <= k < k1, oldest first, row k in slot k % capacity, j = k - k0.  (`drop_last`: the reference drops its last two rows,
 * `log_RL.iloc[0:-2]`, and a vec env with auto-reset has logged one reset row more than the reference.)
 * Per row, in float64 without contraction: reset = bit 31 of `row`, t = its low 31 bits;
 *   reward = env[0], cashflow = env[1], penalty = reset ? 0 : reward - (cashflow * price_multiplier)   (quirk Q13, two roundings)
 *   overload = fabs(env[2]), socv = fabs(env[3]), viol = socv > 0
 *   deg[c] = (!reset && deg_mode != FLEET_DEG_NONE && the table row t is 14:45) ? ev[2][c] : 0
 *   charge[c] = reset ? 0 : (energy of the last EV <= c with action >= 0, else 0) + (energy of the last EV <= c with action < 0,
 *               else 0)                                                                                 (quirk Q8)
 *   row_power = (sum of charge[c] over the EVs) / N; the EV sum is, per chunk of 64 EVs, a xor butterfly over 64 lanes (offsets
 *               1, 2, 4, ..., 32; absent EVs are +0.0), and the chunks are added in ascending order to +0.0
 *   slot s = (60 * hour + minute) / minutes_per_step of S = 1440 / minutes_per_step time-of-day slots
 * Order of every sum: the accumulator starts at +0.0 and adds its rows of one 64-row block (j / 64) in ascending j; the block
 * partials are then added to +0.0 in ascending block order.  No atomics: the result does not depend on the launch geometry.
 * Outputs, DEVICE pointers, every one but `scal` may be NULL:
 *   scal     f64 [E,8]     window rows, sum reward, sum cashflow, sum penalty, sum overload, sum socv, sum viol (a count), the
 *                          number of 14:45 non-reset rows
 *   deg_sum  f64 [E,N]     sum deg[c]
 *   soh_last f64 [E,N]     ev[3][c] of row k1 - 1; NaN for an empty window
 *   prof_sum f64 [E,S]     sum row_power per slot;   prof_cnt i32 [E,S]  rows per slot
 *   hist     i32 [E,bins]  the logged actions of EV `hist_ev` (-1: of every EV) over all window rows, reset rows included, as
 *                          np.histogram(a, bins, range=(lo, hi)) counts them: edge[i] = lo + i * ((hi - lo) / bins) for i < bins,
 *                          edge[bins] = hi; a value falls into the largest i with edge[i] <= a, a == hi into the last bin;
 *                          a < lo, a > hi and NaN are not counted
 * Two launches (block partials: one wavefront per env and 64-row block, one EV per lane; then the fold), enqueued on the handle's
 * stream behind everything the handle has enqueued -- a run on the library's own queue is waited for first, as in
 * fleet_log_read -- and nothing else: no copy, no synchronisation (fleet_synchronize before reading).  The scratch for the
 * partials belongs to the handle: allocated by the first call, freed by fleet_destroy.
 * FLEET_ERR_INVALID, with nothing launched, for: the log being off; a null `args` or args_size != sizeof(FleetLogSummaryArgs); a
 * null `scal`; drop_last < 0; bins outside 1..256 when `hist` is given; hi <= lo or a NaN bound; hist_ev outside -1..N-1 (the last
 * two whether `hist` is given or not: a call states a valid histogram or the defaults 1, -1.0, 1.0, -1); a `prof_*` pointer on a handle whose tables are an irregular time grid or whose step is no whole divisor of a day in minutes (the
 * time-of-day slot is not defined there). */
typedef struct FleetLogSummaryArgs {
  int32_t drop_last;  /* newest rows per env left out of the window (>= 0) */
  int32_t bins;       /* histogram bins, 1..256 */
  int32_t hist_ev;    /* the EV whose actions are counted, or -1: every EV */
  int32_t reserved;   /* 0 */
  double lo, hi;      /* histogram range */
  double* scal;
  double* deg_sum;
  double* soh_last;
  double* prof_sum;
  int32_t* prof_cnt;
  int32_t* hist;
} FleetLogSummaryArgs;
int fleet_log_summary_dev(fleet_handle h, const FleetLogSummaryArgs* args, size_t args_size);

/* Device-side errors -- the conditions under which the reference raises inside step(): `TypeError("Observation format not
 * recognized")` fleet_environment.py:610, `TypeError("DoD too large.")` / `TypeError("Life degradation is negative")` /
 * `RuntimeError("Degradation calculation is not correct")` rainflow_sei_degradation.py:164-167,179-180,209-210, and a table
 * lookup past the last row -- set FLEET_DEVERR_* bits per env (sticky).
 *   - fleet_step_host returns FLEET_ERR_STATE from the very call whose step raised them (its outputs are still complete): the OR
 *     of all bits travels in the block that brings rewards and dones back, no extra launch or transfer.
 *   - the *_dev entry points are asynchronous: poll with fleet_check_errors (one small launch + copy). */
/* FLEET_ERR_STATE if any env has device error bits set; fleet_last_error names the first such env, its table row and the bits */
int fleet_check_errors(fleet_handle h);
/* the OR of all envs' error bits as of the last fleet_step_host (no device work) */
int fleet_last_step_error_bits(fleet_handle h, uint32_t* bits);

/* ---- env state: save, restore, fork (fleet_state.hip; DESIGN.md "Env state in the caller's hands") -------------------------
 * "The state" of a handle is everything a step reads that a step or a reset has written (the list: fleet_device.h, beside FleetDev):
 * per env the hot / schedule / SoH / soc_deg / SEI records, the env record, the EVs' rainflow rows (rainflow degradation), the
 * night policy's window state, the length of the last episode and the data-log ring (log_data = 1); per handle the start schedule,
 * the night-policy parameters and the fleet_set_rainflow_count_all switch.  Tables, scalars, streams and prepared launches are not.
 *
 * A state is a BLOB: a FleetStateHeader at offset 0, then one plain copy of every array ("section") at a 256-byte-aligned offset,
 * in the order of the FLEET_SEC_* ids; the bytes between two sections are zero.  The header carries a FINGERPRINT -- the FleetParams
 * fields that fix the layout and the meaning of the state, and a 64-bit hash of the table contents (fleet_state_table_hash, computed
 * once by fleet_create) -- and a blob is only loaded into, and envs are only forked between, handles whose fingerprints are equal.
 * num_envs is not part of it (a fork may cross handles of different E; a load needs the same E); auto_reset and env_id_offset are
 * not either: the start-row sampler is keyed by the GLOBAL env id, so a state loaded under another env_id_offset continues its
 * running episodes unchanged and draws other start rows from the next reset on.
 * A handle with device error bits raised (fleet_check_errors) is neither saved nor forked: FLEET_ERR_STATE. */
#define FLEET_STATE_MAGIC 0x4554415453544c46ull   /* "FLTSTATE" read as a little-endian 64-bit word */
#define FLEET_STATE_ALIGN 256
#define FLEET_SEC_HOT 0          /* [E,N]  16 B  hot record                                                   */
#define FLEET_SEC_RUN 1          /* [E,N]  16 B  schedule record of the next row                              */
#define FLEET_SEC_SOH 2          /* [E,N]  f64                                                                */
#define FLEET_SEC_SOC_DEG 3      /* [E,N]  f64                                                                */
#define FLEET_SEC_SEI 4          /* [E,N]  4 x f64  fd_cyc, fd_cal, l, soh                                    */
#define FLEET_SEC_ENV 5          /* [E]    64 B  env record                                                   */
#define FLEET_SEC_NIGHT_START 6  /* [E]    i32   night policy: row the charging window opened on              */
#define FLEET_SEC_LAST_LEN 7     /* [E]    i32   length of the last finished episode                          */
#define FLEET_SEC_RF_ROWS 8      /* [E*N, rf_row_stride] f64  rainflow rows (header + stack); FLEET_DEG_RAINFLOW only */
#define FLEET_SEC_LOG_POS 9      /* [E] i32                      the data-log ring; log_data = 1 only         */
#define FLEET_SEC_LOG_ROW 10     /* [log_cap,E] i32                                                           */
#define FLEET_SEC_LOG_ENV 11     /* [log_cap,E,4] f64                                                         */
#define FLEET_SEC_LOG_EV 12      /* [log_cap,E,4,N] f64                                                       */
#define FLEET_SEC_LOG_OBS 13     /* [log_cap,E,obs_dim] f32                                                   */
#define FLEET_SEC_SCHED 14       /* [sched_n,E] i32  the start schedule; absent from fleet_state_layout (its size belongs to the
                                    handle, not to FleetParams): a blob with a schedule is longer than the layout's total      */
#define FLEET_STATE_SECTIONS 16
typedef struct FleetStateSection {
  uint64_t offset;  /* from the start of the blob, a multiple of FLEET_STATE_ALIGN */
  uint64_t bytes;   /* 0: the section is absent */
} FleetStateSection;
typedef struct FleetStateLayout {
  int32_t struct_bytes;   /* sizeof(FleetStateLayout) */
  int32_t alignment;      /* FLEET_STATE_ALIGN */
  uint64_t header_bytes;  /* sizeof(FleetStateHeader) rounded up to the alignment: where section 0 starts */
  uint64_t total_bytes;   /* of a blob without a start schedule */
  int32_t num_envs, num_cars, obs_dim;
  int32_t stack_cap;      /* entries of an EV's rainflow stack workspace (0 without rainflow degradation) */
  int32_t rf_row_stride;  /* f64 words per rainflow row: 6 header words + the stack, rounded up to 16 */
  int32_t log_cap;        /* rows per env of the data-log ring (0: off) */
  FleetStateSection sec[FLEET_STATE_SECTIONS];
} FleetStateLayout;
typedef struct FleetStateFingerprint {
  int32_t num_cars, table_rows, episode_steps, deg_mode, real_time;
  int32_t price_lookahead, bl_pv_lookahead, include_building, include_pv, aux, normalize;  /* the observer: obs_dim, log rows */
  int32_t stack_cap, rf_row_stride, log_cap;
  int32_t picker_mode, reserved;
  uint64_t seed;
  double dt;
  uint64_t table_hash;
} FleetStateFingerprint;
typedef struct FleetStateHeader {
  uint64_t magic;         /* FLEET_STATE_MAGIC */
  int32_t abi_version;    /* FLEET_ABI_VERSION of the library that wrote the blob */
  int32_t header_bytes;   /* sizeof(FleetStateHeader) */
  FleetStateFingerprint fp;
  int32_t num_envs;       /* E: must match on load */
  int32_t env_id_offset;  /* recorded; may differ on load */
  int32_t obs_dim;
  int32_t night_hour, night_minute, night_limit_s;  /* fleet_set_night_policy (night_hour < 0: not configured) */
  int32_t rf_count_all;   /* fleet_set_rainflow_count_all */
  int32_t sched_n;        /* episodes of the start schedule (0: none) */
  uint64_t total_bytes;   /* of this blob, the schedule included */
  FleetStateSection sec[FLEET_STATE_SECTIONS];
} FleetStateHeader;

/* No device needed.  Sizes, offsets and alignment of every section for these parameters (regular time grid: on an irregular one
 * the rainflow workspace follows the tables' finish rows, and the header of a saved blob is the authority). */
int fleet_state_layout(const FleetParams* p, FleetStateLayout* out);
/* No device needed.  The 64-bit hash of the table contents that fleet_create computes, 8 bytes at a time: `there` and every
 * per-row array of FleetTables in full, of time_left and soc_on_return every 16th row and the last one (hashing all of them cost
 * 11 % of fleet_create at T = 35 040, N = 50; the subset's cost: DESIGN.md, "Env state in the caller's hands").  Tables that differ only in time_left / soc_on_return values of the
 * rows in between hash alike. */
int fleet_state_table_hash(const FleetParams* p, const FleetTables* t, uint64_t* hash);
/* No device needed.  Does the blob whose first `bytes` bytes start at blob_header_host fit a handle created from `p` and tables
 * of hash `table_hash`?  FLEET_ERR_INVALID (fleet_last_error(NULL) names the field) for a wrong magic, ABI version, num_envs, a
 * fingerprint field that differs, or a blob shorter than its header says. */
int fleet_state_check(const FleetParams* p, uint64_t table_hash, const void* blob_header_host, uint64_t bytes);
/* Bytes a blob of this handle needs now (fleet_state_layout's total plus the start schedule, if one is set). */
int fleet_state_bytes(fleet_handle h, uint64_t* bytes);
/* Save: one copy per section on the handle's stream, after a direct run has drained.  Every save first reads the handle's error
 * word back (one 4-byte copy and a synchronise: what the stream holds is finished when the call returns from that); _dev then
 * only enqueues -- the blob is device memory, 16-byte aligned, and valid once the stream has got there -- and _host waits for the
 * copies.  `bytes` = the size of the buffer, at least fleet_state_bytes.  Two saves of one state are byte-identical. */
int fleet_state_save_dev(fleet_handle h, void* blob_dev, uint64_t bytes);
int fleet_state_save_host(fleet_handle h, void* blob_host, uint64_t bytes);
/* Load: the header is validated before the device state is touched (_dev reads it back first: one small synchronous copy); then
 * the sections are copied in, the start schedule, night-policy parameters and the count-all switch are restored, the host path's
 * finished-episode list and last error word are cleared.  The handle then continues bit-identically to the one that was saved. */
int fleet_state_load_dev(fleet_handle h, const void* blob_dev, uint64_t bytes);
int fleet_state_load_host(fleet_handle h, const void* blob_host, uint64_t bytes);
/* Fork: env src_idx[i] of `src` is copied to env dst_idx[i] of `dst` (HOST index arrays, n pairs) by one kernel on dst's stream,
 * ordered behind src's stream (and src's stream behind it).  dst may be src.  Like a save it first reads both handles' error
 * words back, which drains their streams; the index upload and the kernel are then enqueued and not waited for.  Checked on the host before anything is launched
 * (FLEET_ERR_INVALID): same device, equal fingerprints (E may differ), indices in range, no duplicate in dst_idx (src_idx may
 * repeat: broadcast), disjoint index sets when dst == src.  FLEET_ERR_UNSUPPORTED when either handle has the data log on;
 * FLEET_ERR_STATE when either has device error bits raised.  Of a rainflow row only the live part moves (the header and the
 * source's stack entries); the destination's words beyond it keep their old, unread contents.
 * The copy includes the episode counter: the destination continues the source's running episode bit-identically (same actions,
 * same outputs) and at its next reset draws the start row of (its OWN global env id, the copied episode count), or its own column
 * of its handle's start schedule.  The night policy's parameters and the start schedule stay the destination handle's own. */
int fleet_fork_envs(fleet_handle dst, fleet_handle src, const int32_t* dst_idx_host, const int32_t* src_idx_host, int n);

/* ---- measurement helpers (bench.py): HIP events on the handle's stream ------------------------------- */
int fleet_timer_start(fleet_handle h);
int fleet_timer_stop(fleet_handle h, float* elapsed_ms);  /* synchronises on the stop event */
/* the same in two halves, for several handles whose streams run concurrently: record every handle's stop event first
 * (asynchronous), then read them (each read synchronises on its own stop event) */
int fleet_timer_mark(fleet_handle h);
int fleet_timer_read(fleet_handle h, float* elapsed_ms);
/* launch `steps` single-step launches back to back from a device-resident action tape [tape_len,E,N]
 * (step i uses tape row i % tape_len).  `use_graph`: how the launches reach the GPU --
 *   FLEET_LAUNCH_EAGER   one hipLaunchKernel per step on the handle's stream
 *   FLEET_LAUNCH_GRAPH   a captured hipGraph of whole tape cycles (>= 64 launches), replayed; shorter remainders eagerly
 *   FLEET_LAUNCH_DIRECT  AQL dispatch packets written by the library into an HSA queue of the handle's own, with the cache
 *                        actions HIP attaches to every kernel boundary reduced to what a run of steps needs: every launch still
 *                        invalidates the per-CU caches, only the LAST launch of the run writes the L2s back: no launch
 *                        waits for the previous one's write-back (workgroup w of every launch of a run stays on one die, so a die
 *                        only reads state it wrote itself; probed when the queue is opened, recorded at the start of every run and
 *                        checked by every launch: FLEET_DEVERR_PLACEMENT, fleet_direct_placement).
 *                        Semantics: asynchronous like the others, but NOT on the HIP stream -- the run starts after everything
 *                        the stream holds has completed (the call waits for that), nothing of it is visible before it has
 *                        completed, and every later call on the handle (fleet_synchronize, a step, a get ...) waits for it first;
 *                        fleet_stream_query reports it.  What a run writes: the state after all its steps, and `obs`, `reward`
 *                        and `done` of its LAST step.  Since nothing is visible before the run has completed, the observation
 *                        rows of the steps before the last -- which the last one overwrites -- are not stored at all (their
 *                        launches skip the observation arithmetic and stores; with one EV per lane also the reward and done
 *                        stores, see fleet_set_direct_state_only).  A caller that needs every step's observation uses
 *                        fleet_step_dev or another mode.
 *                        Single-step configurations only (no real_time, no data log);
 *                        needs libfleet_hip.gfx950.hsaco beside the library (fleetrl_amd.build).  */
#define FLEET_LAUNCH_EAGER 0
#define FLEET_LAUNCH_GRAPH 1
#define FLEET_LAUNCH_DIRECT 2
/* FLEET_LAUNCH_DIRECT covers a batch of more wavefronts than the device holds at once (>= 6144, envs of up to 64 EVs) with two
 * ranges of workgroups on TWO queues, each an in-order chain of its own (the halves drift apart and overlap: 16384 x 50 -17 % per
 * step); FLEET_LAUNCH_DIRECT_ONE_QUEUE never does.  fleet_direct_queues: how the handle's last direct run was laid out (0: none yet). */
#define FLEET_LAUNCH_DIRECT_ONE_QUEUE 3
int fleet_run_tape_dev(fleet_handle h, int steps, const void* tape, int tape_len, int act_dtype,
                       float* obs, double* reward, uint8_t* done, int use_graph);

int fleet_direct_queues(fleet_handle h);

/* What FLEET_LAUNCH_DIRECT relies on, as probed when the handle opened its queue (opens it if need be):
 * map8[k] = the die (HW_REG_XCC_ID) that chain of probe launches found workgroups w with (w & 7) == k on; num_xcc = dies of the
 * device; any_grid = 1 if the map also held across launches whose grids are not multiples of 8 workgroups.  The map is information:
 * the die a queue deals from moves whenever a queue is created or destroyed in the process, so every run records the map afresh on
 * the device (its first launch) and every step launch checks the die it runs on against that record (FLEET_DEVERR_PLACEMENT).  FLEET_ERR_UNSUPPORTED: the probe
 * found the placement not periodic or not stable from launch to launch, and the mode is refused on this platform. */
int fleet_direct_placement(fleet_handle h, int32_t map8[8], int32_t* num_xcc, int32_t* any_grid);
/* How a grid of `grid_workgroups` is laid over the handle's queues (a pure function, no device needed): returns 1 (part_grid[0] = the
 * whole grid) or 2 (two ranges of workgroups: part_grid[0] a multiple of 8 that fits the kernel's 16-bit first-workgroup field). */
int fleet_direct_split_plan(uint32_t grid_workgroups, int split, uint32_t part_grid[2]);
/* Which instance of the step kernel a launch of this kind takes, and its grid of workgroups for `num_envs` envs (a pure function, no
 * device and no handle needed; it runs the library's own launch planner).  A launch is described by the handle's configuration
 * (num_cars, deg_mode, real_time, log_data) and by the call: act_mode = FLEET_ACT_F32 / FLEET_ACT_F64 (an action buffer) or a
 * FLEET_ACT_POLICY_*, K = steps per launch, has_done_count = whether fleet_step_many_dev / fleet_rollout_policy_dev got a
 * done_count buffer (fleet_step_dev, fleet_step_host and the tape replays: K = 1, has_done_count = 0).  name: e.g.
 * "G64.rainflow.single.f32" (the benchmark's kernel), "G32.linear.multi.policy", "G64w.none.multi.log": lanes per env (`w`: every
 * lane walks several EVs), degradation model, single step or K steps per launch, what the instance carries.  Every distinct name is
 * separately compiled code; tests/test_step_instances_cpu.py keeps a test case for each.  FLEET_ERR_INVALID: an argument out of
 * range or a name buffer that is too short (48 bytes are enough). */
int fleet_step_instance(int num_envs, int num_cars, int deg_mode, int real_time, int log_data, int act_mode, int K,
                        int has_done_count, char* name, size_t name_bytes, uint32_t* grid);
/* Up to this many EVs per env every EV has a lane of its own (groups of up to four wavefronts per env); beyond it the lanes of one
 * wavefront walk several EVs each. */
int fleet_max_evs_per_lane_group(void);
/* State-only launches of a run on the library's own queue (fleet_direct.hip; DESIGN.md section 4 "What a run writes").
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * Of a FLEET_LAUNCH_DIRECT run only the last launch's outputs can be read.  Where every EV has a lane of its own and an env is one,
 * two or four whole wavefronts (33..256 EVs per env: groups of 64, 128 or 256 lanes), the single-step kernel has a state-only
 * twin, compiled without anything that feeds `obs`, `reward`, `done` or the cashflow, and every packet of a run but its last takes
 * it.  Results are bit for bit those of the live instance with the run-time flag.
 * fleet_set_direct_state_only: on != 0 (the default) uses the twin where there is one; 0 keeps the live instance for every packet
 * (A/B measurements, tests).  Waits for the handle's run in flight; the prepared argument blocks are rebuilt at the next run.
 * fleet_direct_packet_counts: packets the handle's queue was given so far with the live instance and with the twin (either pointer
 * may be NULL; zeros before the first direct run).
 * fleet_step_has_state_only: whether a launch of this kind has a twin -- a pure function of fleet_step_instance's arguments, no
 * device needed; *has_twin = 1 exactly for single-step launches (K = 1, no done_count, an action buffer, no real_time, no data
 * log) of groups of 64, 128 or 256 lanes with one EV per lane.  FLEET_ERR_INVALID for the arguments fleet_step_instance refuses. */
int fleet_set_direct_state_only(fleet_handle h, int on);
int fleet_direct_packet_counts(fleet_handle h, uint64_t* live, uint64_t* state_only);
int fleet_step_has_state_only(int num_envs, int num_cars, int deg_mode, int real_time, int log_data, int act_mode, int K,
                              int has_done_count, int32_t* has_twin);
/* TEST HOOK for the placement guard (the handle must have run through its own queue before) --
 * kind 1: the handle's NEXT run gets a placement record shifted by one workgroup: what its launches would see if the queue's first
 *         die had moved in the middle of the run;
 * kind 2: in the prepared argument block of tape row `tape_row`, the grid's first workgroup shifted by one (every workgroup steps its
 *         neighbour's envs: the state IS corrupted).
 * The next run (through that row) must raise FLEET_DEVERR_PLACEMENT. */
int fleet_debug_direct_fault(fleet_handle h, int kind, int tape_row);

/* `regions` timed regions of exactly `steps` launches each (as fleet_run_tape_dev), enqueued back to back on the handle's stream
 * with a HIP event before and after each: the kernels' own time per region, without the host's gaps between regions.
 * _begin only enqueues (several handles' streams can be filled before any is read); _read waits and returns the per-region
 * device durations in milliseconds (HOST array [regions]). */
/* (FLEET_LAUNCH_DIRECT: the regions are the runs' own dispatch timestamps -- start of the first launch to end of the last) */
int fleet_time_regions_begin(fleet_handle h, int regions, int steps, const void* tape, int tape_len, int act_dtype,
                             float* obs, double* reward, uint8_t* done, int use_graph);
int fleet_time_regions_read(fleet_handle h, float* region_ms);

/* like fleet_run_tape_dev without a graph, but brackets EVERY launch with its own HIP event pair on the handle's
 * stream and returns the per-launch device durations in milliseconds (HOST array [steps]); synchronous. */
int fleet_time_steps_dev(fleet_handle h, int steps, const void* tape, int tape_len, int act_dtype, float* obs,
                         double* reward, uint8_t* done, float* per_launch_ms);

/* ---- self-test --------------------------------------------------------------------------------------- */
/* The charge arithmetic (EvCharger.charge, ev_charger.py:114,128,189) divides by eta_c and by the battery capacity; the kernels
 * form both quotients from a reciprocal with a residual correction instead of the IEEE division sequence.  This entry runs both
 * forms on `n_pairs` pseudo-random operand pairs of the charge arithmetic's ranges on the device and returns how many quotients
 * differ in any bit: mismatches[0] for `need / eta_c`, mismatches[1] for `energy / cap` (expected: 0 and 0). */
int fleet_selftest_division(int device, uint64_t n_pairs, uint64_t seed, uint64_t* mismatches);
/* The stress of a closed rainflow cycle (deg_rate_cycle, rainflow_sei_degradation.py:68-80: (kd1 * dod^kd2 + kd3)^-1 * e^(k_sigma *
 * (soc - sigma_ref)) * stress_temp) is evaluated with a hardware float32 logarithm inside dod^-0.501 and polynomial exponentials instead
 * of the library's pow / exp.  This entry evaluates both forms on `n_samples` pseudo-random (depth of discharge, mean SOC, cycle weight)
 * triples of the reachable domain on the device and returns the largest relative difference (expected: < 1e-8; the degradation it
 * feeds is a 1e-5-sized correction to the state of health). */
int fleet_selftest_stress(int device, uint64_t n_samples, uint64_t seed, double* max_rel_err);

/* ---- running observation / reward normaliser (fleet_norm.hip) ------------------------------------------------------------
 * stable-baselines3 2.3.2 `VecNormalize` on the device (DESIGN.md "VecNormalize on the device").  State: obs_rms {mean[D],
 * var[D], count}, ret_rms {mean, var, count} (start 0 / 1 / 1e-4) and the discounted returns[E] (start 0), all float64.
 *   reset:  returns = 0; if training && norm_obs: obs_rms.update(obs); obs' = normalise(obs)
 *   step:   if training && norm_obs: obs_rms.update(obs)          (the post-auto-reset rows; terminal rows never)
 *           obs' = clip((obs - mean) / sqrt(var + epsilon), +-clip_obs)   in float64, rounded once to float32
 *           if training: returns = returns * gamma + r; ret_rms.update(returns)      (also with norm_reward = 0)
 *           r'   = clip(r / sqrt(ret_rms.var + epsilon), +-clip_reward)
 *           terminal' = normalise(terminal) for the rows of done envs (same, updated statistics); returns[done] = 0
 *   update(X, n rows): d = mean(X) - mean; tot = count + n; mean += d * n / tot;
 *           var = (var * count + var(X) * n + d * d * count * n / tot) / tot; count = tot
 * r is the raw float64 reward rounded to float32 (what VecNormalize sees on top of FleetVecEnv, whose rewards are float32); the
 * batch moments are accumulated in float64 (SB3 accumulates the observations' in float32).  No floating-point atomics: results
 * are bit-reproducible from run to run.  A normaliser has its own E and D; calls on one normaliser are serialised by the caller. */
typedef struct FleetNormParams {
  int32_t struct_bytes;  /* sizeof(FleetNormParams) */
  int32_t num_envs;      /* E >= 1 */
  int32_t obs_dim;       /* D >= 1 */
  int32_t training, norm_obs, norm_reward;
  double clip_obs, clip_reward;  /* > 0 */
  double gamma;                  /* 0 <= gamma <= 1 */
  double epsilon;                /* > 0 */
} FleetNormParams;
typedef struct FleetNorm* fleet_norm_handle;

int fleet_norm_create(int device, const FleetNormParams* p, fleet_norm_handle* out);  /* allocates everything the steps need */
int fleet_norm_destroy(fleet_norm_handle n);
const char* fleet_norm_last_error(fleet_norm_handle n);  /* n may be NULL: error of the last failed fleet_norm_create */
/* launch on an external hipStream_t (borrowed; NULL = the null stream) from now on instead of the normaliser's own stream */
int fleet_norm_set_stream(fleet_norm_handle n, void* hip_stream);
/* new training / norm_obs / norm_reward flags and constants; num_envs and obs_dim must stay what they were */
int fleet_norm_configure(fleet_norm_handle n, const FleetNormParams* p);
/* device pointers, asynchronous on the normaliser's stream.  obs may equal raw_obs (in place; fleet_norm_original_host then has
 * no raw observations), reward may equal raw_reward, terminal may equal raw_terminal.  raw_terminal / terminal: [E,D] or NULL;
 * only the rows of done envs are read and written. */
int fleet_norm_reset_dev(fleet_norm_handle n, const float* raw_obs, float* obs);
int fleet_norm_step_dev(fleet_norm_handle n, const float* raw_obs, const double* raw_reward, const uint8_t* done,
                        const float* raw_terminal, float* obs, double* reward, float* terminal);
/* host buffers, synchronous; any pointer may be NULL (not read / not written).  set_state recomputes what the steps derive from
 * the statistics. */
int fleet_norm_get_state(fleet_norm_handle n, double* obs_mean, double* obs_var, double* obs_count, double* ret_mean,
                         double* ret_var, double* ret_count, double* returns);
int fleet_norm_set_state(fleet_norm_handle n, const double* obs_mean, const double* obs_var, const double* obs_count,
                         const double* ret_mean, const double* ret_var, const double* ret_count, const double* returns);
/* the raw observations [E,D] and rewards [E] of the last reset / step (SB3's get_original_obs / get_original_reward), to HOST
 * buffers (either may be NULL).  FLEET_ERR_STATE for the observations after an in-place call (they are gone) or before any call. */
int fleet_norm_original_host(fleet_norm_handle n, float* obs, double* reward);
/* The host path with the normaliser between the env's kernels and the transfers, on h's stream: fleet_reset_host (no mask) /
 * fleet_step_host with normalised obs, reward and terminal rows.  fleet_last_step_episodes keeps reporting the raw episode
 * returns.  FLEET_ERR_INVALID when the normaliser's E, D or device differ from the env's. */
int fleet_reset_host_norm(fleet_handle h, fleet_norm_handle n, float* obs);
int fleet_step_host_norm(fleet_handle h, fleet_norm_handle n, const void* actions, int act_dtype, float* obs, double* reward,
                         uint8_t* done, float* terminal_obs);

/* ---- rollout buffer on the device (fleet_rollout.hip; DESIGN.md "Rollouts on the device") -----------------------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * stable-baselines3 2.3.2 `RolloutBuffer` in device memory: K time rows of E envs, SB3's layout (time-major), float32 throughout,
 *   obs f32[K,E,D]  actions f32[K,E,A]  rewards f32[K,E]  episode_starts u8[K,E]  values f32[K,E]  log_probs f32[K,E]
 *   advantages f32[K,E]  returns f32[K,E]
 * in ONE device allocation, each array at a 256-byte-aligned offset (fleet_rollout_layout), followed by one 32-bit error word.
 * Every *_dev call takes device pointers, only enqueues (no host synchronisation) and runs on the buffer's stream: its own, or
 * the one fleet_rollout_set_stream borrowed.  Calls on one buffer are serialised by the caller.  No atomics, no random numbers.
 *   add     row t <- (obs, actions, f32(reward), episode_start, value, log_prob); a source that IS the row's own address
 *           (fleet_rollout_slot) is not copied: an env / normaliser step wrote it there
 *   finish  SB3's compute_returns_and_advantage, operation for operation in float32: g = f32(gamma), gl = f32(gamma * gae_lambda)
 *           (the product in float64), last = 0; for t = K-1 .. 0:
 *             nnt = 1 - (t == K-1 ? dones : episode_starts[t+1]);  nv = (t == K-1 ? last_values : values[t+1])
 *             delta = (rewards[t] + (g * nv) * nnt) - values[t];   last = delta + (gl * nnt) * last
 *             advantages[t] = last;  returns[t] = last + values[t]
 *   gather  SB3's get() for one minibatch: flat indices i = e * K + t (the order of SB3's swap_and_flatten) -> rows of six arrays */
typedef struct FleetRolloutParams {
  int32_t struct_bytes;  /* sizeof(FleetRolloutParams) */
  int32_t num_envs;      /* E >= 1 */
  int32_t n_steps;       /* K >= 1; E * K < 2^31 */
  int32_t obs_dim;       /* D >= 1; E * max(D, A) <= 2^32 - 2048 * 256 (a time row is copied under a 32-bit item counter that */
  int32_t act_dim;       /* A >= 1;   advances by up to 2048 workgroups * 256 threads: a larger row would never finish) */
  int32_t reserved;      /* 0 */
  double gamma;          /* 0 <= gamma <= 1 */
  double gae_lambda;     /* 0 <= gae_lambda <= 1 */
} FleetRolloutParams;
#define FLEET_ROLLOUT_ALIGN 256
#define FLEET_ROLLOUT_OBS 0
#define FLEET_ROLLOUT_ACTIONS 1
#define FLEET_ROLLOUT_REWARDS 2
#define FLEET_ROLLOUT_EPISODE_STARTS 3
#define FLEET_ROLLOUT_VALUES 4
#define FLEET_ROLLOUT_LOG_PROBS 5
#define FLEET_ROLLOUT_ADVANTAGES 6
#define FLEET_ROLLOUT_RETURNS 7
#define FLEET_ROLLOUT_ARRAYS 8
typedef struct FleetRolloutLayout {
  int32_t struct_bytes;  /* sizeof(FleetRolloutLayout) */
  int32_t alignment;     /* FLEET_ROLLOUT_ALIGN */
  uint64_t total_bytes;  /* of the allocation, the error word included */
  uint64_t offset[FLEET_ROLLOUT_ARRAYS];      /* of array FLEET_ROLLOUT_*, a multiple of the alignment */
  uint64_t bytes[FLEET_ROLLOUT_ARRAYS];       /* K * E * (D | A | 1) * (4 | 1) */
  uint64_t row_bytes[FLEET_ROLLOUT_ARRAYS];   /* of one time row: bytes / K */
  uint64_t error_offset; /* of the 32-bit error word */
} FleetRolloutLayout;
typedef struct FleetRolloutArrays {  /* base addresses (row 0) of the eight arrays, device memory */
  float* obs;
  float* actions;
  float* rewards;
  uint8_t* episode_starts;
  float* values;
  float* log_probs;
  float* advantages;
  float* returns;
} FleetRolloutArrays;
typedef struct FleetRolloutSlot {  /* addresses of ONE time row: what fleet_rollout_add_dev skips when it is handed them */
  float* obs;              /* [E,D] */
  float* actions;          /* [E,A] */
  float* reward;           /* [E]   */
  uint8_t* episode_start;  /* [E]   */
  float* value;            /* [E]   */
  float* log_prob;         /* [E]   */
} FleetRolloutSlot;
typedef struct FleetRollout* fleet_rollout_handle;

/* No device needed.  FLEET_ERR_INVALID (fleet_rollout_last_error(NULL) says why) for parameters fleet_rollout_create refuses. */
int fleet_rollout_layout(const FleetRolloutParams* p, FleetRolloutLayout* out);
/* The parameters are validated BEFORE the device is touched: FLEET_ERR_INVALID for E, K, D or A < 1, E * K >= 2^31, a time
 * row past the limit above (the message states it), gamma or gae_lambda outside [0, 1] (NaN included), a wrong struct_bytes, a null
 * pointer.  Then: one allocation, zero-filled. */
int fleet_rollout_create(int device, const FleetRolloutParams* p, fleet_rollout_handle* out);
int fleet_rollout_destroy(fleet_rollout_handle r);
const char* fleet_rollout_last_error(fleet_rollout_handle r);  /* r may be NULL: error of the last failed create / layout */
/* launch on an external hipStream_t (borrowed; NULL = the null stream) from now on instead of the buffer's own stream; waits for
 * what the previous stream still holds of this buffer's work */
int fleet_rollout_set_stream(fleet_rollout_handle r, void* hip_stream);
int fleet_rollout_arrays(fleet_rollout_handle r, FleetRolloutArrays* out);
/* the addresses of time row t (0 <= t < K).  Pass them as obs_out / done_out of the env or normaliser step that produces the row
 * and again to fleet_rollout_add_dev, which then leaves those arrays alone. */
int fleet_rollout_slot(fleet_rollout_handle r, int t, FleetRolloutSlot* out);
/* One launch: time row t <- the sources (device memory, none NULL).  reward: f64[E] (reward_dtype = FLEET_ACT_F64; what the
 * normaliser and the env emit) or f32[E] (FLEET_ACT_F32), rounded ONCE to float32 as SB3's assignment into its float32 array does.
 * A source equal to the row's own address is skipped.  terminal_value f32[E] (or NULL: off, the reference's behaviour) with
 * done u8[E] (the step's dones, required with it): SB3's time-limit bootstrap, rewards[t,e] = f32(reward[e]) + f32(gamma) *
 * terminal_value[e] where done[e] != 0, in float32.  FLEET_ERR_INVALID: t outside [0, K), a null source. */
int fleet_rollout_add_dev(fleet_rollout_handle r, int t, const float* obs, const float* actions, const void* reward,
                          int reward_dtype, const uint8_t* episode_start, const float* value, const float* log_prob,
                          const float* terminal_value, const uint8_t* done);
/* One launch, one lane per env: advantages and returns of all K rows from the stored rewards, values and episode_starts and from
 * last_values f32[E], dones u8[E] (the value of, and the dones before, the observation after the last row).  Bit-identical to the
 * float32 recurrence above evaluated in NumPy. */
int fleet_rollout_finish_dev(fleet_rollout_handle r, const float* last_values, const uint8_t* dones);
/* One launch: out_x[b] = x[t, e] for indices[b] = e * K + t, b < batch; indices i32[batch] in device memory, the permutation is the
 * caller's.  Any output may be NULL (not wanted).  Rows of obs (and of actions) move as 16-byte words when D (A) is a multiple of
 * 4 and the output is 16-byte aligned, as single floats otherwise.  An index outside [0, K * E) writes nothing for its row and sets
 * the buffer's error word (fleet_rollout_check_errors).  FLEET_ERR_INVALID, before any launch, unless
 * batch * D (batch * A) <= 2^32 - 2048 * 256 for the outputs asked for (the same 32-bit item counter; the message states the
 * limit): gather in pieces. */
int fleet_rollout_gather_dev(fleet_rollout_handle r, const int32_t* indices, int batch, float* out_obs, float* out_actions,
                             float* out_values, float* out_log_probs, float* out_advantages, float* out_returns);
/* Waits for the stream, reads the error word back: FLEET_OK, or FLEET_ERR_STATE (a gather met an index out of range since the last
 * check) -- the word is cleared, so the next check is clean. */
int fleet_rollout_check_errors(fleet_rollout_handle r);

/* ---- replay buffer on the device (fleet_replay.hip; DESIGN.md "Replay on the device") ------------------------------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * stable-baselines3 2.3.2 `ReplayBuffer` (optimize_memory_usage = False) in device memory: a ring of R = max(buffer_size / E, 1)
 * rows of E envs,
 *   observations f32[R,E,D]  next_observations f32[R,E,D]  actions f32[R,E,A]  rewards f32[R,E]  dones u8[R,E]  timeouts u8[R,E]
 * in ONE device allocation, each array at a 256-byte-aligned offset (fleet_replay_layout), followed by one 32-bit error word.
 * The observations and rewards are stored RAW and normalised when a minibatch is sampled, with the normaliser's statistics of that
 * moment (SB3's _get_samples -> _normalize_obs / _normalize_reward).  Every *_dev call takes device pointers, only enqueues (no
 * host synchronisation) and runs on the buffer's stream: its own, or the one fleet_replay_set_stream borrowed.  Calls on one buffer
 * are serialised by the caller.  No atomics.  The host keeps the write position, the `full` flag and the count of drawn minibatches.
 *   add     row pos <- (obs, done ? terminal : next_obs, action, f32(reward), done != 0, timeout); pos = (pos + 1) % R
 *   gather  rows (rows[b], envs[b]) of the five sampled arrays, normalised; dones' = f32(done) * (1 - f32(timeout))
 *   sample  the same at indices drawn on the device: sample b of call c takes one Philox4x32-10 block, key (seed lo, seed hi),
 *           counter (b, 0, c lo, c hi) -> x0..x3;  row = mulhi64(x0 | x1 << 32, upper), env = mulhi64(x2 | x3 << 32, E),
 *           upper = full ? R : pos  (a 64-bit multiply-high: bias <= n / 2^64, never equal to n, no rejection loop)
 *   normalisation (a fleet_norm_handle given): obs' = (float)clip(((double)x - mean[col]) / sd[col], +-clip_obs) when its norm_obs
 *           is set, r' = (float)clip((double)r / ret_sd, +-clip_reward) when its norm_reward is set: the normaliser's own
 *           arithmetic, read from its device block when the launch RUNS, behind the normaliser's last enqueued launch */
typedef struct FleetReplayParams {
  int32_t struct_bytes;  /* sizeof(FleetReplayParams) */
  int32_t num_envs;      /* E >= 1; E <= 2^31 - 2048 * 4 (the env rows are walked under an int that advances by up to 2048 * 4) */
  int32_t buffer_size;   /* transitions, >= 1; R = max(buffer_size / E, 1), R * E < 2^31 */
  int32_t obs_dim;       /* D >= 1; D, A <= 2^31 - 64 (a row's words are walked under an int that advances by the 64 lanes) */
  int32_t act_dim;       /* A >= 1 */
  int32_t reserved;      /* 0 */
  uint64_t seed;         /* Philox key of the index draw */
} FleetReplayParams;
#define FLEET_REPLAY_ALIGN 256
#define FLEET_REPLAY_OBS 0
#define FLEET_REPLAY_NEXT_OBS 1
#define FLEET_REPLAY_ACTIONS 2
#define FLEET_REPLAY_REWARDS 3
#define FLEET_REPLAY_DONES 4
#define FLEET_REPLAY_TIMEOUTS 5
#define FLEET_REPLAY_ARRAYS 6
typedef struct FleetReplayLayout {
  int32_t struct_bytes;  /* sizeof(FleetReplayLayout) */
  int32_t alignment;     /* FLEET_REPLAY_ALIGN */
  int32_t rows;          /* R */
  int32_t reserved;
  uint64_t total_bytes;  /* of the allocation, the error word included */
  uint64_t offset[FLEET_REPLAY_ARRAYS];     /* of array FLEET_REPLAY_*, a multiple of the alignment */
  uint64_t bytes[FLEET_REPLAY_ARRAYS];      /* R * E * (D | A | 1) * (4 | 1) */
  uint64_t row_bytes[FLEET_REPLAY_ARRAYS];  /* of one ring row: bytes / R */
  uint64_t error_offset; /* of the 32-bit error word */
} FleetReplayLayout;
typedef struct FleetReplayArrays {  /* base addresses (row 0) of the six arrays, device memory */
  float* observations;
  float* next_observations;
  float* actions;
  float* rewards;
  uint8_t* dones;
  uint8_t* timeouts;
} FleetReplayArrays;
typedef struct FleetReplay* fleet_replay_handle;

/* No device needed.  FLEET_ERR_INVALID (fleet_replay_last_error(NULL) says why) for parameters fleet_replay_create refuses. */
int fleet_replay_layout(const FleetReplayParams* p, FleetReplayLayout* out);
/* The parameters are validated BEFORE the device is touched: FLEET_ERR_INVALID for E, buffer_size, D or A < 1, R * E >= 2^31, an
 * E, D or A past the limits above (the message states them), a wrong struct_bytes, a null pointer.  Then: one allocation,
 * zero-filled (a failure names its byte count). */
int fleet_replay_create(int device, const FleetReplayParams* p, fleet_replay_handle* out);
int fleet_replay_destroy(fleet_replay_handle r);
const char* fleet_replay_last_error(fleet_replay_handle r);  /* r may be NULL: error of the last failed create / layout */
/* launch on an external hipStream_t (borrowed; NULL = the null stream) from now on instead of the buffer's own stream; waits for
 * what the previous stream still holds of this buffer's work */
int fleet_replay_set_stream(fleet_replay_handle r, void* hip_stream);
int fleet_replay_arrays(fleet_replay_handle r, FleetReplayArrays* out);
/* One launch: ring row pos <- the step's tensors (device memory), then pos advances and wraps.  obs, next_obs f32[E,D], action
 * f32[E,A], reward f64[E] (reward_dtype = FLEET_ACT_F64) or f32[E] (FLEET_ACT_F32), rounded ONCE to float32, done u8[E].
 * terminal f32[E,D] or NULL: next_observations[pos,e] = done[e] ? terminal[e] : next_obs[e]; terminal rows of envs that are not
 * done are never read.  timeout u8[E] or NULL (zeros are stored).  Rows move as 16-byte words when D (A) is a multiple of 4 and the
 * source is 16-byte aligned, as single floats otherwise.  The sources are copied, never adopted in place: in a ring a row written
 * in place would corrupt the oldest transition until the next add. */
int fleet_replay_add_dev(fleet_replay_handle r, const float* obs, const float* next_obs, const float* action, const void* reward,
                         int reward_dtype, const uint8_t* done, const float* terminal, const uint8_t* timeout);
/* One launch, explicit indices: sample b <- transition (rows[b], envs[b]), both i32[batch] in device memory (SB3's _get_samples with
 * given env_indices; the hook for prioritised replay).  Outputs (any may be NULL): out_obs, out_next_obs f32[batch,D] and
 * out_rewards f32[batch] normalised as above when `norm` is not NULL (its obs_dim must be D, else FLEET_ERR_INVALID), out_actions
 * f32[batch,A], out_dones f32[batch] = f32(done) * (1 - f32(timeout)).  A pair outside [0, upper) x [0, E), upper = full ? R : pos,
 * writes nothing for its sample and sets the buffer's error word (fleet_replay_check_errors). */
int fleet_replay_gather_dev(fleet_replay_handle r, const int32_t* rows, const int32_t* envs, int batch, fleet_norm_handle norm,
                            float* out_obs, float* out_actions, float* out_next_obs, float* out_dones, float* out_rewards);
/* One launch, drawn indices (above); the handle's call counter is used and then incremented: the same seed and the same sequence
 * of calls give the same minibatches, on any stream.  out_rows / out_envs i32[batch] (or NULL) receive what was drawn.
 * FLEET_ERR_STATE, before any launch, for an empty buffer. */
int fleet_replay_sample_dev(fleet_replay_handle r, int batch, fleet_norm_handle norm, float* out_obs, float* out_actions,
                            float* out_next_obs, float* out_dones, float* out_rewards, int32_t* out_rows, int32_t* out_envs);
/* Waits for the stream, reads the error word back: FLEET_OK, or FLEET_ERR_STATE (a gather met an index out of range since the last
 * check) -- the word is cleared, so the next check is clean. */
int fleet_replay_check_errors(fleet_replay_handle r);
/* host bookkeeping (any output may be NULL): the next row to be written, whether the ring has wrapped, R, minibatches drawn so far */
int fleet_replay_size(fleet_replay_handle r, int32_t* pos, int32_t* full, int32_t* rows, uint64_t* calls);
/* what a caller needs to resume (the arrays themselves are the caller's to fill): 0 <= pos < R, full 0 / 1, the call counter */
int fleet_replay_set_position(fleet_replay_handle r, int32_t pos, int32_t full, uint64_t calls);

/* ---- MLP policy on the device (fleet_policy.hip; DESIGN.md "The agent's forward pass on the device") ---------------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * The deterministic forward pass of a trained stable-baselines3 MLP policy, float32 throughout, ONE launch per forward.  A policy
 * is one or two heads over the same [E,D] float32 input: head 0 the actor, head 1 an optional critic.  A head is a chain of
 * 1..FLEET_POLICY_MAX_LAYERS linear layers y = W x + b (W float32 [out, in], torch's layout), a hidden activation after every
 * layer but the last, and an output transform after the last:
 *   NONE  y        CLIP  min(max(y, lo), hi) (SB3's clip of a Gaussian policy's mean to the action space)        TANH  tanh(y)
 * Every output element is one chain acc = 0; acc = fmaf(x[k], W[j][k], acc) for k = 0 .. in-1; y = acc + b[j], evaluated by one
 * lane: a row's result does not depend on E, on the row's position in the batch, on the stream or on the other head.  For finite
 * inputs that chain is the result bit for bit (ReLU is y < 0 ? 0 : y, CLIP y < lo ? lo : (y > hi ? hi : y)).  An input element that
 * is not finite reaches no other row; in its own row the result is the chain's or NaN, because the layout's zero padding meets it
 * (inf * 0 in a padded column of a hidden layer, read by the next layer when its `in` is no multiple of 4): 20-1-3 with one +inf
 * input gives NaN where the chain gives the bias or an infinity.
 * Input normalisation (a fleet_norm_handle given): the input is the RAW observation and each element goes through the normaliser's
 * own arithmetic first, x' = (float)clip(((double)x - mean[col]) / sd[col], +-clip_obs), with its statistics as they are when the
 * launch RUNS, behind the normaliser's last enqueued launch; with its norm_obs off the input passes through.  Nothing is updated.
 * Every *_dev call takes device pointers, only enqueues (no host synchronisation) and runs on the policy's stream: its own, or the
 * one fleet_policy_set_stream borrowed.  Calls on one policy are serialised by the caller.  No atomics, no random numbers. */
#define FLEET_POLICY_MAX_HEADS 2
#define FLEET_POLICY_MAX_LAYERS 4
#define FLEET_POLICY_MAX_WIDTH 512
#define FLEET_POLICY_MAX_OBS_DIM 8192
#define FLEET_POLICY_ACT_TANH 0
#define FLEET_POLICY_ACT_RELU 1
#define FLEET_POLICY_OUT_NONE 0
#define FLEET_POLICY_OUT_CLIP 1
#define FLEET_POLICY_OUT_TANH 2
typedef struct FleetPolicyHead {
  int32_t n_layers;                        /* linear layers, 1..FLEET_POLICY_MAX_LAYERS */
  int32_t width[FLEET_POLICY_MAX_LAYERS];  /* outputs of layer l, 1..FLEET_POLICY_MAX_WIDTH; the last one is the head's output width */
  int32_t activation;                      /* FLEET_POLICY_ACT_*, after every layer but the last */
  int32_t output;                          /* FLEET_POLICY_OUT_*, after the last layer */
  int32_t reserved;                        /* 0 */
  float lo, hi;                            /* FLEET_POLICY_OUT_CLIP: lo <= hi */
} FleetPolicyHead;
typedef struct FleetPolicyParams {
  int32_t struct_bytes;  /* sizeof(FleetPolicyParams) */
  int32_t obs_dim;       /* D, 1..FLEET_POLICY_MAX_OBS_DIM */
  int32_t n_heads;       /* 1 (actor) or 2 (actor, critic) */
  int32_t tile_rows;     /* out (fleet_policy_describe): env rows one workgroup takes through every layer; ignored by create */
  FleetPolicyHead head[FLEET_POLICY_MAX_HEADS];
} FleetPolicyParams;
typedef struct FleetPolicy* fleet_policy_handle;

/* The parameters and the weights are validated BEFORE the device is touched: FLEET_ERR_INVALID (fleet_policy_last_error(NULL)
 * says why) for obs_dim outside 1..8192, a width outside 1..512, a layer count outside 1..4, n_heads outside 1..2, an unknown
 * activation or output transform, lo > hi or a NaN bound, a wrong struct_bytes, a null pointer, a weight that is not finite.
 * host_weights: packed float32 in declaration order -- for head 0 then head 1, for each layer W[out, in] (row-major) then b[out]. */
int fleet_policy_create(int device, const FleetPolicyParams* p, const float* host_weights, fleet_policy_handle* out);
int fleet_policy_destroy(fleet_policy_handle h);
const char* fleet_policy_last_error(fleet_policy_handle h);  /* h may be NULL: error of the last failed fleet_policy_create */
/* launch on an external hipStream_t (borrowed; NULL = the null stream) from now on instead of the policy's own stream; waits for
 * what the previous stream still holds of this policy's work */
int fleet_policy_set_stream(fleet_policy_handle h, void* hip_stream);
/* New weights from HOST memory, packed as for create; FLEET_ERR_INVALID (nothing changes) when one is not finite.  The upload is
 * enqueued behind the policy's earlier forwards, and the host waits for it. */
int fleet_policy_load_host(fleet_policy_handle h, const float* weights);
/* New weights from DEVICE memory: `tensors` is a host array of `count` device pointers, torch's parameter tensors in declaration
 * order (W, b per layer, head 0 then head 1; count must be twice the number of layers).  One launch on the policy's stream copies
 * and re-lays them, no host synchronisation: a training loop refreshes the device policy after an optimiser step.  The values are
 * not inspected (that would need the host): a weight that is not finite shows in the outputs. */
int fleet_policy_load_dev(fleet_policy_handle h, const float* const* tensors, int count);
/* One launch: actions f32[E, width of head 0] <- head 0 of obs f32[E,D]; values f32[E, width of head 1] <- head 1 when `values` is
 * not NULL (FLEET_ERR_INVALID on a one-head policy).  norm: NULL, or the normaliser whose statistics the input goes through (its
 * obs_dim must be D and its device the policy's, else FLEET_ERR_INVALID; its num_envs is not looked at).  FLEET_ERR_INVALID for
 * E < 1 or a null obs / actions.  The outputs may feed fleet_step_dev directly (FLEET_ACT_F32). */
int fleet_policy_forward_dev(fleet_policy_handle h, const float* obs, int E, fleet_norm_handle norm, float* actions, float* values);
/* the parameters the policy was created with, and tile_rows */
int fleet_policy_describe(fleet_policy_handle h, FleetPolicyParams* out);

/* ---- exploration actions on the device (fleet_policy.hip; DESIGN.md "Exploration on the device") ---------------------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * What a training loop does between reading a step's observations and stepping the env, in ONE launch on a policy handle: the actor
 * (and the critic when `values` is given) as fleet_policy_forward_dev runs them, the exploration noise drawn on the device, and the
 * sampled action, the action the env steps on, the summed log-probability and the value written where the caller says -- the rows
 * of a rollout slot (fleet_rollout_slot) included, which fleet_rollout_add_dev then leaves alone.  float32 throughout.
 * Noise.  eps[e][j] of env row e and action column j comes from Philox4x32-10 (the generator of fleet_replay_sample_dev) with key
 * (seed lo, seed hi) and counter (env_id_offset + e, j / 4, step lo, step hi): the block's words x0..x3 give the standard normals of
 * columns 4(j/4) .. 4(j/4)+3 by Box-Muller on the pairs (x0, x1) and (x2, x3),
 *   u1 = ((x >> 8) + 1) * 2^-24 in (0, 1],  u2 = (x' >> 8) * 2^-24 in [0, 1),  r = sqrtf(-2 logf(u1)),
 *   even column r * cosf(2 pi u2), odd column r * sinf(2 pi u2)                                    (|eps| <= sqrt(48 ln 2) = 5.77)
 * with the device library's functions.  A draw depends on (seed, global env id, step, column) and on nothing else: not on E, on the
 * row's place in the batch, on the stream, on the critic, or on how the envs are sharded over GPUs.  noise_mode GIVEN reads eps from
 * noise[e][j] instead; DRAW with a non-null `noise` writes what was drawn there.
 * GAUSSIAN (PPO / A2C: SB3's DiagGaussianDistribution with a state-independent log_std = scale[A], read from device memory when the
 * launch runs).  mean = head 0's last layer BEFORE its output transform; std = expf(log_std[j]); a = fmaf(std, eps, mean);
 * actions = a; env_actions = the head's output transform of a (CLIP for PPO: the env sees the clipped action, the buffer keeps the
 * sampled one); log_prob[e] = sum over j of -((a - mean)^2) / (2 * std * std) - log_std[j] - 0.9189385332f, torch's expression on
 * the STORED action, summed in an order that depends on A alone.
 * ACTION_NOISE (TD3 / DDPG: SB3's NormalActionNoise on the unit action space).  d = head 0's output (tanh for TD3);
 * a = d + (shift[j] + sigma[j] * eps) with sigma = scale[A] and shift[A] (NULL: 0), clipped to [noise_lo, noise_hi]; actions and
 * env_actions both get a.
 * UNIFORM (the learning_starts warm-up, action_space.sample()): a = noise_lo + (noise_hi - noise_lo) * u2 of the column's own word,
 * kept below noise_hi where the float32 sum rounds up to it (noise_lo == noise_hi gives noise_lo);
 * no network runs (a small kernel of its own), obs may be NULL, `noise` (when given in DRAW mode) receives u2.
 * `mean` (optional, f32[E, A]) receives mean (GAUSSIAN) or d (ACTION_NOISE).  Every output of a row is a function of that row. */
#define FLEET_EXPLORE_GAUSSIAN 0
#define FLEET_EXPLORE_ACTION_NOISE 1
#define FLEET_EXPLORE_UNIFORM 2
#define FLEET_EXPLORE_NOISE_DRAW 0
#define FLEET_EXPLORE_NOISE_GIVEN 1
typedef struct FleetExploreArgs {
  int32_t struct_bytes;    /* sizeof(FleetExploreArgs) */
  int32_t mode;            /* FLEET_EXPLORE_GAUSSIAN / _ACTION_NOISE / _UNIFORM */
  int32_t noise_mode;      /* FLEET_EXPLORE_NOISE_DRAW / _GIVEN */
  int32_t reserved0;       /* 0 */
  uint64_t seed;           /* Philox key */
  uint64_t step;           /* Philox counter words 2, 3: the caller's step count */
  int32_t env_id_offset;   /* global id of row 0 (a shard of a larger batch); >= 0 */
  int32_t reserved1;       /* 0 */
  const float* scale;      /* device f32[A]: log_std (GAUSSIAN) or sigma (ACTION_NOISE); unused in UNIFORM */
  const float* shift;      /* device f32[A] or NULL (0): the action noise's mean */
  float noise_lo, noise_hi;/* ACTION_NOISE: the clip of a; UNIFORM: the range.  Not read in GAUSSIAN */
  float* noise;            /* device f32[E, A]: read (GIVEN), written when not NULL (DRAW) */
  float* actions;          /* device f32[E, A]: the action the buffer keeps */
  float* env_actions;      /* device f32[E, A] or NULL: the action the env steps on */
  float* log_prob;         /* device f32[E] or NULL; GAUSSIAN only */
  float* values;           /* device f32[E, width of head 1] or NULL: the critic's output */
  float* mean;             /* device f32[E, A] or NULL */
} FleetExploreArgs;
/* Enqueues on the policy's stream, no host synchronisation.  norm: as for fleet_policy_forward_dev (ignored in UNIFORM).
 * FLEET_ERR_INVALID (fleet_policy_last_error(h) says why, nothing is launched) for a wrong struct_bytes, an unknown mode or
 * noise_mode, E < 1, a null `actions`, a null obs or scale outside UNIFORM, log_prob outside GAUSSIAN, values on a one-head policy
 * or in UNIFORM, GIVEN with a null noise, a NaN bound or noise_lo > noise_hi (ACTION_NOISE, UNIFORM; GAUSSIAN does not read
 * the bounds and accepts any), a negative env_id_offset, a normaliser of another width or device. */
int fleet_explore_act_dev(fleet_policy_handle h, const float* obs, int E, fleet_norm_handle norm, const FleetExploreArgs* args);

/* ---- evaluation of the agent on the device (fleet_eval.hip; DESIGN.md "Evaluating the agent on the device") -----------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * stable-baselines3 2.3.2's EvalCallback as ONE enqueue-only call: sync_envs_normalization, evaluate_policy for n_eval_episodes
 * deterministic episodes, and "keep the best model" decided and carried out on the device.  The handle BORROWS the evaluation env
 * (auto_reset = 1), an optional evaluation normaliser (NULL: none) and a policy, which must outlive it, and owns one block, zeroed at
 * create: the observation buffer f32[E,D] and the raw-observation buffer f32[E,D] (one buffer without a normaliser), the actions
 * f32[E,A], the raw and the normalised reward f64[E] each, done u8[E], the running sums f64[E], the running lengths i32[E] and the
 * episode counts i32[E], the episode lists ep_reward f64[max_episodes] and ep_length i32[max_episodes], a u64 count of the episodes
 * listed, best_mean_reward f64 (which starts at -inf), a u64 count of the evaluations run, a u32 gate, and the snapshot: room for the
 * policy image's floats.
 * fleet_eval_sync_norm_dev(dst, src), ONE launch on dst's stream: obs_rms {mean, var, count} and ret_rms {mean, var, count} of src
 * into dst -- what sync_envs_normalization copies -- and what the steps derive from them, sd = sqrt(var + dst's epsilon), in the
 * arithmetic fleet_norm_set_state leaves behind.  dst's returns and settings stay.  The counts are the host's (functions of the
 * number of updates enqueued so far) and are copied there.  When src's last launch went to another stream, dst's stream is made to
 * wait for it by an event; src's next update on another stream waits for the copy.  FLEET_ERR_INVALID for a null handle, another D
 * or another device.
 * fleet_eval_run_dev only enqueues, in this order:
 *   1. with sync_from: the sync launch into the handle's normaliser
 *   2. the reset: fleet_reset_dev with no mask into the raw buffer, fleet_norm_reset_dev from it into the observation buffer (not
 *      without a normaliser), then one small launch that clears the sums, the lengths, the counts and the list's count
 *   3. for t = 0 .. n_steps-1: fleet_policy_forward_dev on the observation buffer (norm NULL: it holds normalised observations; no
 *      values), fleet_step_dev into the raw buffer, the raw reward and done (no terminal rows), fleet_norm_step_dev from them into the
 *      observation buffer and the normalised reward (not without a normaliser), the bookkeeping launch below
 *   4. the closing launch          5. the snapshot launch
 * 4 n_steps + 5 launches with a normaliser, 3 n_steps + 4 without, one more with sync_from (an entry of another family counts as one).
 * n_steps is the caller's: the device cannot end a host loop.  Outside real_time every episode of an env handle has episode_steps
 * steps, so SB3's loop ends after exactly ceil(n_eval_episodes / E) * episode_steps steps; steps after every quota is met change
 * nothing in the lists.
 * The bookkeeping launch (eval_episodes: ONE workgroup of 1024 threads, chunks of 1024 envs in env order, a ballot and a popcount per
 * wavefront, a prefix over the sixteen wavefront counts; no atomics) is evaluate_policy's inner loop.  Env i owes
 * target_i = (n_eval_episodes + i) / E episodes (integer division).  With r the reward the stack hands SB3 -- the normaliser's float64
 * output with a normaliser, (double)(float)raw reward without one:
 *   sums[i] += r;  lengths[i] += 1
 *   if counts[i] < target_i and done[i]:  list slot (listed + k) takes the episode;  counts[i] += 1;  sums[i] = 0;  lengths[i] = 0
 * k: the env's rank among this step's envs that satisfy the predicate, ascending env id; then listed += c, their number.  A slot at
 * or beyond max_episodes is not written (the run call cannot get there: the targets sum to n_eval_episodes <= max_episodes).
 * reward_source 0: the episode is (sums[i], lengths[i]) as they stand before they are zeroed -- what evaluate_policy sums on an env
 * without Monitor.  reward_source 1: the env is Monitor-wrapped (what make_vec_env gives), the episode is the env's
 * FLEET_F_LAST_EP_RETURN and FLEET_F_LAST_EP_LEN (raw rewards; Monitor's round(.., 6) is not applied).
 * The closing launch (eval_finish: one workgroup of 256 threads) writes stats f64[FLEET_EVAL_STATS]; with n = listed and S the
 * ordered float64 sum fleet_train_ppo_dev's section states (256 lane sums over positions t, t + 256, ... ascending, then the halving
 * tree s = 128 .. 1):
 *   [0] mean_reward = S(ep_reward) / n        [1] std_reward = sqrt(S((x - mean_reward)^2) / n), the population std (np.std)
 *   [2] mean_ep_length = S((double)ep_length) / n                [3] the lengths' std, the same way        [4] n
 *   [5] best_mean_reward after this call      [6] 1.0 if mean_reward > best_mean_reward held (SB3's test: false for NaN), else 0.0
 *   [7] (double)num_timesteps                 [8] evaluations run on this handle so far, this one included        [9..15] 0
 * [0] .. [3] are NaN when n == 0.  The launch writes the gate ([6] as a u32) and, when it is set, best_mean_reward = mean_reward.
 * The snapshot launch (eval_snapshot: a grid over the policy image's weights) copies them into the handle's snapshot iff the gate is
 * set: a call that does not improve leaves the snapshot's bits alone.  The gate is read on the device; the host does not look.
 * Everything refusable is refused before the first launch -- nothing is launched then -- in the words of the entry that would refuse.
 * A result depends on the handles' state and the arguments and on nothing else: not on the stream, not on max_episodes.  Env,
 * normaliser and policy must launch on ONE stream when a call is made; sync_from may launch elsewhere.  Calls are serialised by the
 * caller.  Out of scope: stochastic evaluation, real_time envs, callback_on_new_best, success rates. */
#define FLEET_EVAL_MAX_EPISODES 65536
#define FLEET_EVAL_STATS 16
typedef struct FleetEvalParams {
  int32_t struct_bytes;          /* sizeof(FleetEvalParams) */
  int32_t max_episodes;          /* 1..FLEET_EVAL_MAX_EPISODES: the lists' length, the largest n_eval_episodes */
} FleetEvalParams;
typedef struct FleetEvalArgs {
  int32_t struct_bytes;          /* sizeof(FleetEvalArgs) */
  int32_t n_eval_episodes;       /* 1..max_episodes */
  int32_t n_steps;               /* >= 1: env steps to take */
  int32_t reward_source;         /* 0: the sums of the step rewards; 1: the env's own episode records (Monitor) */
  fleet_norm_handle sync_from;   /* or NULL: the training normaliser whose statistics the evaluation normaliser takes first */
  uint64_t reserved;             /* 0 */
  uint64_t num_timesteps;        /* passed through to stats[7] */
  double* stats;                 /* device f64[FLEET_EVAL_STATS] */
} FleetEvalArgs;
typedef struct FleetEvalInfo {
  int32_t num_envs, obs_dim, act_dim;
  int32_t max_episodes;
  int32_t has_norm;              /* 1: a normaliser was given */
  int32_t launches;              /* launches the last fleet_eval_run_dev enqueued */
  uint64_t block_bytes;
  uint64_t snapshot_floats;      /* the policy image's size */
  float* obs;                    /* device f32[E,D] */
  float* raw_obs;                /* device f32[E,D]; obs itself without a normaliser */
  float* actions;                /* device f32[E,A] */
  double* raw_reward;            /* device f64[E] */
  double* reward;                /* device f64[E] */
  uint8_t* done;                 /* device u8[E] */
  double* sums;                  /* device f64[E] */
  int32_t* lengths;              /* device i32[E] */
  int32_t* counts;               /* device i32[E] */
  double* ep_reward;             /* device f64[max_episodes] */
  int32_t* ep_length;            /* device i32[max_episodes] */
  uint64_t* listed;              /* device u64 */
  double* best_mean_reward;      /* device f64 */
  uint64_t* evaluations;         /* device u64 */
  uint32_t* gate;                /* device u32 */
  float* snapshot;               /* device f32[snapshot_floats]: the image's layout; its record's bytes stay zero */
} FleetEvalInfo;
typedef struct FleetEval* fleet_eval_handle;

/* Everything is refused BEFORE the device is touched: FLEET_ERR_INVALID (fleet_eval_last_error(NULL) says why, starting with the
 * entry's name) for a null or wrongly sized FleetEvalParams, max_episodes outside 1..FLEET_EVAL_MAX_EPISODES, a null output, env or
 * policy, a handle that is no policy, an env without auto_reset, E, D, A or the device of env, normaliser and policy disagreeing.
 * FLEET_ERR_HIP with the byte count when the block cannot be allocated. */
int fleet_eval_create(fleet_handle env, fleet_norm_handle norm, fleet_policy_handle policy, const FleetEvalParams* p, fleet_eval_handle* out);
int fleet_eval_destroy(fleet_eval_handle h);
const char* fleet_eval_last_error(fleet_eval_handle h);  /* h may be NULL: error of the last failed call without a handle */
int fleet_eval_describe(fleet_eval_handle h, FleetEvalInfo* out);
int fleet_eval_sync_norm_dev(fleet_norm_handle dst, fleet_norm_handle src);
/* The arguments are looked at before the handle is: with h NULL the reason (or "null handle") goes to fleet_eval_last_error(NULL).
 * FLEET_ERR_INVALID for a null or wrongly sized args struct, n_eval_episodes < 1, n_steps < 1, a reward_source outside {0, 1}, a
 * reserved that is not 0, null stats, and -- these need the handle -- n_eval_episodes > max_episodes, handles that do not launch on
 * one stream, sync_from without a normaliser on the handle, a sync_from of another D or device. */
int fleet_eval_run_dev(fleet_eval_handle h, const FleetEvalArgs* a);
/* The bookkeeping launch on the caller's device arrays done u8[E], reward f64[E] (taken as it is), and for reward_source 1 ep_return
 * f64[E] and ep_len i32[E] (else they may be NULL), 1 <= E <= the handle's num_envs: the same kernel body behind another loader.  The
 * clearing launch on its own. */
int fleet_eval_episodes_dev(fleet_eval_handle h, const uint8_t* done, const double* reward, const double* ep_return, const int32_t* ep_len,
                            int E, int n_eval_episodes, int reward_source);
int fleet_eval_clear_dev(fleet_eval_handle h);
/* The snapshot into a policy of identical layout (dst may be the evaluated policy; it must launch on the env's stream), one launch;
 * and into `count` device tensors in torch's layout and order, the ones fleet_policy_load_dev reads, one launch.  FLEET_ERR_STATE
 * before the first fleet_eval_run_dev. */
int fleet_eval_best_load_dev(fleet_eval_handle h, fleet_policy_handle dst);
int fleet_eval_best_export_dev(fleet_eval_handle h, float* const* tensors, int count);
/* Synchronous: the lists and their count to HOST buffers ep_reward f64[max_episodes], ep_length i32[max_episodes], count u64 (any may
 * be NULL). */
int fleet_eval_episodes_read(fleet_eval_handle h, double* ep_reward, int32_t* ep_length, uint64_t* count);

/* ---- correlated action noise on the device (fleet_noise.hip; DESIGN.md "Correlated action noise on the device") -------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * A process that produces the eps rows f32[E, A] fleet_explore_act_dev reads with noise_mode GIVEN, one row per env and call, with
 * per-env episode resets (SB3's VectorizedActionNoise.reset(indices)).  Two kinds.
 * PINK: power-law ("colored") noise, the Timmer-Koenig generator as colorednoise.powerlaw_psd_gaussian(beta, n) evaluates it, which
 * pink.ColoredNoiseProcess / PinkActionNoise wrap (beta = 1): unit scale, the caller's sigma scales it.  Restated from the published
 * algorithm.  One sequence of n = seq_len samples belongs to (seed, global env id g = env_id_offset + e, column j, sequence number
 * q) and depends on nothing else: not on E, on the sharding, on the stream, on which other envs regenerate in the same call.  With
 * K = n/2 + 1, f_k = k/n (f_0 := f_1), s_k = f_k^(-beta/2), w = s[1:] with its last element times (1 + n mod 2)/2 and
 * sigma = 2 sqrt(sum w^2)/n, the host builds in float64 and rounds to float32 once
 *   gain[0] = sqrt(2) s_0/(n sigma), gain[k] = 2 s_k/(n sigma) for 0 < 2k < n, gain[n/2] = sqrt(2) s_{n/2}/(n sigma) for even n,
 *   twiddle[m] = (cos, sin)(2 pi m/n), m < n                                              (fleet_noise_pink_tables returns both)
 * and the device evaluates the inverse real transform as a direct sum, sample by sample, in float32:
 *   (a_k, b_k): Philox4x32-10 under key (seed lo, seed hi) at counter (g, 0x80000000 | (j/2), q, k); the Box-Muller of the
 *   exploration section on (x0, x1) gives (a_k, b_k) of column 2(j/2), on (x2, x3) of column 2(j/2)+1 (cosine: a, sine: b)
 *   ga = gain[k] * a_k;  gb = gain[k] * b_k, and gb = +0 for k = 0 and for 2k = n
 *   y[t]: acc = 0; for k = 0 .. K-1 ascending, m = (k t) mod n in integers:
 *           acc = fmaf(ga, cos[m], acc); acc = fmaf(-gb, sin[m], acc)
 * -- that chain bit for bit; no sinf / cosf in it, no FFT.  Bit 31 of counter word 1 keeps the draws apart from the exploration
 * epilogue's white noise (word 1 <= 127 there) and from OU's (bit 30) under one seed.  Var(y[t]) = sum of gain[k]^2 (slightly above
 * 1: the DC term), corr(y[t], y[t+d]) = sum gain[k]^2 cos(2 pi k d/n) / sum gain[k]^2.
 * State per env: t (int32, the position, 0..n) and q (uint32, the sequence number); the handle also keeps the current sequences of
 * every env, E * n * A float32 as [E][n][A] (157 MB at 4096 x 192 x 50).  create generates q = 0 for every env, t = 0.
 * fleet_noise_next_dev, one launch: an env with done[e] != 0 or t == n (the sequence is used up: the process's own wrap-around)
 * takes q += 1, t = 0 and regenerates its n x A samples -- only such envs do; then eps_out[e][:] = sequence[t][:] and t += 1.
 * A call in which many envs regenerate costs n^2/2 x 2 fused multiply-adds per column of each: with phase-locked episodes that is
 * one slow call per episode.
 * OU: SB3's OrnsteinUhlenbeckActionNoise per env, x <- x + theta (mu - x) dt + sigma sqrt(dt) eps, the output is x (it carries mu and
 * sigma: pass sigma = 1 to the exploration step).  Host tables in float64 rounded to float32: th = theta * dt, ss[j] = sigma[j] *
 * sqrt(dt), mu[j].  eps: the white normal of the exploration section at counter (g, 0x40000000 | (j/4), c lo, c hi), c = the number of
 * fleet_noise_next_dev calls before this one (uint64, kept by the handle).  Per element, float32:
 *   x0 = done[e] ? 0 : x;  d = mu[j] - x0;  u = fmaf(th, d, x0);  x = fmaf(ss[j], eps, u)
 * State: x f32[E, A] and the call count.  Reset zeroes x.
 * Every *_dev entry takes device pointers and enqueues on the handle's stream (its own, or the one fleet_noise_set_stream borrowed)
 * without waiting for it, except fleet_noise_set_state_dev of a PINK process, which reads the positions back to look at them.  Calls
 * on one handle are serialised by the caller.  No atomics. */
#define FLEET_NOISE_PINK 0
#define FLEET_NOISE_OU 1
#define FLEET_NOISE_MAX_ACT_DIM 512
#define FLEET_NOISE_MAX_SEQ_LEN 4096
typedef struct FleetNoiseParams {
  int32_t struct_bytes;   /* sizeof(FleetNoiseParams) */
  int32_t kind;           /* FLEET_NOISE_PINK / _OU */
  int32_t num_envs;       /* E >= 1 */
  int32_t act_dim;        /* A, 1..FLEET_NOISE_MAX_ACT_DIM */
  int32_t env_id_offset;  /* global id of row 0 (a shard of a larger batch); >= 0 */
  int32_t seq_len;        /* PINK: n, 2..FLEET_NOISE_MAX_SEQ_LEN (the episode's steps); ignored by OU */
  uint64_t seed;          /* Philox key */
  double beta;            /* PINK: the spectrum's exponent, finite and >= 0 (1: pink, 0: white, 2: red) */
  double theta, dt;       /* OU: finite, dt >= 0 (SB3's defaults: 0.15, 1e-2) */
  const double* mu;       /* OU: HOST array [A], finite; read by create and not kept (describe returns NULL) */
  const double* sigma;    /* OU: HOST array [A], finite */
  uint64_t cache_bytes;   /* out (fleet_noise_describe): bytes of the PINK sequences on the device, 0 for OU; ignored by create */
} FleetNoiseParams;
typedef struct FleetNoise* fleet_noise_handle;

/* The host tables of a PINK process, no device: gain f32[seq_len/2 + 1], twiddle f32[seq_len][2] (cos, sin).  FLEET_ERR_INVALID for
 * seq_len outside 2..4096, a negative or non-finite beta, a null output. */
int fleet_noise_pink_tables(int seq_len, double beta, float* gain, float* twiddle);
/* The parameters are validated BEFORE the device is touched: FLEET_ERR_INVALID (fleet_noise_last_error(NULL) says why, starting with
 * the entry's name) for a wrong struct_bytes, an unknown kind, num_envs < 1, act_dim outside 1..512, seq_len outside 2..4096, a
 * negative or non-finite beta, a negative env_id_offset, non-finite theta / dt / mu / sigma or dt < 0, null mu / sigma (OU), a cache of
 * more than 2^40 bytes.  FLEET_ERR_HIP with the byte count when the allocation fails.  The host waits for the first sequences. */
int fleet_noise_create(int device, const FleetNoiseParams* p, fleet_noise_handle* out);
int fleet_noise_destroy(fleet_noise_handle h);
const char* fleet_noise_last_error(fleet_noise_handle h);  /* h may be NULL: error of the last failed fleet_noise_create */
/* launch on an external hipStream_t (borrowed; NULL = the null stream) from now on; waits for what the previous stream still holds */
int fleet_noise_set_stream(fleet_noise_handle h, void* hip_stream);
/* eps_out f32[E, A] <- the next row of every env; done u8[E] or NULL (no env is done).  FLEET_ERR_INVALID for a null eps_out. */
int fleet_noise_next_dev(fleet_noise_handle h, const uint8_t* done, float* eps_out);
/* What fleet_noise_next_dev does to the envs with mask[e] != 0 (NULL: all) when they are done, and nothing else: PINK q += 1, t = 0
 * and new sequences; OU x = 0.  Nothing is emitted, the other envs and OU's call count stay. */
int fleet_noise_reset_dev(fleet_noise_handle h, const uint8_t* mask);
/* The state into / from device arrays: PINK t i32[E] and q u32[E] (x is not looked at), OU x f32[E, A] (t, q are not looked at); the
 * call count through the host (`calls` may be NULL in get).  set of a PINK process regenerates every env's sequences from q, and
 * refuses (FLEET_ERR_INVALID, nothing changes) a t outside 0..n after reading the positions back: it waits for the stream. */
int fleet_noise_get_state_dev(fleet_noise_handle h, int32_t* t, uint32_t* q, float* x, uint64_t* calls);
int fleet_noise_set_state_dev(fleet_noise_handle h, const int32_t* t, const uint32_t* q, const float* x, uint64_t calls);
/* the parameters the process was created with (mu, sigma NULL), and cache_bytes */
int fleet_noise_describe(fleet_noise_handle h, FleetNoiseParams* out);

/* ---- collect_rollouts on the device (fleet_collect.hip; DESIGN.md "Rollout collection on the device") -----------------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * stable-baselines3 2.3.2's OnPolicyAlgorithm.collect_rollouts (PPO) and OffPolicyAlgorithm.collect_rollouts (TD3 / DDPG) as ONE
 * enqueue-only call each: the loop over env steps that calls the families' own entries, as they are, and the one number of SB3's
 * rollout log that nothing else produces on the device -- rollout/ep_rew_mean and rollout/ep_len_mean over ep_info_buffer, the last
 * W = stats_window finished episodes in the order Monitor reports them.  The handle BORROWS an env (auto_reset = 1), an optional
 * normaliser (NULL: none) and a policy, which must outlive it, and owns one block, zeroed at create: two carry observation
 * buffers f32[E,D] and two raw-observation buffers f32[E,D] (none without a normaliser: the env writes the carry buffers), the raw
 * terminal rows f32[E,D], the raw and the normalised reward f64[E] each, two carry episode_start / done arrays u8[E], the env actions
 * f32[E,A], a noise row f32[E,A], last_values f32[E], and the episode ring: ring_return f64[W], ring_length i32[W], a u64 count of the
 * episodes appended so far and a u64 count of those appended since the last closing launch.  The carry buffers PING-PONG: a call reads
 * side `cur` and leaves what the next call starts from on the other side, so a rollout of one step copies nothing.
 * fleet_collect_reset_dev (SB3's _setup_learn): fleet_reset_dev with no mask into raw buffer 0, fleet_norm_reset_dev from it into
 * carry buffer 0 (without a normaliser the env writes carry buffer 0), cur = 0, episode_start = 1 for every env (one small launch);
 * the ring and its counts are cleared only when clear_episodes is not 0 (the closing launch then reports NaN means).
 * fleet_collect_ppo_dev fills all K = n_steps rows of the buffer.  Step t = 0 .. K-1, with cur = the carry for t = 0 and row t's own
 * obs / episode_start afterwards, next = row t+1's, or the other carry side when t = K-1:
 *   1. fleet_explore_act_dev GAUSSIAN, DRAW, norm NULL (the buffer holds normalised observations, as under SB3's VecNormalize), key
 *      (seed, env_id_offset, step = first_step + t); actions, log_prob and values are row t's own, env_actions the handle's
 *   2. fleet_step_dev into the raw buffer and the raw reward (straight into next.obs without a normaliser), done -> next.episode_start,
 *      no terminal rows
 *   3. fleet_norm_step_dev from them into next.obs and the normalised reward                          (not without a normaliser)
 *   4. fleet_rollout_add_dev(t, cur.obs, row t's actions, the reward as F64, cur.episode_start, row t's value and log_prob, NULL, NULL)
 *   5. the episode launch below
 * then fleet_policy_forward_dev on the carry for last_values, fleet_rollout_finish_dev(last_values, the carry's episode_start) and
 * the closing launch: 5 K + 3 launches with a normaliser, 4 K + 3 without.  SB3's time-limit bootstrap stays off (the reference
 * never sets TimeLimit.truncated).
 * fleet_collect_offpolicy_dev takes n_steps env steps.  Global step s = first_step + t:
 *   1. s < learning_starts: fleet_explore_act_dev UNIFORM DRAW; else with a noise handle fleet_noise_next_dev(noise, the carry's
 *      done, the noise row) and ACTION_NOISE GIVEN, without one ACTION_NOISE DRAW -- on the carry observation, norm NULL (the actor
 *      reads normalised observations), key (seed, env_id_offset, step = s), actions = env_actions = the handle's
 *   2. fleet_step_dev into the other raw buffer, the raw reward and the other done array, with the raw terminal rows
 *   3. fleet_norm_step_dev from the raw buffer into the other carry buffer (terminal rows are not normalised: nobody reads them)
 *   4. fleet_replay_add_dev(raw cur, raw next, the actions, the raw reward as F64, done, the raw terminal rows, NULL): the replay
 *      buffer stores raw observations, as SB3 does
 *   5. the episode launch; the sides swap
 * then the closing launch: 4 per step and 1, one more per step with a normaliser, one more per step that asks the noise handle.
 * The episode launch (collect_episodes: ONE workgroup of 1024 threads, chunks of 1024 envs, a ballot-and-popcount scan in env order;
 * no atomics).  With count the ring's running total and c the step's number of finished envs, the k-th of them (k = 0 .. c-1,
 * ascending env id) writes its last episode's return and length -- what info["episode"] carries: FLEET_F_LAST_EP_RETURN and
 * FLEET_F_LAST_EP_LEN -- to slot (count + k) % W iff c - k <= W: only the last W of a step survive, so no two lanes write one slot.
 * Then count += c.  This is SB3's _update_info_buffer: a deque(maxlen = W) extended over infos in env order.
 * The closing launch (collect_finish: one workgroup of 256 threads) writes stats f64[FLEET_COLLECT_STATS]; with n = min(count, W):
 *   [0] ep_rew_mean = S(ring_return[s], s = 0 .. n-1) / n      [1] ep_len_mean = S((double)ring_length[s], s = 0 .. n-1) / n
 *   [2] the episodes appended since the previous closing launch (of a run call: those of the call)     [3] count
 *   [4] (double)(first_step + steps)      [5..15] 0
 * S is the ordered float64 sum fleet_train_ppo_dev's section states: 256 lane sums over positions t, t + 256, ... ascending, then the
 * halving tree s = 128 .. 1.  [0] and [1] are NaN when n == 0 (SB3 logs nothing then).
 * Both run calls only enqueue (they may block on the queue's depth, never on the device) on the stream the borrowed handles launch
 * on when the call is made: env, normaliser, policy, buffer and noise handle must launch on ONE stream then.  Everything refusable
 * is refused before the first launch -- nothing is launched then, no counter moves -- in the words of the entry that would refuse.
 * A result depends on (the handles' state, seed, first_step) and on nothing else.  Out of scope: the time-limit bootstrap, gSDE,
 * SAC, train_freq in episodes, callbacks.  Calls are serialised by the caller. */
#define FLEET_COLLECT_MAX_WINDOW 4096
#define FLEET_COLLECT_STATS 16
typedef struct FleetCollectParams {
  int32_t struct_bytes;          /* sizeof(FleetCollectParams) */
  int32_t stats_window;          /* W, 1..FLEET_COLLECT_MAX_WINDOW (SB3's stats_window_size: 100) */
} FleetCollectParams;
typedef struct FleetCollectPpoArgs {
  int32_t struct_bytes;          /* sizeof(FleetCollectPpoArgs) */
  int32_t n_steps;               /* K: must be the buffer's */
  int32_t env_id_offset;         /* the noise's global id of env 0; >= 0 */
  int32_t reserved;              /* 0 */
  fleet_rollout_handle buffer;   /* E, D, A as the handle's; launches on the env's stream */
  const float* log_std;          /* device f32[A] */
  uint64_t seed;                 /* Philox key of the exploration noise */
  uint64_t first_step;           /* the noise counter: env steps taken before this call */
  double* stats;                 /* device f64[FLEET_COLLECT_STATS] */
} FleetCollectPpoArgs;
typedef struct FleetCollectOffpolicyArgs {
  int32_t struct_bytes;          /* sizeof(FleetCollectOffpolicyArgs) */
  int32_t n_steps;               /* >= 1 */
  int32_t env_id_offset;         /* >= 0 */
  int32_t reserved;              /* 0 */
  uint64_t learning_starts;      /* global steps below it draw uniform actions */
  fleet_replay_handle replay;    /* E, D, A as the handle's */
  const float* sigma;            /* device f32[A] */
  const float* shift;            /* device f32[A] or NULL (0) */
  float noise_lo, noise_hi;      /* the action space: noise_lo <= noise_hi */
  fleet_noise_handle noise;      /* or NULL: white noise drawn by the exploration launch */
  uint64_t seed;
  uint64_t first_step;           /* env steps taken before this call */
  double* stats;                 /* device f64[FLEET_COLLECT_STATS] */
} FleetCollectOffpolicyArgs;
typedef struct FleetCollectInfo {
  int32_t num_envs, obs_dim, act_dim;
  int32_t stats_window;
  int32_t has_norm;              /* 1: a normaliser was given */
  int32_t cur;                   /* the side the next call starts from */
  int32_t launches;              /* kernel launches the last run call (or reset) enqueued */
  int32_t reserved;
  uint64_t block_bytes;
  float* carry_obs[2];           /* device f32[E,D]; [cur]: what the next call's first step reads */
  float* raw_obs[2];             /* device f32[E,D]; the carry buffers themselves without a normaliser */
  uint8_t* carry_start[2];       /* device u8[E] */
  float* raw_terminal;           /* device f32[E,D] */
  double* raw_reward;            /* device f64[E] */
  double* reward;                /* device f64[E] */
  float* env_actions;            /* device f32[E,A] */
  float* last_values;            /* device f32[E] */
  double* ring_return;           /* device f64[W] */
  int32_t* ring_length;          /* device i32[W] */
  uint64_t* ring_count;          /* device u64[2]: appended so far, appended since the last closing launch */
} FleetCollectInfo;
typedef struct FleetCollect* fleet_collect_handle;

/* Everything is refused BEFORE the device is touched: FLEET_ERR_INVALID (fleet_collect_last_error(NULL) says why, starting with the
 * entry's name) for a null or wrongly sized FleetCollectParams, stats_window outside 1..FLEET_COLLECT_MAX_WINDOW, a null output, env
 * or policy, a handle that is no policy, an env without auto_reset, a critic head wider than 1, E, D, A or the device of env,
 * normaliser and policy disagreeing (A: the env's EVs against the actor's output width).  FLEET_ERR_HIP with the byte count when the
 * block cannot be allocated. */
int fleet_collect_create(fleet_handle env, fleet_norm_handle norm, fleet_policy_handle policy, const FleetCollectParams* p,
                         fleet_collect_handle* out);
int fleet_collect_destroy(fleet_collect_handle h);
const char* fleet_collect_last_error(fleet_collect_handle h);  /* h may be NULL: error of the last failed call without a handle */
int fleet_collect_describe(fleet_collect_handle h, FleetCollectInfo* out);
/* Two launches and the small one with a normaliser, one and the small one without.  FLEET_ERR_INVALID when env and normaliser do not
 * launch on one stream. */
int fleet_collect_reset_dev(fleet_collect_handle h, int clear_episodes);
/* The arguments are looked at before the handle is: with h NULL the reason (or "null handle") goes to fleet_collect_last_error(NULL).
 * FLEET_ERR_INVALID for a null or wrongly sized args struct, n_steps < 1, a reserved that is not 0, a negative env_id_offset, a null
 * buffer / replay, log_std / sigma or stats, noise_lo > noise_hi or a NaN bound, and -- these need the handle -- a one-head policy
 * (PPO), n_steps that is not the buffer's, a buffer or a noise handle whose E, D or A differ from the handle's or that lies on
 * another device, handles that do not launch on one stream. */
int fleet_collect_ppo_dev(fleet_collect_handle h, const FleetCollectPpoArgs* a);
int fleet_collect_offpolicy_dev(fleet_collect_handle h, const FleetCollectOffpolicyArgs* a);
/* The episode launch on the caller's device arrays done u8[E], ep_return f64[E], ep_len i32[E] (E: any, >= 1) instead of the env's
 * records: the same kernel body behind another loader.  The closing launch on its own: stats as above with steps = `steps`. */
int fleet_collect_episodes_dev(fleet_collect_handle h, const uint8_t* done, const double* ep_return, const int32_t* ep_len, int E);
int fleet_collect_finish_dev(fleet_collect_handle h, uint64_t first_step, int32_t steps, double* stats);
/* Synchronous: the ring and its count to HOST buffers ring_return f64[W], ring_length i32[W], count u64 (any may be NULL).  The last
 * n = min(count, W) episodes, oldest first, lie in slots (count - n + i) % W, i = 0 .. n-1. */
int fleet_collect_episodes_read(fleet_collect_handle h, double* ring_return, int32_t* ring_length, uint64_t* count);

/* ---- TD3 / DDPG learning targets on the device (fleet_qtarget.hip; DESIGN.md "Learning targets on the device") --------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * The TARGET networks of an off-policy actor-critic agent -- one target actor and n_critics target Q networks (2: TD3; 1: DDPG, with
 * sigma = 0) -- which torch never differentiates, and the two things a gradient step does with them: the bootstrap target of a
 * minibatch in ONE launch, and the Polyak update from the online networks' parameters in ONE launch.  float32 throughout.
 * Networks.  The actor is a FleetPolicyHead over D = obs_dim inputs, its output width is A.  Critic c is a FleetPolicyHead over D + A
 * inputs -- the observation, then the action: SB3's ContinuousCritic, cat([features, actions], 1) -- with output width 1 and output
 * transform NONE.  The policy's limits hold: 1..FLEET_POLICY_MAX_LAYERS layers, widths 1..FLEET_POLICY_MAX_WIDTH (so A <= 512),
 * D + A <= FLEET_POLICY_MAX_OBS_DIM.  The weights are re-laid at upload as the policy's are (Wt[in4][out64], zero padding).
 * The target, per row b of the minibatch (what fleet_replay_sample_dev wrote: next_obs f32[B,D] already normalised, rewards f32[B],
 * dones f32[B]), every step in float32 and exactly so:
 *   d[j]  = the actor head's output, its output transform applied (TANH for TD3)
 *   n[j]  = sigma[j] * eps[b][j], clipped to [-noise_clip, +noise_clip]               (x < lo ? lo : (x > hi ? hi : x), here and below)
 *   a'[j] = d[j] + n[j], clipped to [act_lo, act_hi]
 *   q_c   = critic c over concat(next_obs[b], a'): the policy section's chain, acc = 0; fmaf in ascending k over the D + A inputs; + bias
 *   qmin  = n_critics == 2 ? (q_1 < q_0 ? q_1 : q_0) : q_0
 *   t     = (1.0f - dones[b]) * gamma;  y[b] = rewards[b] + t * qmin          (the product and the sum are rounded one by one: no fma)
 * Every output of a row is a function of that row: not of B, of the row's place in the batch, of the stream, of which optional
 * outputs are asked for; next_actions and q[:, 0] do not depend on n_critics.  One workgroup takes 16 rows through the actor, then
 * through critic 0, then through critic 1: no atomics, no ordering between workgroups.
 * Noise.  eps follows the counter scheme of fleet_explore_act_dev, unchanged: Philox4x32-10 under key (seed lo, seed hi) at counter
 * (row_offset + b, j / 4, step lo, step hi), Box-Muller as there; noise_mode FLEET_EXPLORE_NOISE_DRAW or _GIVEN as there, and DRAW
 * with a non-null `noise` records the draw.  A caller who also explores with fleet_explore_act_dev gives the target a SEED OF ITS OWN:
 * under one seed, row b of a minibatch at gradient step s would repeat the exploration noise of env b at env step s.
 * The Polyak update.  Every real element t of the padded image, with p the online network's element, becomes
 *   t' = fmaf(tau32, p, t * omt32),  tau32 = (float)tau,  omt32 = (float)(1.0 - tau)
 * -- SB3's polyak_update, target.mul_(1 - tau); torch.add(target, param, alpha=tau), with the scaled addition fused into one
 * rounding.  The padding is not touched and stays zero.  tau = 0 leaves t, tau = 1 gives p bit for bit (but a p of -0 comes out +0
 * unless t is negative, IEEE's sum of zeros; and a t that is not finite stays NaN: t * 0).
 * Every *_dev call takes device pointers, only enqueues (no host synchronisation) and runs on the handle's stream: its own, or the one
 * fleet_qtarget_set_stream borrowed.  Calls on one handle are serialised by the caller. */
typedef struct FleetQTargetParams {
  int32_t struct_bytes;       /* sizeof(FleetQTargetParams) */
  int32_t obs_dim;            /* D >= 1 */
  int32_t n_critics;          /* 1 or 2 */
  int32_t tile_rows;          /* out (fleet_qtarget_describe): minibatch rows one workgroup takes through every network; ignored by create */
  FleetPolicyHead actor;      /* over D inputs; the last width is A */
  FleetPolicyHead critic[2];  /* over D + A inputs; the last width must be 1, the output FLEET_POLICY_OUT_NONE */
} FleetQTargetParams;
typedef struct FleetQTargetArgs {
  int32_t struct_bytes;   /* sizeof(FleetQTargetArgs) */
  int32_t noise_mode;     /* FLEET_EXPLORE_NOISE_DRAW / _GIVEN */
  uint64_t seed;          /* Philox key */
  uint64_t step;          /* Philox counter words 2, 3: the caller's gradient-step count */
  int32_t row_offset;     /* global id of row 0 (a shard of a larger minibatch); >= 0 */
  int32_t reserved;       /* 0 */
  float gamma;            /* the discount */
  float noise_clip;       /* >= 0; +inf: no clip */
  float act_lo, act_hi;   /* the action space: act_lo <= act_hi */
  const float* sigma;     /* device f32[A]: the target-policy smoothing noise's scale (0: DDPG) */
  float* noise;           /* device f32[B, A] or NULL: read (GIVEN), written when not NULL (DRAW) */
  float* target_q;        /* device f32[B]: y */
  float* next_actions;    /* device f32[B, A] or NULL: a' */
  float* q;               /* device f32[B, n_critics] or NULL: q_c */
} FleetQTargetArgs;
typedef struct FleetQTarget* fleet_qtarget_handle;

/* The parameters and the weights are validated BEFORE the device is touched: FLEET_ERR_INVALID (fleet_qtarget_last_error(NULL) says
 * why) for a wrong struct_bytes, obs_dim < 1, n_critics outside 1..2, a layer count outside 1..4, a width outside 1..512, D + A above
 * 8192, a critic whose last width is not 1 or whose output is not NONE, an unknown activation or output transform, lo > hi or a NaN
 * bound of a CLIP actor, a null pointer, a weight that is not finite.
 * host_weights: packed float32 -- the actor, then critic 0, then critic 1; for each layer W[out, in] (row-major) then b[out]. */
int fleet_qtarget_create(int device, const FleetQTargetParams* p, const float* host_weights, fleet_qtarget_handle* out);
int fleet_qtarget_destroy(fleet_qtarget_handle h);
const char* fleet_qtarget_last_error(fleet_qtarget_handle h);  /* h may be NULL: error of the last failed call without a handle */
/* launch on an external hipStream_t (borrowed; NULL = the null stream) from now on; waits for what the previous stream still holds */
int fleet_qtarget_set_stream(fleet_qtarget_handle h, void* hip_stream);
/* New weights from HOST memory, packed as for create; FLEET_ERR_INVALID (nothing changes) when one is not finite.  The host waits. */
int fleet_qtarget_load_host(fleet_qtarget_handle h, const float* weights);
/* `tensors`: a host array of `count` device pointers, torch's parameter tensors in the order of host_weights (W, b per layer; count
 * must be twice the number of layers of all networks).  load: one launch copies and re-lays them (a hard update, and how the targets
 * start as copies of the online networks).  polyak: `tensors` are the ONLINE networks' parameters; one launch, the update above;
 * FLEET_ERR_INVALID for a tau outside [0, 1] or NaN.  export: the inverse re-lay, the target weights out into torch-layout tensors
 * (checkpoints; tests that read an update's result).  The values are not inspected. */
int fleet_qtarget_load_dev(fleet_qtarget_handle h, const float* const* tensors, int count);
int fleet_qtarget_polyak_dev(fleet_qtarget_handle h, const float* const* tensors, int count, double tau);
int fleet_qtarget_export_dev(fleet_qtarget_handle h, float* const* tensors, int count);
/* One launch: the targets of B rows.  FLEET_ERR_INVALID (nothing is launched) for a null or wrongly sized FleetQTargetArgs, an unknown
 * noise_mode, B < 1, a null next_obs / rewards / dones / sigma / target_q, a NaN bound or act_lo > act_hi, a noise_clip that is
 * negative or NaN, GIVEN with a null noise, a negative row_offset.  The arguments are looked at before the handle is: with h NULL
 * the reason (or "null handle") goes to fleet_qtarget_last_error(NULL), so the checks can be exercised without a device. */
int fleet_qtarget_target_dev(fleet_qtarget_handle h, const float* next_obs, const float* rewards, const float* dones, int B,
                             const FleetQTargetArgs* args);
/* the parameters the handle was created with, and tile_rows */
int fleet_qtarget_describe(fleet_qtarget_handle h, FleetQTargetParams* out);

/* ---- TD3 / DDPG's whole update on the device (fleet_offpolicy.hip; DESIGN.md "TD3's whole update on the device") -------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * stable-baselines3 2.3.2's TD3.train(gradient_steps, batch_size) -- and DDPG's: n_critics = 1, policy_delay = 1, sigma zeros -- as ONE
 * enqueue-only call.  The handle BORROWS five handles, which must outlive it: a replay buffer, the TARGET networks' fleet_qtarget handle,
 * and -- all three on ONE second fleet_qtarget handle that holds the ONLINE networks -- a fleet_td3 gradient handle, a fleet_adam handle
 * over the actor (span 0, 1, no extras) and one over the critics (span 1, n_critics, no extras).  It owns one block, zeroed at create:
 * the staging arrays of max_batch rows (the gradient handle's) and max_steps slots of per-step statistics.
 * Gradient step g = 0 .. gradient_steps - 1 of a call, with u = first_update + g, through the families' own entries, as they are (their
 * sections state their arithmetic):
 *   1. fleet_replay_sample_dev(replay, batch_size, norm, the staging arrays): the buffer's own call counter is used, which so advances by
 *      gradient_steps per call
 *   2. fleet_qtarget_target_dev on the TARGET networks from the staged next_obs, rewards and dones into the staged target_q; noise_mode
 *      DRAW (not recorded), key (seed, row_offset 0, step = u)
 *   3. fleet_td3_critic_grad_dev on the staged obs, actions and target_q; stats -> slot g, floats 0..7
 *   4. fleet_adam_step_dev(adam_critic, lr, beta1[1], beta2[1], eps[1], max_grad_norm[1])
 *   5. iff (u + 1) % policy_delay == 0 (SB3 increments _n_updates before it tests):
 *      fleet_td3_actor_grad_dev on the staged obs; stats -> slot g, floats 8..15
 *      fleet_adam_step_dev(adam_actor, lr, beta1[0], beta2[0], eps[0], max_grad_norm[0])
 *      the image-to-image Polyak update below with tau
 * FIVE launches on a plain step, NINE on a delayed one (SB3's TD3 does not clip: with a max_grad_norm > 0 each optimiser step is two),
 * and one closing launch per call.  The result is bit-equal to the same entries called one by one.  Every argument is stateless:
 * first_update is the number of gradient steps taken so far (SB3's _n_updates), the only thing a checkpoint adds to the five handles'.
 * The fleet_adam handle keeps no hyperparameters, so both optimisers' travel in the arguments.
 * The image-to-image Polyak update.  Since the optimisers write every new weight to torch's parameter AND to the online image with the
 * same bits, the targets' image is updated from the online IMAGE: both have one layout, so this is one contiguous stream over the floats
 * behind the two records, with no pointer array and no transposition,
 *   t' = fmaf(tau32, p, t * omt32),  tau32 = (float)tau,  omt32 = (float)(1.0 - tau)
 * -- fleet_qtarget_polyak_dev's expression: the same bits whenever the online image holds torch's parameters.  The launch walks the zero
 * padding too, which stays +0: fmaf(tau32, +0, +0 * omt32) = +0 for tau in [0, 1].  A caller who changed torch's parameters without
 * fleet_qtarget_load_dev on the ONLINE handle has let the two diverge: the update follows the image, and the divergence is the caller's.
 * The statistics block, stats f64[FLEET_TRAIN_STATS], written by the closing launch (one workgroup of 256 threads) with the ordered
 * float64 sum S of "PPO's whole update on the device" (256 lane sums over positions t, t + 256, ... ascending, then the halving tree
 * s = 128 .. 1) over the call's slots, G = gradient_steps:
 *   [0] critic_loss  [1] critic_0_loss  [2] critic_1_loss (0 with one critic): S((double)slot[g][k], g = 0 .. G - 1) / (double)G, k = 0, 1, 2
 *   [3] actor_loss: S((double)slot[g_j][8], j = 0 .. n - 1) / (double)n over the call's n actor steps g_0 < g_1 < ..., position j of the
 *       sum being the j-th of them; NaN when n == 0 (SB3 logs train/actor_loss only when there was one)
 *   [4] the LAST step's critic_loss  [5] the last actor step's actor_loss, or NaN  [6] (double)(first_update + G) (train/n_updates)
 *   [7] n, the actor steps of the call  [8..15] 0
 * Which slots hold an actor step follows from (first_update, G, policy_delay) in the launch's arguments, not from a flag in memory:
 *   g_0 = (policy_delay - (first_update % policy_delay + 1) % policy_delay) % policy_delay;  g_j = g_0 + j * policy_delay
 * Every *_dev call takes device pointers, only enqueues (it may block on the queue's depth, it never waits for the device) and launches
 * on the stream the borrowed handles launch on when the call is made: the replay buffer, the target networks and the online networks
 * must launch on ONE stream then (streams are not ordered with events here).  No atomics, no ordering between workgroups.  Calls are
 * serialised by the caller. */
#define FLEET_OFFPOLICY_MAX_STEPS 65536
#define FLEET_OFFPOLICY_SLOT_FLOATS 16
typedef struct FleetOffpolicyParams {
  int32_t struct_bytes;          /* sizeof(FleetOffpolicyParams) */
  int32_t max_steps;             /* 1..FLEET_OFFPOLICY_MAX_STEPS: gradient steps one call may take */
} FleetOffpolicyParams;
typedef struct FleetOffpolicyArgs {
  int32_t struct_bytes;          /* sizeof(FleetOffpolicyArgs) */
  int32_t gradient_steps;        /* 1..max_steps */
  int32_t batch_size;            /* 1..max_batch */
  int32_t policy_delay;          /* >= 1 */
  int32_t reserved;              /* 0 */
  float gamma;                   /* the discount, as fleet_qtarget_target_dev takes it */
  double tau;                    /* in [0, 1], as fleet_qtarget_polyak_dev takes it */
  float noise_clip;              /* >= 0; +inf: no clip */
  float act_lo, act_hi;          /* the action space: act_lo <= act_hi */
  const float* sigma;            /* device f32[A]: the target-policy smoothing noise's scale (zeros: DDPG) */
  double lr;                     /* finite, >= 0; both optimisers', constant within the call */
  double beta1[2], beta2[2];     /* in [0, 1); [0] the actor optimiser's, [1] the critic optimiser's, here and below */
  double eps[2];                 /* finite, >= 0 */
  double max_grad_norm[2];       /* <= 0: no clipping (SB3's TD3) */
  uint64_t seed;                 /* Philox key of the target-policy smoothing noise */
  uint64_t first_update;         /* gradient steps taken before this call */
  fleet_norm_handle norm;        /* or NULL: the minibatches are sampled raw */
  double* stats;                 /* device f64[FLEET_TRAIN_STATS] */
} FleetOffpolicyArgs;
typedef struct FleetOffpolicyInfo {
  int32_t obs_dim, act_dim, n_critics;   /* the networks' D, A and critics */
  int32_t max_batch;             /* the gradient handle's: rows the staging arrays hold */
  int32_t max_steps;             /* slots */
  int32_t n_actor_tensors;       /* the counts the update takes: W, b per layer of the actor ... */
  int32_t n_critic_tensors;      /* ... and of the critics, critic after critic */
  int32_t reserved;
  uint64_t staging_bytes;        /* of the staging arrays */
  void* staging;                 /* device: obs [max_batch, D], actions [max_batch, A], next_obs [max_batch, D], dones, rewards, target_q
                                    [max_batch], each at the next multiple of 256 bytes; the LAST step's rows (tests) */
  void* slots;                   /* device f32[max_steps][FLEET_OFFPOLICY_SLOT_FLOATS] behind them: the last call's per-step stats */
} FleetOffpolicyInfo;
typedef struct FleetOffpolicy* fleet_offpolicy_handle;

/* FLEET_ERR_INVALID (fleet_offpolicy_last_error(NULL) says why, starting with the entry's name) for a null or wrongly sized
 * FleetOffpolicyParams, max_steps out of range, a null output or handle, a target handle that is no fleet_qtarget handle, online and
 * target networks that are one handle, whose records differ in any byte (shapes, activations, output transform and bounds) or that lie on
 * different devices, an optimiser on another image than the gradient handle, an actor optimiser whose span is not (0, 1, no extras), a
 * critic optimiser whose span is not (1, n_critics, no extras), a replay buffer on another device or whose D or A differs from the
 * networks'.  FLEET_ERR_HIP with the byte count when the block cannot be allocated.  (grad: a fleet_td3_handle, the optimisers:
 * fleet_adam_handles; their sections follow this one, so the struct tags stand here.) */
struct FleetTd3;
struct FleetAdam;
int fleet_offpolicy_create(fleet_replay_handle replay, fleet_qtarget_handle targets, struct FleetTd3* grad, struct FleetAdam* adam_actor,
                           struct FleetAdam* adam_critic, const FleetOffpolicyParams* p, fleet_offpolicy_handle* out);
int fleet_offpolicy_destroy(fleet_offpolicy_handle h);
const char* fleet_offpolicy_last_error(fleet_offpolicy_handle h);  /* h may be NULL: error of the last failed call without a handle */
int fleet_offpolicy_describe(fleet_offpolicy_handle h, FleetOffpolicyInfo* out);
/* The update.  actor_params / actor_grads: host arrays of n_actor device pointers as fleet_adam_step_dev takes them (W, b per layer of
 * the actor); critic_params / critic_grads: the critics', critic after critic.  The parameters are stepped in place (and the online image
 * with them); the gradient tensors hold the last step's gradients.  Everything that can be refused is refused before the first launch:
 * nothing is launched then, and the replay buffer's call counter and both step counts stay.  FLEET_ERR_INVALID for a null or wrongly
 * sized FleetOffpolicyArgs, gradient_steps < 1, batch_size < 1, policy_delay < 1, a reserved that is not 0, a null stats, whatever
 * fleet_qtarget_target_dev, fleet_qtarget_polyak_dev, fleet_td3_*_grad_dev and fleet_adam_step_dev refuse (in their words), and -- these
 * need the handle -- gradient_steps above max_steps, batch_size above max_batch, wrong tensor counts, a norm whose obs_dim is not D, a
 * replay buffer, target networks and online networks that do not launch on one stream; FLEET_ERR_STATE for an empty buffer.  The
 * arguments are looked at before the handle is: with h NULL the reason (or "null handle") goes to fleet_offpolicy_last_error(NULL). */
int fleet_offpolicy_td3_dev(fleet_offpolicy_handle h, const FleetOffpolicyArgs* a, float* const* actor_params, float* const* actor_grads,
                            int n_actor, float* const* critic_params, float* const* critic_grads, int n_critic);
/* The image-to-image Polyak update on its own, one launch: the targets' image <- the online image.  FLEET_ERR_INVALID for a tau outside
 * [0, 1] or NaN, and when the two handles do not launch on one stream. */
int fleet_offpolicy_polyak_dev(fleet_offpolicy_handle h, double tau);

/* ---- PPO's whole update on the device (fleet_train.hip; DESIGN.md "PPO's whole update on the device") ------------------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * stable-baselines3 2.3.2's PPO.train() with clip_range_vf = None and target_kl = None as ONE enqueue-only call: n_epochs passes over a
 * finished rollout buffer (fleet_rollout_finish_dev has run) in freshly shuffled minibatches of batch_size rows, the short last one
 * when n % batch_size != 0 included, as SB3's get() yields them; n = E * K; a batch_size above n means one minibatch of n rows.  Per
 * minibatch FIVE launches on the policy's stream: the minibatch launch below, fleet_ppo_grad_dev's two, fleet_adam_step_dev's two --
 * those four through their own entries, as they are (their sections state their arithmetic), on the staged rows, with the call's
 * clip_range, vf_coef, ent_coef, lr, betas, eps and max_grad_norm; Adam's step count advances once per minibatch.  log_std is the LAST
 * tensor of params / grads: updated in place, read by the next gradient launch.  One closing launch per call writes the statistics.
 * The handle BORROWS a rollout buffer, a fleet_ppo handle and a fleet_adam handle, which must outlive it, and owns the staging block.
 * The shuffle.  perm(n, seed, epoch, p) is a keyed bijection of [0, n), evaluated per position, nothing materialised:
 *   h = the smallest h >= FLEET_TRAIN_MIN_HALF_BITS with 2^(2h) >= n;  mask = 2^h - 1;  x = p
 *   repeat:  L = x >> h;  R = x & mask
 *            for r = 0 .. FLEET_TRAIN_ROUNDS - 1:
 *              F = word 0 of philox4x32_10(counter (R, r, epoch_lo, epoch_hi); key (seed_lo, seed_hi)) & mask;  (L, R) = (R, L ^ F)
 *            x = (L << h) | R
 *   until x < n;  perm = x        (cycle walking: a bijection of [0, 2^(2h)) walked from a point below n returns below n)
 * Epoch e of a call shuffles with epoch = first_epoch + e: a caller that counts its epochs never repeats a shuffle, and a checkpoint
 * needs that count only.  Position start + b of the epoch is row b of the minibatch at `start`; i = perm(...) is the flat index
 * e_env * K + t of fleet_rollout_gather_dev.
 * The minibatch launch gathers obs, actions, old log-probabilities, advantages and returns of its B rows into the staging block (rows
 * of obs / actions as 16-byte words when D / A is a multiple of 4; old values are gathered by fleet_train_ppo_vclip_dev alone, below) and, when
 * normalize_advantage != 0 and B > 1, writes a second advantage array, which the gradient launches then read:
 *   ordered sum S(x) of B values in minibatch order, float64: lane t of 256: s_t = 0.0; s_t = s_t + x[b] for b = t, t + 256, ... ascending;
 *     then for s = 128, 64, ..., 1: s_t = s_t + s_(t + s) for t < s; the result is s_0
 *   mean64 = S((double)adv) / (double)B;  std64 = sqrt(S(((double)adv - mean64)^2) / (double)(B - 1))     (the unbiased one)
 *   mean32 = (float)mean64;  std32 = (float)std64;  advn[b] = (adv[b] - mean32) / (std32 + 1e-8f)           (float32, SB3's expression)
 * The bits depend on the B values in minibatch order alone: not on the grid, the stream, max_batch or the run.  With B == 1 or
 * normalize_advantage == 0 the raw advantages are used (SB3 makes the same exception for one row).
 * The statistics block, stats f64[FLEET_TRAIN_STATS], written by the closing launch:
 *   [0] policy_loss [1] value_loss [2] entropy_loss [3] approx_kl [4] clip_fraction: the float64 mean over ALL minibatches of all epochs
 *       of the gradient launches' float32 statistic, in the order they ran: acc = 0.0; acc = acc + (double)stat; acc / (double)count
 *       -- what SB3 logs as train/policy_gradient_loss, train/value_loss, train/entropy_loss, train/approx_kl, train/clip_fraction
 *       ([3] averages over ALL epochs; SB3 clears its approx_kl list at the start of every epoch, so what it logs as train/approx_kl
 *       is the LAST epoch's mean: slot [13] of fleet_train_ppo_kl_dev, below, carries that one)
 *   [5] loss: the LAST minibatch's (train/loss)        [6] count: the number of minibatches
 *   [7] explained_variance = 1 - vd / vy over the whole buffer, y = (double)returns, d = y - (double)values, time-major order
 *       (x[t * E + e]), float64 with the ordered sum S over the n values: my = S(y) / n;  md = S(d) / n;
 *       vy = S((y - my)^2) / n;  vd = S((d - md)^2) / n;  NaN when vy == 0, as SB3's helper returns
 *   [8] std = S(exp((double)log_std[j])) / A after the last step (train/std)        [9..15] 0
 * Every *_dev call takes device pointers, only enqueues (it may block on the queue's depth, it never waits for the device) and launches
 * on the POLICY's stream, whichever that is when the call is made; the rollout buffer must launch on that same stream then (streams
 * are not ordered with events here).  No atomics, no ordering between workgroups.  Calls are serialised by the caller. */
#define FLEET_TRAIN_ROUNDS 8
#define FLEET_TRAIN_MIN_HALF_BITS 4
#define FLEET_TRAIN_STATS 16
typedef struct FleetTrainPpoArgs {
  int32_t struct_bytes;          /* sizeof(FleetTrainPpoArgs) */
  int32_t n_epochs;              /* >= 1 */
  int32_t batch_size;            /* >= 1; min(batch_size, n) <= the gradient handle's max_batch */
  int32_t normalize_advantage;   /* 0: off */
  float clip_range;              /* in (0, 1) */
  float vf_coef, ent_coef;       /* not NaN */
  int32_t reserved;              /* 0 */
  double lr;                     /* finite, >= 0; constant within the call */
  double beta1, beta2;           /* in [0, 1) */
  double eps;                    /* finite, >= 0 */
  double max_grad_norm;          /* <= 0: no clipping */
  uint64_t seed;                 /* the shuffle's key */
  uint64_t first_epoch;          /* epoch e of the call shuffles with first_epoch + e */
  double* stats;                 /* device f64[FLEET_TRAIN_STATS] */
} FleetTrainPpoArgs;
typedef struct FleetTrainInfo {
  int32_t num_envs, n_steps, obs_dim, act_dim;   /* the rollout buffer's E, K, D, A */
  int32_t max_batch;             /* the gradient handle's: rows the staging block holds */
  int32_t n_tensors;             /* the `count` the update takes: the policy's tensors + 1 */
  int32_t rounds, min_half_bits; /* of the shuffle */
  int32_t tile_rows;             /* rows per tile of the minibatch launch (4) */
  int32_t cache_rows;            /* positions of a minibatch whose buffer rows the launch keeps in the LDS (2048) */
  uint64_t staging_bytes;        /* of the staging arrays */
  void* staging;                 /* device: obs [max_batch, D], actions [max_batch, A], old_log_prob, advantages, normalised advantages,
                                    returns [max_batch], each at the next multiple of 256 bytes; the LAST minibatch's rows (tests) */
} FleetTrainInfo;
typedef struct FleetTrain* fleet_train_handle;

/* FLEET_ERR_INVALID (fleet_train_last_error(NULL) says why, starting with the entry's name) for a null handle or output, a gradient
 * handle and an optimiser on different policies, a rollout buffer on another device or whose D or A differs from the policy's, an
 * optimiser whose span is not both heads plus one extra of length A.  FLEET_ERR_HIP with the byte count when the staging block cannot
 * be allocated.  (grad: a fleet_ppo_handle, adam: a fleet_adam_handle; their sections follow this one, so the struct tags stand here.) */
struct FleetPpo;
struct FleetAdam;
int fleet_train_create(fleet_rollout_handle buffer, struct FleetPpo* grad, struct FleetAdam* adam, fleet_train_handle* out);
int fleet_train_destroy(fleet_train_handle h);
const char* fleet_train_last_error(fleet_train_handle h);  /* h may be NULL: error of the last failed call without a handle */
int fleet_train_describe(fleet_train_handle h, FleetTrainInfo* out);
/* The update.  params, grads: host arrays of `count` device pointers as fleet_adam_step_dev takes them (W, b per layer, head 0 then head
 * 1, then log_std).  FLEET_ERR_INVALID (nothing is launched, the step count stays) for a null or wrongly sized FleetTrainPpoArgs,
 * n_epochs < 1, batch_size < 1, a reserved that is not 0, a null stats, whatever fleet_ppo_grad_dev and fleet_adam_step_dev refuse (in
 * their words), and -- these need the handle -- a count that is not the policy's tensors + 1, a minibatch above max_batch, a rollout
 * buffer that launches on another stream than the policy.  The arguments are looked at before the handle is: with h NULL the reason
 * (or "null handle") goes to fleet_train_last_error(NULL). */
int fleet_train_ppo_dev(fleet_train_handle h, const FleetTrainPpoArgs* a, float* const* params, float* const* grads, int count);
/* The shuffle on its own, one launch: out[k] = perm(n, seed, epoch, start + k) for k < count, int32 in device memory; any n in
 * 1 .. 2^31 - 1.  FLEET_ERR_INVALID for n < 1, positions outside [0, n), a null out. */
int fleet_train_indices_dev(fleet_train_handle h, int32_t n, uint64_t seed, uint64_t epoch, int32_t start, int32_t count, int32_t* out);
/* -- the update with value-function clipping (clip_range_vf; DESIGN.md "PPO's value clipping on the device") --
 * (entries added under FLEET_ABI_VERSION 11 on the existing handle: fleet_train_ppo_dev, FleetTrainPpoArgs and FleetTrainInfo are as
 * they were)  fleet_train_ppo_dev with SB3's clip_range_vf = cv > 0: still five launches per minibatch.  The minibatch launch also
 * gathers the buffer's values of its rows (lane 0, with the row's other scalars) into one more staging array, f32[max_batch], which
 * lies BEHIND the existing parts of the block -- staging_bytes, the stats and the running sums keep their places --, and the gradient
 * step goes through fleet_ppo_grad_vclip_dev (the PPO gradients' section states the arithmetic).  The statistics block keeps its
 * layout; [1] and [5] carry the clipped value loss.  FLEET_ERR_INVALID for a null or wrongly sized FleetTrainPpoVclipArgs, whatever
 * fleet_train_ppo_dev refuses of `base` (in its words), a clip_range_vf that is not finite and > 0. */
typedef struct FleetTrainPpoVclipArgs {
  int32_t struct_bytes;          /* sizeof(FleetTrainPpoVclipArgs) */
  float clip_range_vf;           /* cv: finite, > 0 */
  FleetTrainPpoArgs base;        /* everything fleet_train_ppo_dev takes; base.struct_bytes = sizeof(FleetTrainPpoArgs) */
} FleetTrainPpoVclipArgs;
extern int fleet_train_ppo_vclip_dev(fleet_train_handle h, const FleetTrainPpoVclipArgs* a, float* const* params, float* const* grads,
                                     int count);
/* *old_values_offset: the bytes from FleetTrainInfo.staging to the staged old values f32[max_batch] (the LAST value-clipped
 * minibatch's rows; tests).  FLEET_ERR_INVALID for a null handle or output. */
extern int fleet_train_describe_vclip(fleet_train_handle h, uint64_t* old_values_offset);
/* -- the update with early stopping on approx_kl (target_kl; DESIGN.md "PPO's early stopping on the device") --
 * (an entry added under FLEET_ABI_VERSION 11 on the existing handle: everything above is as it was)  SB3 2.3.2's PPO.train() with
 * target_kl set, still ONE enqueue-only call and still five launches per scheduled minibatch.  thr = 1.5 * target_kl, formed once in
 * double on the host.  Per minibatch, in the order fleet_train_ppo_dev runs them: the minibatch launch, the two gradient launches (they
 * write the minibatch's statistics), then:  if (double)approx_kl > thr -- approx_kl the float32 stats[4] of the gradient launches; a NaN
 * does NOT stop, as in SB3 -- the update STOPS: this minibatch's optimiser step is not taken and no later launch of the call does any
 * work; otherwise the two Adam launches run.  The arithmetic of every minibatch that runs is fleet_train_ppo_dev's (clip_range_vf 0) or
 * fleet_train_ppo_vclip_dev's, bit for bit; a target_kl that never triggers gives their weights, moments, step count and stats [0..8].
 * The stopping minibatch's statistics DO count in the means (SB3 appends them before its break).
 * One difference from SB3: after a stop the gradient tensors (`.grad`) hold the STOPPING minibatch's gradients -- the gradient launches
 * had run when the decision fell; they were never applied.  SB3 does not call backward() for that minibatch.
 * The device decides, with launch boundaries only and no atomics: gated instances of the six kernels (the ungated ones are the code
 * they were) and a control record in the handle's block, behind the staged old values (every earlier offset stays).  NO launch reads
 * a word that a workgroup of the SAME launch may write:
 *   decided  written by the statistics workgroup of a minibatch's second gradient launch: (double)approx_kl > thr.  Read only by
 *            LATER launches: that minibatch's two Adam launches (set: they return at their top and write nothing -- no parameter, no
 *            moment, no image word, no norm) and every workgroup of the NEXT minibatch launch (set: no gather).
 *   stopped  read and written by thread 0 of workgroup 0 of the minibatch launch alone: when it is clear, the previous minibatch's
 *            statistics go into the running float64 sums, as in fleet_train_ppo_dev, and the device's counters are bumped (minibatches
 *            run; optimiser steps taken: only when decided is clear; epochs entered; the last epoch's approx_kl sum); then stopped =
 *            decided.  Read by LATER launches: both gradient launches return at their top when it is set.
 *   The call's first launch clears the record.  The closing launch folds the last minibatch that ran, unless that was done, and divides
 *   by the DEVICE's count.  After a stop every remaining launch of the call reads one word (a uniform load, a scalar branch) and returns.
 * The optimiser's step count.  The host's scheduled t = (count before the call) + 1 + k is right for every step that runs, since nothing
 * runs after a skip: the bias corrections stay host-formed in double.  The count AFTER the call is the device's to say: the call ends
 * with fleet_adam_settle_dev (the optimiser's section), a 4-byte copy to pinned host memory and an event.  The call is therefore
 * enqueue-only but NOT capturable into a graph: FLEET_ERR_STATE, nothing launched, when the policy's stream is capturing.
 * The statistics block keeps its 16 doubles; this entry defines:
 *   [0..4] the means over the minibatches that RAN, the stopping one included, in the order they ran (the same ordered float64 sum)
 *   [5] loss of the last minibatch that ran     [6] minibatches that ran     [7], [8] as above ([8]: after the last step TAKEN)
 *   [9] optimiser steps taken     [10] epochs entered (what SB3 adds to _n_updates)     [11] 1.0 if the update stopped early, else 0.0
 *   [12] approx_kl of the last minibatch that ran: the value that was compared
 *   [13] the mean of approx_kl over the minibatches of the LAST epoch entered (acc = 0.0; acc = acc + (double)stat in order; acc / their
 *        number): what SB3 logs as train/approx_kl          [14], [15] 0
 * FLEET_ERR_INVALID for a null or wrongly sized FleetTrainPpoKlArgs, whatever fleet_train_ppo_dev refuses of `base` (in its words), a
 * target_kl that is not finite and > 0, a clip_range_vf that is negative or not finite. */
typedef struct FleetTrainPpoKlArgs {
  int32_t struct_bytes;          /* sizeof(FleetTrainPpoKlArgs) */
  float clip_range_vf;           /* 0: no value clipping; otherwise cv of fleet_train_ppo_vclip_dev: finite, > 0 */
  double target_kl;              /* finite, > 0 */
  FleetTrainPpoArgs base;        /* everything fleet_train_ppo_dev takes; base.struct_bytes = sizeof(FleetTrainPpoArgs) */
} FleetTrainPpoKlArgs;
FLEET_API int fleet_train_ppo_kl_dev(fleet_train_handle h, const FleetTrainPpoKlArgs* a, float* const* params, float* const* grads,
                                     int count);

/* ---- Adam and clip_grad_norm_ on the device (fleet_adam.hip; DESIGN.md "The optimiser step on the device") -------------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * What a gradient step does behind the gradients -- torch.nn.utils.clip_grad_norm_(params, max_grad_norm), torch.optim.Adam.step() and
 * the *_load_dev that copied the new weights into the weight image -- in TWO launches.  The optimiser is created ON a weight image (of a
 * fleet_policy or a fleet_qtarget handle, which it BORROWS and which must outlive it) and owns nets first_net .. first_net + n_nets - 1
 * of it, W then b per layer, net after net, and behind them n_extra flat tensors that are in no image (PPO's log_std).  Spans: both
 * heads of a policy (0, 2); the actor of a TD3 image (0, 1); its critics (1, n_critics); n_nets = 0 with one extra is a plain flat
 * Adam.  Two optimisers with disjoint spans on one image are allowed.  Every new weight p' goes to torch's own parameter tensor and,
 * for a tensor of the span, to the image element Wt[k][j] / b[j]: the same bits in both, so no *_load_dev follows a step.  The image's
 * zero padding is not touched.  The gradients are READ ONLY: the clipped gradient is used and NOT written back.
 * No weight decay, no amsgrad, no maximize (SB3's defaults use none).  No atomics, no random numbers; every sum in the order below.
 * The arithmetic, float32 but where stated, no fused contraction but the fmaf written here, sqrtf and / correctly rounded.
 * The host forms in double, as torch's Python does, with t = the handle's step count + 1, and rounds to float:
 *   omb1 = 1 - beta1;  omb2 = 1 - beta2;  b2 = beta2;  nstep = -(lr / (1 - beta1^t));  bs = sqrt(1 - beta2^t);  eps;  maxn32 = max_grad_norm
 * The norm runs iff max_grad_norm > 0 or norm_out is not NULL.  A chunk is 1024 consecutive elements of ONE gradient tensor (a tensor's
 * last chunk is short; a chunk never straddles two tensors); chunks are numbered tensor after tensor, ascending inside a tensor.
 *   thread t of 256: acc = 0; acc = fmaf(g, g, acc) over elements 4t .. 4t + 3 of the chunk in ascending order, those past the end skipped
 *   wavefront w (threads 64w .. 64w + 63): for off = 32, 16, 8, 4, 2, 1: acc = acc + (the acc of lane ^ off)
 *   part[chunk] = ((wave 0 + wave 1) + wave 2) + wave 3
 *   norm = (float)sqrt(the float64 sum of (double)part[chunk] in ascending chunk order)
 * The bits depend on the gradients alone: not on a tensor's alignment, on the grid, on the stream or on which workgroup summed.
 * The clip, as clip_grad_norm_ does it (error_if_nonfinite = False):
 *   q = maxn32 / (norm + 1e-6f);  c = q > 1.0f ? 1.0f : q   (torch.clamp(q, max = 1): a NaN stays NaN, and then every g' is NaN)
 *   g' = g * c   (applied even when c == 1; not applied at all, g' = g, when max_grad_norm <= 0)
 * The update, per element (m: exp_avg, v: exp_avg_sq):
 *   m' = fmaf(g' - m, omb1, m)
 *   v' = fmaf(g' * omb2, g', v * b2)
 *   den = sqrtf(v') / bs + eps
 *   p' = fmaf(m' / den, nstep, p)
 * -- torch's single-tensor Adam (lerp, mul + addcmul, sqrt / bias_correction2_sqrt + eps, addcdiv with value -step_size), each fused
 * where one torch kernel rounds once.  This is NOT bit-equal to torch's float32 CPU Adam, whose vectorised kernels differ from their
 * own scalar arithmetic by an ulp here and there; the bits are pinned to the lines above.
 * The state (m, v per tensor in torch's layout, zero at create; the step count on the host, 0 at create, as torch's non-capturable Adam
 * keeps it) goes into and out of torch.optim.Adam.state_dict() unchanged through fleet_adam_state_dev.
 * Every *_dev call takes device pointers, only enqueues, and launches on the IMAGE handle's stream, whichever that is when the call is
 * made: a forward enqueued behind a step on that handle sees the new weights with no host wait.  Calls are serialised by the caller. */
#define FLEET_ADAM_MAX_EXTRA 2
#define FLEET_ADAM_STATE_EXPORT 0
#define FLEET_ADAM_STATE_LOAD 1
typedef struct FleetAdamParams {
  int32_t struct_bytes;                      /* sizeof(FleetAdamParams) */
  int32_t first_net;                         /* first net of the span in the image (policy: 0 actor head, 1 critic head; TD3: 0 actor, 1.. critics) */
  int32_t n_nets;                            /* nets in the span, 0 .. the image's */
  int32_t n_extra;                           /* flat tensors behind the span, 0..FLEET_ADAM_MAX_EXTRA */
  int32_t extra_len[FLEET_ADAM_MAX_EXTRA];   /* their lengths, 1..2^24 */
} FleetAdamParams;
typedef struct FleetAdamStepArgs {
  int32_t struct_bytes;   /* sizeof(FleetAdamStepArgs) */
  double lr;              /* finite, >= 0; per call: SB3 sets it anew every iteration */
  double beta1, beta2;    /* in [0, 1) */
  double eps;             /* finite, >= 0 */
  double max_grad_norm;   /* <= 0: no clipping */
  float* norm_out;        /* device f32[1] or NULL: the norm BEFORE clipping, what clip_grad_norm_ returns */
} FleetAdamStepArgs;
typedef struct FleetAdamInfo {
  uint64_t state_bytes;   /* of exp_avg and exp_avg_sq together */
  uint64_t n_elements;    /* of all tensors */
  int64_t step;           /* steps taken (or loaded) */
  int32_t n_tensors;      /* the span's, then the extras */
  int32_t norm_chunk;     /* elements per chunk of the norm launch (1024) */
  int32_t step_tile;      /* edge of a W tile of the step launch (32) */
  int32_t reserved;
} FleetAdamInfo;
typedef struct FleetAdam* fleet_adam_handle;

/* FLEET_ERR_INVALID (fleet_adam_last_error(NULL) says why, starting with the entry's name), before the device is touched, for a null or
 * wrongly sized FleetAdamParams, a negative first_net or n_nets, n_extra outside 0..2, an extra_len outside 1..2^24, nothing to
 * optimise, a null output or image handle, a handle of the other family, a span that ends behind the image's last net.  FLEET_ERR_HIP
 * with the byte count when the state cannot be allocated. */
int fleet_adam_create_policy(fleet_policy_handle policy, const FleetAdamParams* p, fleet_adam_handle* out);
int fleet_adam_create_qtarget(fleet_qtarget_handle nets, const FleetAdamParams* p, fleet_adam_handle* out);
int fleet_adam_destroy(fleet_adam_handle h);
const char* fleet_adam_last_error(fleet_adam_handle h);  /* h may be NULL: error of the last failed call without a handle */
/* the parameters the handle was created with, and what FleetAdamInfo lists */
int fleet_adam_describe(fleet_adam_handle h, FleetAdamParams* out, FleetAdamInfo* info);
/* One step, two launches (one when the norm does not run), enqueued only; adds one to the step count.  params, grads: host arrays of
 * `count` device pointers, contiguous float32 tensors in torch's [out, in] layout, the span's (W, b per layer, net after net) then the
 * extras; params are read and written in place, grads are read.  FLEET_ERR_INVALID (nothing is launched, the step count stays) for a
 * null or wrongly sized FleetAdamStepArgs, an lr or eps that is negative or not finite, a beta outside [0, 1), a NaN max_grad_norm, a
 * null array or a null pointer in one, a params[i] that is its own grads[i], and -- this one needs the handle -- a count that is not
 * the number of the handle's tensors.  The arguments are looked at before the handle is: with h NULL the reason (or "null handle")
 * goes to fleet_adam_last_error(NULL). */
int fleet_adam_step_dev(fleet_adam_handle h, const FleetAdamStepArgs* a, float* const* params, float* const* grads, int count);
/* mode FLEET_ADAM_STATE_EXPORT: the state out into `count` pairs of tensors in torch's layout, and the step count into *step (at once:
 * it lives on the host).  FLEET_ADAM_STATE_LOAD: the reverse; a negative *step is refused.  Copies on the image handle's stream. */
int fleet_adam_state_dev(fleet_adam_handle h, int mode, float* const* exp_avg, float* const* exp_avg_sq, int count, int64_t* step);
/* The WHOLE image the handle was created on (every net of it, not the span alone) out into `count` torch-layout tensors, W then b per
 * layer, net after net: the inverse re-lay of *_load_dev in one launch on the image handle's stream.  What a test reads a step's
 * result from, and the only way to read a policy's image back.  FLEET_ERR_INVALID for a null array or pointer, a wrong count. */
int fleet_adam_export_image_dev(fleet_adam_handle h, float* const* tensors, int count);
/* -- a step the device may skip, and a step count settled after the fact (DESIGN.md "PPO's early stopping on the device") --
 * (entries added under FLEET_ABI_VERSION 11 on the existing handle: the entries above are as they were)
 * fleet_adam_step_gated_dev is fleet_adam_step_dev plus a device word, skip u32[1], read when the launches run: nonzero means that both
 * launches return at their top -- a gated instance of each kernel, one uniform load and a scalar branch; the ungated ones are the code
 * they were -- and write NOTHING: no parameter, no moment, no image word, no partial sum, no norm_out.  An EARLIER launch must have
 * written the word.  With the word clear the step is fleet_adam_step_dev's, bit for bit.  The host's step count advances by one either
 * way, as scheduled: a caller that lets the device skip steps says afterwards how many ran, with fleet_adam_settle_dev.
 * FLEET_ERR_INVALID for whatever fleet_adam_step_dev refuses (in its words) and a null skip.
 * fleet_adam_settle_dev(h, base_step, steps_taken): the step count becomes base_step + *steps_taken, steps_taken a device u32[1] read
 * BEHIND everything enqueued on the image handle's stream so far: the entry enqueues a 4-byte copy into pinned host memory that the
 * handle owns and records an event; it does not wait, and no kernel writes host memory.  Settling on use: every entry that reads or
 * writes the step count -- fleet_adam_step_dev, fleet_adam_step_gated_dev, fleet_adam_state_dev, fleet_adam_describe, this one --
 * first waits for a pending settlement's event and fixes the count.  In a training loop a whole rollout lies between two updates and
 * the wait costs nothing; a caller that asks for the count right away gets the right one at the price of that wait.  An event wait
 * cannot be captured: FLEET_ERR_STATE when the stream is capturing a graph.  FLEET_ERR_INVALID for a negative base_step, a null word. */
FLEET_API int fleet_adam_step_gated_dev(fleet_adam_handle h, const FleetAdamStepArgs* a, float* const* params, float* const* grads,
                                        int count, const uint32_t* skip);
FLEET_API int fleet_adam_settle_dev(fleet_adam_handle h, int64_t base_step, const uint32_t* steps_taken);

/* ---- TD3 / DDPG minibatch gradients on the device (fleet_td3.hip; DESIGN.md "TD3's minibatch gradients on the device") -------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * What stable-baselines3 2.3.2's TD3.train does with one minibatch between the target and the optimisers, in two entries of TWO
 * launches each: the critic loss sum_c mse_loss(Q_c(obs, actions), y) with its backward, and -- on a delayed step -- the actor loss
 * -mean(Q_0(obs, pi(obs))) with its backward into the actor.  The networks are the ONLINE ones: the handle BORROWS the weight image of a
 * fleet_qtarget handle created from the online actor and critics (a second one beside the targets'), which the caller refreshes with
 * fleet_qtarget_load_dev after every optimiser step and which must outlive this handle.  float32 throughout, no fused contraction but
 * the fmaf written below, no atomics, no random numbers.  invB = 1.0f / (float)B.
 * The critic entry, per row b (obs f32[B,D] and actions f32[B,A] as fleet_replay_sample_dev wrote them, y = target_q f32[B] as
 * fleet_qtarget_target_dev wrote it), for every critic c, exactly:
 *   q_c  = critic c over concat(obs[b], actions[b]): the learning targets' chain (acc = 0; fmaf in ascending k over D + A; + bias)
 *   e_c  = q_c - y[b];  dq_c = (2.0f * invB) * e_c        (the delta of the critic's last layer)
 * The actor entry, per row b (obs f32[B,D]), exactly:
 *   mean[j] = the actor's last layer BEFORE its output transform;  a[j] = the transform of mean[j] (x < lo ? lo : (x > hi ? hi : x), tanhf)
 *   q    = critic 0 over concat(obs[b], a);  dq = -invB;  back through critic 0's layers to its first layer's delta d0
 *   da[j] = (acc = 0; acc = fmaf(Wt0[D + j][i], d0[i], acc) for i ascending over layer 0's outputs)      (no activation factor)
 *   dmean[j] = da[j] * g:  g = fmaf(-a, a, 1.0f) (TANH);  g = (mean >= lo && mean <= hi) ? 1 : 0 (CLIP: torch's clamp, the bounds
 *   inclusive);  g = 1 (NONE)                              (the delta of the actor's last layer)
 * No critic gradient is produced by the actor entry (SB3 discards it there too), and critic 1 is not run.
 * Back through layer l into layer l - 1 (h: that layer's activation), in both entries:
 *   d_prev[k] = (acc = 0; acc = fmaf(Wt[k][j], d[j], acc) for j ascending over the layer's outputs) * act'(h[k]),
 *   tanh' = fmaf(-h, h, 1.0f), relu' = h > 0 ? 1 : 0
 * Gradients, each element one chain over the rows in ascending b:
 *   dW[j][k]: acc = 0; acc = fmaf(d[b][j], x[b][k], acc);  db[j]: acc = 0; acc += d[b][j]
 *   x: the layer's input; for a critic's first layer column k is obs[b][k] for k < D and actions[b][k - D] behind it
 * Statistics, stats f32[8].  A tile is 16 consecutive rows; a tile's partial is the COMPENSATED sum of its rows' terms in ascending
 * order (Neumaier: s = 0, c = 0; per term x: t = s + x; c += |s| >= |x| ? (s - t) + x : (x - t) + s; s = t; the result is s + c), a
 * total the compensated sum of the tiles' partials in ascending order:
 *   critic entry: [1] = total(e_0 * e_0) * invB;  [2] = total(e_1 * e_1) * invB, 0 with one critic;  [0] = [1] + [2];  [3..7] 0
 *   actor entry:  [0] = -(total(q) * invB);  [1..7] 0
 * Every result is a function of the inputs and B only: not of the stream, of max_batch, of what lies behind row B in the buffers, of
 * which optional outputs are asked for, or of the run.  The gradient tensors and stats are OVERWRITTEN, not accumulated.  The per-row
 * outputs (q, actions_out) depend on their row alone: an observation that is not finite stays in its row there; it does reach the
 * gradients and the statistics, which sum over the rows.  The handle owns a scratch sized for max_batch rows (every layer's
 * activations and deltas).  It launches on the NETWORKS handle's stream, whichever that is when the call is made: a call enqueued behind
 * fleet_qtarget_load_dev on that handle sees the new weights with no host wait.  Calls are serialised by the caller. */
typedef struct FleetTd3Params {
  int32_t struct_bytes;  /* sizeof(FleetTd3Params) */
  int32_t max_batch;     /* rows the scratch holds, 1..2^24 */
} FleetTd3Params;
typedef struct FleetTd3CriticArgs {
  int32_t struct_bytes;    /* sizeof(FleetTd3CriticArgs) */
  int32_t B;               /* rows, 1..max_batch */
  const float* obs;        /* device f32[B, D] (normalised, as the replay buffer samples them) */
  const float* actions;    /* device f32[B, A] */
  const float* target_q;   /* device f32[B]: y */
  float* q;                /* device f32[B, n_critics] or NULL: q_c */
  float* stats;            /* device f32[8] */
  uint64_t reserved;       /* 0 */
} FleetTd3CriticArgs;
typedef struct FleetTd3ActorArgs {
  int32_t struct_bytes;    /* sizeof(FleetTd3ActorArgs) */
  int32_t B;               /* rows, 1..max_batch */
  const float* obs;        /* device f32[B, D] */
  float* actions_out;      /* device f32[B, A] or NULL: a */
  float* q;                /* device f32[B] or NULL: q */
  float* stats;            /* device f32[8] */
  uint64_t reserved;       /* 0 */
} FleetTd3ActorArgs;
typedef struct FleetTd3* fleet_td3_handle;

/* FLEET_ERR_INVALID (fleet_td3_last_error(NULL) says why, starting with the entry's name) for a null or wrongly sized FleetTd3Params,
 * max_batch outside 1..2^24, a null output or networks handle.  FLEET_ERR_HIP with the byte count when the scratch cannot be allocated. */
int fleet_td3_create(fleet_qtarget_handle nets, const FleetTd3Params* p, fleet_td3_handle* out);
int fleet_td3_destroy(fleet_td3_handle h);
const char* fleet_td3_last_error(fleet_td3_handle h);  /* h may be NULL: error of the last failed call without a handle */
/* the parameters the handle was created with, the bytes of its scratch, and the rows one workgroup of a rows launch takes */
int fleet_td3_describe(fleet_td3_handle h, FleetTd3Params* out, uint64_t* scratch_bytes, int32_t* tile_rows);
/* Two launches each, enqueued only.  grads: a host array of `count` device pointers, the gradient tensors in torch's [out, in] layout,
 * W then b per layer: critic 0's then critic 1's for the critic entry (count = the critics' tensors), the actor's for the actor entry.
 * FLEET_ERR_INVALID (nothing is launched) for a null or wrongly sized argument struct, B < 1, a null obs / actions / target_q / stats
 * (critic) or obs / stats (actor), a reserved that is not 0, a null grads or a null pointer in it, and -- these two need the handle --
 * a count that is not the entry's number of tensors, B > max_batch.  The arguments are looked at before the handle is: with h NULL the
 * reason (or "null handle") goes to fleet_td3_last_error(NULL). */
int fleet_td3_critic_grad_dev(fleet_td3_handle h, const FleetTd3CriticArgs* a, float* const* grads, int count);
int fleet_td3_actor_grad_dev(fleet_td3_handle h, const FleetTd3ActorArgs* a, float* const* grads, int count);

/* ---- PPO minibatch gradients on the device (fleet_ppo.hip; DESIGN.md "PPO's minibatch gradients on the device") --------------------
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays)
 * What stable-baselines3 2.3.2's PPO.train does with one minibatch before the optimiser -- evaluate_actions, the clipped loss
 * (clip_range_vf = None) and loss.backward() -- in TWO launches on a two-head policy's weight image (actor = head 0 with a
 * state-independent log_std, critic = head 1 of width 1 and output NONE):
 *   loss = -mean(min(adv * ratio, adv * clamp(ratio, 1 - c, 1 + c))) + vf_coef * mean((returns - v)^2) - ent_coef * mean(entropy)
 * and its gradient with respect to every weight and bias of both heads and to log_std.  float32 throughout, no fused contraction but
 * the fmaf written below, no atomics, no random numbers.  Per row b of the B rows (obs f32[B,D], actions f32[B,A], old_log_prob,
 * advantages, returns f32[B], as fleet_rollout_gather_dev writes them), exactly:
 *   mean[j], v = the policy section's forward chain; mean is head 0's last layer BEFORE its output transform
 *   sd = expf(ls[j]);  dm = a[j] - mean[j];  t[j] = -(dm * dm) / (2.0f * sd * sd) - ls[j] - 0.9189385332f        (ls = log_std)
 *   lp = the t[j] summed as fleet_explore_act_dev sums them: lane i of 64 adds j = i, i + 64, ... in ascending order to 0, then
 *        the xor butterfly s += shuffle_xor(s, 1), 2, 4, ..., 32 -- the same bits as the log_prob that launch stored
 *   lr = lp - old;  ratio = expf(lr);  lo = 1.0f - c;  hi = 1.0f + c;  cl = ratio < lo ? lo : (ratio > hi ? hi : ratio)
 *   s1 = adv * ratio;  s2 = adv * cl;  the row's policy term is -(s1 < s2 ? s1 : s2)
 *   alive = (ratio >= lo && ratio <= hi) || s1 < s2          (what torch's min / clamp backward rules, ties included, collapse to)
 *   invB = 1.0f / (float)B;  glp = alive ? -(adv * ratio) * invB : 0
 *   dmean[j] = glp * (dm / (sd * sd));  the row's log_std term u[j] = glp * ((dm * dm) / (sd * sd) - 1.0f)
 *   dv = ((2.0f * vf_coef) * invB) * (v - ret)
 * Back through layer l into layer l - 1 (h: that layer's activation):
 *   d_prev[k] = (acc = 0; acc = fmaf(Wt[k][j], d[j], acc) for j ascending over the layer's outputs) * act'(h[k]),
 *   tanh' = fmaf(-h, h, 1.0f), relu' = h > 0 ? 1 : 0
 * Gradients, each element one chain over the rows in ascending b:
 *   dW[j][k]: acc = 0; acc = fmaf(d[b][j], x[b][k], acc)  (x: the layer's input, obs for a first layer);  db[j]: acc = 0; acc += d[b][j]
 *   dlog_std[j]: acc = 0; acc += u[b][j];  then acc - ent_coef   (the entropy of the Gaussian is sum_j(1.4189385332f + ls[j]))
 * Statistics, stats f32[8].  A tile is 16 consecutive rows; a tile's partial is the COMPENSATED sum of its rows' terms in ascending
 * order (Neumaier: s = 0, c = 0; per term x: t = s + x; c += |s| >= |x| ? (s - t) + x : (x - t) + s; s = t; the result is s + c), a
 * total the compensated sum of the tiles' partials in ascending order:
 *   [0] policy_loss = total(policy term) * invB        [1] value_loss = total((ret - v) * (ret - v)) * invB
 *   [2] entropy_loss = -(ascending sum over j of (1.4189385332f + ls[j]))
 *   [3] loss = (policy_loss + ent_coef * entropy_loss) + vf_coef * value_loss
 *   [4] approx_kl = total((ratio - 1.0f) - lr) * invB   [5] clip_fraction = total(fabsf(ratio - 1.0f) > c ? 1 : 0) * invB   [6], [7] 0
 * Every result is a function of the inputs and B only: not of the stream, of max_batch, of what lies behind row B in the buffers,
 * or of the run.  The gradient tensors and stats are OVERWRITTEN, not accumulated.  values[b] and log_prob[b] depend on row b
 * alone: an observation that is not finite stays in its row there; it does reach the gradients and the statistics, which sum over
 * the rows.  The handle owns a scratch sized for max_batch rows (every layer's activations and deltas) and BORROWS the policy's
 * image: the policy must outlive it.  It launches on the POLICY's stream, whichever that is when the call is made: a call enqueued
 * behind fleet_policy_load_dev sees the new weights with no host wait.  Calls are serialised by the caller. */
typedef struct FleetPpoParams {
  int32_t struct_bytes;  /* sizeof(FleetPpoParams) */
  int32_t max_batch;     /* rows the scratch holds, 1..2^24 */
} FleetPpoParams;
typedef struct FleetPpoGradArgs {
  int32_t struct_bytes;        /* sizeof(FleetPpoGradArgs) */
  int32_t B;                   /* rows, 1..max_batch */
  const float* obs;            /* device f32[B, D] (normalised, as the rollout buffer keeps them) */
  const float* actions;        /* device f32[B, A]: the stored (unclipped) actions */
  const float* old_log_prob;   /* device f32[B] */
  const float* advantages;     /* device f32[B] (already normalised if the caller normalises) */
  const float* returns;        /* device f32[B] */
  const float* log_std;        /* device f32[A], read when the launch runs */
  float clip_range;            /* c, in (0, 1) */
  float vf_coef, ent_coef;     /* not NaN */
  int32_t reserved;            /* 0 */
  float* values;               /* device f32[B] or NULL: v */
  float* log_prob;             /* device f32[B] or NULL: lp */
  float* stats;                /* device f32[8] */
} FleetPpoGradArgs;
typedef struct FleetPpo* fleet_ppo_handle;

/* FLEET_ERR_INVALID (fleet_ppo_last_error(NULL) says why, starting with the entry's name) for a null or wrongly sized FleetPpoParams,
 * max_batch outside 1..2^24, a null output or policy, a one-head policy, a critic whose last width is not 1 or whose output is not
 * NONE.  FLEET_ERR_HIP with the byte count when the scratch cannot be allocated.
 * A handle of another family (a fleet_qtarget handle) is refused as well: "the handle is not a policy handle". */
int fleet_ppo_create(fleet_policy_handle policy, const FleetPpoParams* p, fleet_ppo_handle* out);
int fleet_ppo_destroy(fleet_ppo_handle h);
const char* fleet_ppo_last_error(fleet_ppo_handle h);  /* h may be NULL: error of the last failed call without a handle */
/* the parameters the handle was created with, the bytes of its scratch, and the rows one workgroup of the rows launch takes */
int fleet_ppo_describe(fleet_ppo_handle h, FleetPpoParams* out, uint64_t* scratch_bytes, int32_t* tile_rows);
/* Two launches, enqueued only.  grads: a host array of `count` device pointers, the gradient tensors in torch's [out, in] layout and
 * fleet_policy_load_dev's order (W, b per layer, head 0 then head 1), then log_std's f32[A]: count = the policy's tensors + 1.
 * FLEET_ERR_INVALID (nothing is launched) for a null or wrongly sized FleetPpoGradArgs, B < 1, a null obs / actions / old_log_prob /
 * advantages / returns / log_std / stats, a clip_range outside (0, 1) or NaN, a NaN vf_coef or ent_coef, a null grads or a null
 * pointer in it, and -- these two need the handle -- a count that is not the policy's tensors + 1, B > max_batch.  The arguments are
 * looked at before the handle is: with h NULL the reason (or "null handle") goes to fleet_ppo_last_error(NULL). */
int fleet_ppo_grad_dev(fleet_ppo_handle h, const FleetPpoGradArgs* args, float* const* grads, int count);

/* -- the same with value-function clipping (clip_range_vf; DESIGN.md "PPO's value clipping on the device") --
 * (an entry added under FLEET_ABI_VERSION 11 on the existing handle: fleet_ppo_grad_dev and FleetPpoGradArgs are as they were)
 * SB3 2.3.2 with clip_range_vf = cv > 0:  values_pred = old_values + clamp(values - old_values, -cv, cv);  value_loss =
 * mse_loss(returns, values_pred).  Per row b, with ov = old_values[b], the critic head's tail becomes, float32, no contraction:
 *   dl  = v - ov
 *   cd  = dl < -cv ? -cv : (dl > cv ? cv : dl)
 *   vp  = ov + cd
 *   e   = ret - vp;  the row's value term is e * e             (stats[1] = total(e * e) * invB, the same compensated sums)
 *   inside = (dl >= -cv && dl <= cv)                           (torch's clamp backward: ties pass, NaN does not)
 *   dv  = inside ? ((2.0f * vf_coef) * invB) * (vp - ret) : 0.0f
 * values[b] stays the unclipped v.  The critic's tensors, stats[1] and with it stats[3] follow from dv and e; the actor's tensors, the
 * log_std gradient, stats[0], [2], [4], [5], values and log_prob are fleet_ppo_grad_dev's bits on the same batch.  The same two
 * launches (the rows launch is a second instance of its kernel with the clip compiled in, so that the first stays the code it was),
 * the same scratch, the same rules.
 * FLEET_ERR_INVALID for a null or wrongly sized FleetPpoGradVclipArgs, whatever fleet_ppo_grad_dev refuses of `base` (in its words), a
 * null old_values, a clip_range_vf that is not finite and > 0; the arguments are looked at before the handle is. */
typedef struct FleetPpoGradVclipArgs {
  int32_t struct_bytes;        /* sizeof(FleetPpoGradVclipArgs) */
  float clip_range_vf;         /* cv: finite, > 0 */
  const float* old_values;     /* device f32[B]: the values the rollout stored */
  FleetPpoGradArgs base;       /* everything fleet_ppo_grad_dev takes; base.struct_bytes = sizeof(FleetPpoGradArgs) */
} FleetPpoGradVclipArgs;
extern int fleet_ppo_grad_vclip_dev(fleet_ppo_handle h, const FleetPpoGradVclipArgs* args, float* const* grads, int count);

/* -- the same behind a gate, for early stopping on approx_kl (target_kl; DESIGN.md "PPO's early stopping on the device") --
 * (an entry added under FLEET_ABI_VERSION 11 on the existing handle: the entries above are as they were)
 * fleet_ppo_grad_dev (clip_range_vf == 0) or fleet_ppo_grad_vclip_dev (clip_range_vf > 0, with old_values) behind two device words:
 *   skip     u32[1], written by an EARLIER launch, read when the launches run: nonzero means that every workgroup of both launches
 *            returns at its top (one uniform load, a scalar branch) and NOTHING is written: no gradient, no stats, no decided
 *   decided  u32[1], written by the statistics workgroup behind stats:  decided = ((double)stats[4] > threshold) ? 1 : 0
 *            (stats[4] = approx_kl, the float32 that was stored; a NaN gives 0).  No workgroup of these two launches reads it.
 * With skip clear the gradients, stats, values and log_prob are the ungated entry's, bit for bit; the launches are gated instances of
 * the same kernels (the ungated ones stay the code they were).  skip and decided must be two words: no launch reads a word that a
 * workgroup of the same launch may write.
 * FLEET_ERR_INVALID for a null or wrongly sized FleetPpoGradGatedArgs, whatever fleet_ppo_grad_dev refuses of `base` (in its words), a
 * clip_range_vf that is negative or not finite, a null old_values with clip_range_vf > 0, a null gate.skip or gate.decided, the same
 * word for both, a NaN gate.threshold; the arguments are looked at before the handle is. */
typedef struct FleetPpoGate {
  const uint32_t* skip;        /* device u32[1] */
  uint32_t* decided;           /* device u32[1] */
  double threshold;            /* not NaN; fleet_train_ppo_kl_dev passes 1.5 * target_kl */
} FleetPpoGate;
typedef struct FleetPpoGradGatedArgs {
  int32_t struct_bytes;        /* sizeof(FleetPpoGradGatedArgs) */
  float clip_range_vf;         /* 0: no value clipping; otherwise cv: finite, > 0 */
  const float* old_values;     /* device f32[B]; read only when clip_range_vf > 0 */
  FleetPpoGate gate;
  FleetPpoGradArgs base;       /* everything fleet_ppo_grad_dev takes; base.struct_bytes = sizeof(FleetPpoGradArgs) */
} FleetPpoGradGatedArgs;
FLEET_API int fleet_ppo_grad_gated_dev(fleet_ppo_handle h, const FleetPpoGradGatedArgs* args, float* const* grads, int count);

/* ==== SAC on the device: squashed-Gaussian actor and soft Q targets (fleet_sac.hip; DESIGN.md "SAC on the device") ====================
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays.  The section stands behind the
 * last of the "----" sections, whose order and count stay what they were, and every entry of it starts with fleet_sac_.)
 * The forward side of stable-baselines3 2.3.2's SAC: the stochastic actor's action with its log-probability in ONE launch, and the
 * entropy-regularised bootstrap target of a minibatch in ONE launch.  float32 throughout, no contraction except the fmaf written.
 * Networks.  SB3's SAC actor is latent_pi (an MLP) followed by two linear heads over the same input, mu and log_std.  Here it is ONE
 * FleetPolicyHead over D = obs_dim inputs whose last layer has width 2A: rows 0..A-1 are mu, rows A..2A-1 are log_std, the output
 * transform is NONE.  One torch parameter pair [2A, H] / [2A] -- cat([mu.weight, log_std.weight]) -- is one layer of the weight image
 * (Wt[in4][out64], zero padding, as the policy's).  2A <= FLEET_POLICY_MAX_WIDTH, so A <= 256.  Critic c is SB3's ContinuousCritic over
 * D + A inputs (not D + 2A), last width 1, output NONE; D + A <= FLEET_POLICY_MAX_OBS_DIM.
 * fleet_sac_create returns a fleet_qtarget_handle of the existing type, marked as a squashed actor's.  The entries that only walk nets
 * or critics serve it unchanged: fleet_qtarget_destroy / _last_error / _set_stream / _load_host / _load_dev / _polyak_dev / _export_dev /
 * _describe (FleetQTargetParams: the actor's last width reads 2A), fleet_td3_create with fleet_td3_critic_grad_dev (the critics' input is
 * D + act_dim, and the scratch is laid out per net), fleet_adam_create_qtarget.  Three entries would run the actor forward as a TD3
 * actor and REFUSE such a handle with FLEET_ERR_INVALID, their name and the reason in their last_error, nothing launched:
 * fleet_qtarget_target_dev, fleet_td3_actor_grad_dev (its kernel takes act64 for the actor's last out64), fleet_offpolicy_create.
 * The action, per row e of obs f32[E,D] (`norm` as for fleet_policy_forward_dev), exactly:
 *   m[j], l[j]  = columns j and A + j of the actor's last layer: the policy section's chain (acc = 0; fmaf ascending k; + bias)
 *   ls[j]       = l[j] < -20.0f ? -20.0f : (l[j] > 2.0f ? 2.0f : l[j])          (SB3's LOG_STD_MIN / LOG_STD_MAX)
 *   sd[j]       = expf(ls[j]);   u[j] = fmaf(sd[j], eps[j], m[j]);   a[j] = tanhf(u[j])
 *   t[j]        = fmaf(-0.5f * eps[j], eps[j], -ls[j]) - 0.9189385332f            (the Gaussian's log-density at u, written in eps)
 *   c[j]        = logf((1.0f - a[j] * a[j]) + 1e-6f)                              (SB3's correction, epsilon 1e-6, on the STORED action)
 *   log_prob    = S(t) - S(c)     S: the lane order of fleet_explore_act_dev (lane i of 64 adds j = i, i+64, ... ascending; xor butterfly 1..32)
 *   deterministic: a[j] = tanhf(m[j]); no noise is read or written; log_prob / gaussian_actions / noise must be NULL
 * eps is the existing draw: Philox4x32-10 under key (seed lo, seed hi) at counter (env_id_offset + e, j / 4, step lo, step hi) over the A
 * action columns (not 2A), Box-Muller as there: under one (seed, step, env id) the bits fleet_explore_act_dev draws.  noise_mode
 * FLEET_EXPLORE_NOISE_DRAW or _GIVEN as there; DRAW with a non-null `noise` records the draw.
 * Deviation from SB3: torch's Normal.log_prob computes -(u - m)^2 / (2 sd^2) - ls - log(sqrt(2 pi)); t[j] is the same quantity with
 * (u - m) / sd = eps put in.  It does not depend on expf's last bit, and it can be restated exactly from stored values (ls, eps).
 * The correction is SB3's SquashedDiagGaussianDistribution.log_prob, log(1 - tanh(u)^2 + 1e-6), evaluated on the action that was stored.
 * Every output of a row is a function of that row: not of E, of the row's place, of which optional outputs are asked for, of the stream.
 * The target, per row b (next_obs f32[B,D] normalised, rewards f32[B], dones f32[B], as fleet_replay_sample_dev writes them):
 *   a', lp = exactly the action above on next_obs[b], by the ONLINE handle's actor   (the same code path: the bits fleet_sac_act_dev
 *            gives for that row, seed, step and offset)
 *   q_c    = critic c of the TARGETS handle over concat(next_obs[b], a'): the learning targets' chain
 *   qmin   = n_critics == 2 ? (q_1 < q_0 ? q_1 : q_0) : q_0
 *   p = alpha * lp;  v = qmin - p;  t = (1.0f - dones[b]) * gamma;  y[b] = rewards[b] + t * v       (each rounded on its own: no fma)
 * alpha = ent_coef[0], a device float read when the launch runs: the caller keeps exp(log_ent_coef) in a tensor.  One workgroup takes
 * 16 rows through the online actor, then through the target critics: two image bases, no atomics, no ordering between workgroups.
 * The targets handle keeps a copy of the actor that nothing reads; a Polyak update over all tensors stays correct.  As for the TD3
 * targets, the target gets a SEED OF ITS OWN, different from the acting seed.
 * Every *_dev call takes device pointers, only enqueues and runs on the handle's stream (fleet_qtarget_set_stream).  The actor and
 * entropy-coefficient gradients are the section below's.  Out of scope: a one-call train(), a SAC collector, gSDE, a log_ent_coef
 * form of alpha. */
typedef struct FleetSacParams {
  int32_t struct_bytes;       /* sizeof(FleetSacParams) */
  int32_t obs_dim;            /* D >= 1 */
  int32_t n_critics;          /* 1 or 2 */
  int32_t reserved;           /* 0 */
  FleetPolicyHead actor;      /* over D inputs; the last width is 2A (even), the output FLEET_POLICY_OUT_NONE */
  FleetPolicyHead critic[2];  /* over D + A inputs; the last width must be 1, the output FLEET_POLICY_OUT_NONE */
} FleetSacParams;
typedef struct FleetSacActArgs {
  int32_t struct_bytes;     /* sizeof(FleetSacActArgs) */
  int32_t noise_mode;       /* FLEET_EXPLORE_NOISE_DRAW / _GIVEN */
  int32_t deterministic;    /* 0 / 1 */
  int32_t env_id_offset;    /* global id of row 0; >= 0 */
  uint64_t seed;            /* Philox key */
  uint64_t step;            /* Philox counter words 2, 3 */
  float* noise;             /* device f32[E, A] or NULL: read (GIVEN), written when not NULL (DRAW) */
  float* actions;           /* device f32[E, A]: the squashed action a, which both the env and the buffer get */
  float* gaussian_actions;  /* device f32[E, A] or NULL: the pre-squash u */
  float* log_prob;          /* device f32[E] or NULL */
  float* mean;              /* device f32[E, A] or NULL: m */
  float* log_std;           /* device f32[E, A] or NULL: the clamped ls */
} FleetSacActArgs;
typedef struct FleetSacTargetArgs {
  int32_t struct_bytes;     /* sizeof(FleetSacTargetArgs) */
  int32_t noise_mode;       /* FLEET_EXPLORE_NOISE_DRAW / _GIVEN */
  uint64_t seed;            /* Philox key: not the acting seed */
  uint64_t step;            /* Philox counter words 2, 3: the caller's gradient-step count */
  int32_t row_offset;       /* global id of row 0 (a shard of a larger minibatch); >= 0 */
  float gamma;              /* the discount */
  const float* ent_coef;    /* device f32[1]: alpha itself, read when the launch runs */
  float* noise;             /* device f32[B, A] or NULL: read (GIVEN), written when not NULL (DRAW) */
  float* target_q;          /* device f32[B]: y */
  float* next_actions;      /* device f32[B, A] or NULL: a' */
  float* next_log_prob;     /* device f32[B] or NULL: lp */
  float* q;                 /* device f32[B, n_critics] or NULL: q_c */
} FleetSacTargetArgs;

/* The parameters and the weights are validated BEFORE the device is touched: FLEET_ERR_INVALID (fleet_sac_last_error(NULL) says why,
 * starting with the entry's name) for a wrong struct_bytes, obs_dim < 1, n_critics outside 1..2, a layer count outside 1..4, a width
 * outside 1..512 (so 2A > 512), an odd last actor width, an actor output that is not NONE, D + A above 8192, a critic whose last width
 * is not 1 or whose output is not NONE, an unknown activation, a null pointer, a weight that is not finite.
 * host_weights: packed float32 -- the actor, then critic 0, then critic 1; for each layer W[out, in] (row-major) then b[out]. */
int fleet_sac_create(int device, const FleetSacParams* p, const float* host_weights, fleet_qtarget_handle* out);
/* h may be NULL: error of the last failed fleet_sac_* call without a handle; with a handle, what fleet_qtarget_last_error(h) returns */
const char* fleet_sac_last_error(fleet_qtarget_handle h);
/* One launch.  FLEET_ERR_INVALID (nothing is launched) for a null or wrongly sized FleetSacActArgs, an unknown noise_mode, E < 1, a null
 * obs / actions, a deterministic outside 0..1, GIVEN with a null noise, a negative env_id_offset, a noise / log_prob / gaussian_actions
 * with deterministic -- these are looked at before the handle is: with nets NULL the reason (or "null handle") goes to
 * fleet_sac_last_error(NULL) -- and, with the handle, for one whose actor is not squashed and a normaliser of another width or device. */
int fleet_sac_act_dev(fleet_qtarget_handle nets, const float* obs, int E, fleet_norm_handle norm, const FleetSacActArgs* a);
/* One launch on the online handle's stream.  FLEET_ERR_INVALID (nothing is launched) for a null or wrongly sized FleetSacTargetArgs, an
 * unknown noise_mode, B < 1, a null next_obs / rewards / dones / ent_coef / target_q, GIVEN with a null noise, a negative row_offset
 * (before the handle, as above), and, in the online handle's last_error: a null `targets`, a handle of either that fleet_sac_create did
 * not make, obs_dim, act_dim or n_critics that differ between the two, another device, handles that do not launch on one stream. */
int fleet_sac_target_dev(fleet_qtarget_handle online, fleet_qtarget_handle targets, const float* next_obs, const float* rewards,
                         const float* dones, int B, const FleetSacTargetArgs* a);

/* ==== SAC actor and entropy-coefficient gradients on the device (fleet_td3.hip: sac_actor_rows, sac_weights; DESIGN.md "SAC's actor
 * ==== and entropy-coefficient gradients on the device") ==============================================================================
 * (an entry added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays.  It is declared
 * `extern FLEET_API int`, behind the SAC section's own -- closed -- list of entries, and starts with fleet_sac_.)
 * What stable-baselines3 2.3.2's SAC.train does with one minibatch for the actor and for a learned entropy coefficient, in TWO launches,
 * on a fleet_td3 handle whose networks handle came from fleet_sac_create (the ONLINE networks, the critics AFTER their optimiser step):
 *   actions_pi, log_prob = actor.action_log_prob(obs)
 *   ent_coef_loss = -(log_ent_coef * (log_prob + target_entropy).detach()).mean()
 *   actor_loss    = (ent_coef * log_prob - min_c critic_c(obs, actions_pi)).mean()              (gradient into the actor only)
 * Forward, per row b: m, l, ls, eps, a and lp = log_prob exactly as the section above has them -- the same epilogue code: under one
 * (seed, row_offset + b, step) the bits fleet_sac_act_dev gives for that row; q_c = critic c over concat(obs[b], a), the learning
 * targets' chain; the selecting critic k = 1 when n_critics == 2 and NOT (q_0 <= q_1), else 0; qmin = q_k.
 * Backward, float32, every operation rounded on its own (no contraction but the fmaf written); invB = 1.0f / (float)B, alpha =
 * ent_coef[0] read when the launch runs, ab = alpha * invB:
 *   critic c is walked back from dq = -invB in the rows with k == c and 0.0f in the others, as fleet_td3_actor_grad_dev walks critic 0,
 *   to its first layer's delta d0 and into the action columns: da_c[j] = (acc = 0; acc = fmaf(Wt0[D + j][i], d0[i], acc), i ascending);
 *   da[j] = da_0[j], with two critics da_0[j] + da_1[j]        (one addend is an exact zero in every row)
 *   w     = 1.0f - a[j] * a[j];   g = (2.0f * a[j]) / (w + 1e-6f);   dLa = da[j] + ab * g;   du = dLa * w
 *   dm[j] = du                                                       (the delta of column j of the actor's last layer)
 *   dl[j] = (l[j] >= -20.0f && l[j] <= 2.0f) ? (du * (sdb * eps[j])) - ab : 0.0f      (the delta of column A + j; torch's clamp
 *           backward, the bounds inclusive)   with sdb = (float)exp((double)ls[j]): the DOUBLE exponential rounded once, not the
 *           forward's expf, so that the deltas can be restated from stored values (ls, eps, a) without the device's expf bits
 *   then back through the actor's layers and into dW, db exactly as the TD3 section has it (d_prev, dW[j][k], db[j]).
 * No critic gradient is produced (SB3 discards it there too).  The last layer's pair is the ONE [2A, H] / [2A] pair of the image.
 * Statistics, stats f32[8], tiles and compensated sums as the TD3 section has them, term_b = alpha * lp - qmin (two roundings):
 *   [0] actor_loss = total(term) * invB;  [2] = total(lp) * invB;  [3] = total(qmin) * invB;  [4] = alpha as read;  [5..7] 0
 *   with log_ent_coef:  gl = -([2] + target_entropy);  log_ent_coef_grad[0] = gl;  [1] ent_coef_loss = log_ent_coef[0] * gl;  else [1] = 0
 * Every result is a function of the inputs and B only, as for the TD3 entries; the gradient tensors, stats and log_ent_coef_grad are
 * OVERWRITTEN.  Launches on the NETWORKS handle's stream; rows at and past B are neither read nor written. */
typedef struct FleetSacActorArgs {
  int32_t struct_bytes;        /* sizeof(FleetSacActorArgs) */
  int32_t B;                   /* rows, 1..max_batch */
  int32_t noise_mode;          /* FLEET_EXPLORE_NOISE_DRAW / _GIVEN */
  int32_t row_offset;          /* global id of row 0; >= 0 */
  uint64_t seed;               /* Philox key */
  uint64_t step;               /* Philox counter words 2, 3 */
  const float* obs;            /* device f32[B, D] (normalised, as the replay buffer samples them) */
  const float* ent_coef;       /* device f32[1]: alpha itself, read when the launches run */
  float* noise;                /* device f32[B, A] or NULL: read (GIVEN), written when not NULL (DRAW) */
  const float* log_ent_coef;   /* device f32[1] or NULL: asks for ent_coef_loss and its gradient */
  float* log_ent_coef_grad;    /* device f32[1]: given exactly when log_ent_coef is */
  float target_entropy;        /* SB3's "auto": -(float)A */
  int32_t reserved;            /* 0 */
  float* actions_out;          /* device f32[B, A] or NULL: a */
  float* log_prob_out;         /* device f32[B] or NULL: lp */
  float* q_out;                /* device f32[B, n_critics] or NULL: q_c */
  float* dheads_out;           /* device f32[B, 2A] or NULL: dm, then dl */
  float* stats;                /* device f32[8] */
} FleetSacActorArgs;
/* Two launches, enqueued only.  grads: W, b per layer of the actor; count is checked as fleet_td3_actor_grad_dev checks it.
 * FLEET_ERR_INVALID (nothing is launched; the message starts with the entry's name) for a null or wrongly sized FleetSacActorArgs, an
 * unknown noise_mode, B < 1, a null obs / ent_coef / stats, GIVEN with a null noise, a negative row_offset, one of log_ent_coef and
 * log_ent_coef_grad without the other, a reserved that is not 0, a null grads or a null pointer in it -- looked at before the handle:
 * with h NULL the reason (or "null handle") goes to fleet_td3_last_error(NULL) -- and, with the handle, a wrong count, B > max_batch,
 * and networks whose actor is not squashed (the message points to fleet_td3_actor_grad_dev). */
extern FLEET_API int fleet_sac_actor_grad_dev(fleet_td3_handle h, const FleetSacActorArgs* a, float* const* grads, int count);

/* ==== SAC's whole update on the device (fleet_sactrain.hip; DESIGN.md "SAC's whole update on the device") ===========================
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays.  They are declared
 * `FLEET_API extern`, behind the closed entry lists of the sections above, and every one starts with fleet_sactrain_.)
 * stable-baselines3 2.3.2's SAC.train(gradient_steps, batch_size) as ONE enqueue-only call.  The handle BORROWS its handles, which must
 * outlive it: a replay buffer, the TARGET critics' fleet_sac_create handle, and -- all on ONE second fleet_sac_create handle that holds
 * the ONLINE networks -- a fleet_td3 gradient handle, a fleet_adam handle over the actor (span 0, 1, no extras), one over the critics
 * (span 1, n_critics, no extras) and, for a learned entropy coefficient, one over no net with ONE extra of length 1 (log_ent_coef);
 * NULL for a fixed alpha.  It owns one block, zeroed at create: the staging arrays of max_batch rows (the gradient handle's; the six
 * of the TD3 section), one alpha cell, max_steps slots of f32[FLEET_SACTRAIN_SLOT_FLOATS] -- the critic launch's stats[8], then the
 * actor launch's -- and the scale launch's chunk table.
 * Gradient step g = 0 .. gradient_steps - 1 of a call, with u = first_update + g, through the families' own entries, as they are:
 *   1. fleet_replay_sample_dev(replay, batch_size, norm, the staging arrays): the buffer's own call counter advances by gradient_steps
 *   2. learned alpha only: the alpha launch, alpha = (float)exp((double)log_ent_coef[0]), into the alpha cell -- read BEFORE the
 *      entropy coefficient's optimiser step of this gradient step, as SB3 reads it; a fixed alpha: the caller's ent_coef pointer as it is
 *   3. fleet_sac_target_dev(online, targets) from the staged next_obs, rewards and dones into the staged target_q; DRAW (not recorded),
 *      key (target_seed, row_offset 0, step = u)
 *   4. fleet_td3_critic_grad_dev on the staged obs, actions and target_q; stats -> slot g, floats 0..7
 *   5. the scale launch, grad[i] = grad[i] * (float)loss_scale over the critics' gradient tensors (SB3's critic loss is 0.5 * the
 *      launches'); skipped when (float)loss_scale == 1
 *   6. fleet_adam_step_dev(adam_critic, lr, beta1[1], beta2[1], eps[1], max_grad_norm[1])
 *   7. fleet_sac_actor_grad_dev on the staged obs, on the critics just stepped; key (seed, row_offset 0, step = u); stats -> slot g,
 *      floats 8..15; log_ent_coef and log_ent_coef_grad when learned
 *   8. fleet_adam_step_dev(adam_actor, ... [0])
 *   9. learned alpha only: fleet_adam_step_dev(adam_ent, ... [2]) on (log_ent_coef, log_ent_coef_grad)
 *  10. iff g % target_update_interval == 0 -- the index INSIDE the call, not the update count: step 0 of every call updates the
 *      targets -- the image-to-image Polyak update of the TD3 section on the two images (the same kernel)
 * and one closing launch per call.  The result is bit-equal to the same entries called one by one.  Every argument is stateless.
 * The alpha launch is the DOUBLE exponential rounded once, so that the value can be restated on the host; it is not torch.exp's bits.
 * The scale launch: one workgroup per chunk of 1024 consecutive elements of ONE tensor, the tensors' pointers in the kernel arguments.
 * The statistics block, stats f64[FLEET_TRAIN_STATS], written by the closing launch (one workgroup of 256 threads) with the ordered
 * float64 sum S of "PPO's whole update on the device" over the call's slots, G = gradient_steps, c[g] / a[g] the critic / actor half:
 *   [0] critic_loss = (double)(float)loss_scale * S((double)c[g][0]) / (double)G      [1] actor_loss = S(a[g][0]) / G
 *   [2] ent_coef = S(a[g][4]) / G       [3] ent_coef_loss = S(a[g][1]) / G, NaN with a fixed alpha
 *   [4] the LAST step's critic loss, (double)(float)loss_scale * (double)c[G-1][0]     [5] the last step's actor loss
 *   [6] (double)(first_update + G) (train/n_updates)      [7] the call's target updates, (G - 1) / target_update_interval + 1
 *   [8] S(a[g][2]) / G, the mean log_prob      [9] S(a[g][3]) / G, the mean qmin      [10..15] 0
 * Every *_dev call takes device pointers, only enqueues and launches on the stream the borrowed handles launch on: the replay buffer,
 * the target networks and the online networks must launch on ONE stream.  No atomics, no ordering between workgroups: launch
 * boundaries only.  Calls are serialised by the caller.  Out of scope: a SAC collector, gSDE, learning-rate schedules inside a call. */
#define FLEET_SACTRAIN_MAX_STEPS 65536
#define FLEET_SACTRAIN_SLOT_FLOATS 16
#define FLEET_SACTRAIN_SCALE_CHUNK 1024
typedef struct FleetSacTrainParams {
  int32_t struct_bytes;          /* sizeof(FleetSacTrainParams) */
  int32_t max_steps;             /* 1..FLEET_SACTRAIN_MAX_STEPS: gradient steps one call may take */
} FleetSacTrainParams;
typedef struct FleetSacTrainArgs {
  int32_t struct_bytes;          /* sizeof(FleetSacTrainArgs) */
  int32_t gradient_steps;        /* 1..max_steps */
  int32_t batch_size;            /* 1..max_batch */
  int32_t target_update_interval; /* >= 1 */
  float gamma;                   /* the discount, as fleet_sac_target_dev takes it */
  float target_entropy;          /* as fleet_sac_actor_grad_dev takes it (SB3's "auto": -(float)A); read with a learned alpha only */
  double tau;                    /* in [0, 1] */
  double loss_scale;             /* finite; SB3: 0.5.  Used as (float)loss_scale */
  double lr;                     /* finite, >= 0; all optimisers', constant within the call */
  double beta1[3], beta2[3];     /* in [0, 1); [0] the actor optimiser's, [1] the critics', [2] the entropy coefficient's, here and below */
  double eps[3];                 /* finite, >= 0 */
  double max_grad_norm[3];       /* <= 0: no clipping (SB3's SAC) */
  uint64_t seed;                 /* Philox key of the actor step's draw */
  uint64_t target_seed;          /* Philox key of the target's draw: not `seed` */
  uint64_t first_update;         /* gradient steps taken before this call */
  const float* ent_coef;         /* device f32[1]: a FIXED alpha; exactly one of ent_coef and log_ent_coef */
  float* log_ent_coef;           /* device f32[1]: the LEARNED coefficient's logarithm, stepped in place; given exactly when adam_ent was */
  float* log_ent_coef_grad;      /* device f32[1]: given exactly when log_ent_coef is */
  fleet_norm_handle norm;        /* or NULL: the minibatches are sampled raw */
  double* stats;                 /* device f64[FLEET_TRAIN_STATS] */
} FleetSacTrainArgs;
typedef struct FleetSacTrainInfo {
  int32_t obs_dim, act_dim, n_critics;   /* the networks' D, A and critics */
  int32_t max_batch;             /* the gradient handle's: rows the staging arrays hold */
  int32_t max_steps;             /* slots */
  int32_t n_actor_tensors;       /* the counts the update takes: W, b per layer of the actor ... */
  int32_t n_critic_tensors;      /* ... and of the critics, critic after critic */
  int32_t learned_alpha;         /* 1 when created with an entropy-coefficient optimiser */
  int32_t scale_chunks;          /* workgroups of the scale launch */
  int32_t reserved;
  uint64_t staging_bytes;        /* of the staging arrays */
  void* staging;                 /* device: obs, actions, next_obs, dones, rewards, target_q as in FleetOffpolicyInfo */
  void* alpha;                   /* device f32[1]: the alpha cell (the last step's alpha with a learned coefficient) */
  void* slots;                   /* device f32[max_steps][FLEET_SACTRAIN_SLOT_FLOATS]: the last call's per-step stats */
} FleetSacTrainInfo;
typedef struct FleetSacTrain* fleet_sactrain_handle;

/* FLEET_ERR_INVALID (fleet_sactrain_last_error(NULL) says why, starting with the entry's name) for a null or wrongly sized
 * FleetSacTrainParams, max_steps out of range, a null output or handle (adam_ent alone may be NULL), networks that fleet_sac_create did
 * not make (the message points to fleet_offpolicy_create), online and target networks that are one handle, whose records differ in any
 * byte or that lie on different devices, an optimiser on another image than the gradient handle, an optimiser whose span is not the one
 * stated above, a replay buffer on another device or whose D or A differs from the networks'.  FLEET_ERR_HIP with the byte count when
 * the block cannot be allocated. */
FLEET_API extern int fleet_sactrain_create(fleet_replay_handle replay, fleet_qtarget_handle targets, fleet_td3_handle grad,
                                           fleet_adam_handle adam_actor, fleet_adam_handle adam_critic, fleet_adam_handle adam_ent,
                                           const FleetSacTrainParams* p, fleet_sactrain_handle* out);
FLEET_API extern int fleet_sactrain_destroy(fleet_sactrain_handle h);
FLEET_API extern const char* fleet_sactrain_last_error(fleet_sactrain_handle h);  /* h may be NULL: the last failed call without a handle */
FLEET_API extern int fleet_sactrain_describe(fleet_sactrain_handle h, FleetSacTrainInfo* out);
/* The alpha launch on its own: out[0] = (float)exp((double)log_ent_coef[0]); out NULL: the handle's alpha cell.  FLEET_ERR_INVALID for
 * a null log_ent_coef. */
FLEET_API extern int fleet_sactrain_alpha_dev(fleet_sactrain_handle h, const float* log_ent_coef, float* out);
/* The scale launch on its own: grads[t][i] = grads[t][i] * (float)s over the critics' gradient tensors (W, b per layer, critic after
 * critic), also for s == 1.  FLEET_ERR_INVALID for an s that is not finite, a null grads or a null pointer in it, a wrong count. */
FLEET_API extern int fleet_sactrain_scale_dev(fleet_sactrain_handle h, float* const* grads, int count, double s);
/* The image-to-image Polyak update on its own, one launch: the targets' image <- the online image.  FLEET_ERR_INVALID for a tau outside
 * [0, 1] or NaN, and when the two handles do not launch on one stream. */
FLEET_API extern int fleet_sactrain_polyak_dev(fleet_sactrain_handle h, double tau);
/* The update.  actor_params / actor_grads: host arrays of n_actor device pointers as fleet_adam_step_dev takes them (W, b per layer of
 * the actor, the last pair the ONE [2A, H] / [2A] pair); critic_params / critic_grads: the critics', critic after critic.  The
 * parameters are stepped in place (and the online image with them); the gradient tensors hold the last step's gradients (the critics'
 * scaled).  Everything that can be refused is refused before the first launch: nothing is launched then, and the replay buffer's call
 * counter and all three step counts stay.  FLEET_ERR_INVALID for a null or wrongly sized FleetSacTrainArgs, gradient_steps < 1,
 * batch_size < 1, target_update_interval < 1, a null stats, both or neither of ent_coef and log_ent_coef, one of log_ent_coef and
 * log_ent_coef_grad without the other, a loss_scale that is not finite, whatever the entries above refuse (in their words), and -- these
 * need the handle -- gradient_steps above max_steps, batch_size above max_batch, wrong tensor counts, a log_ent_coef that is not given
 * exactly when adam_ent was, a norm whose obs_dim is not D, a replay buffer, target networks and online networks that do not launch on
 * one stream; FLEET_ERR_STATE for an empty buffer.  The arguments are looked at before the handle is: with h NULL the reason (or "null
 * handle") goes to fleet_sactrain_last_error(NULL). */
FLEET_API extern int fleet_sactrain_sac_dev(fleet_sactrain_handle h, const FleetSacTrainArgs* a, float* const* actor_params,
                                            float* const* actor_grads, int n_actor, float* const* critic_params,
                                            float* const* critic_grads, int n_critic);

#ifdef __cplusplus
}
#endif
#endif /* FLEET_HIP_H */
