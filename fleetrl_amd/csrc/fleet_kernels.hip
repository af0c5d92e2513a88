// fleet_kernels.hip -- the FleetEnv step / reset hot path as hand-written HIP for gfx950 (MI355X, CDNA4).
//
// What runs here (reference: the fleetrl package, float64 in the reference's operation order):
//   EvCharger.charge            utils/ev_charging/ev_charger.py:39-231
//   LoadCalculation.check_violation + ScoreConfig.overloading_penalty
//                               utils/load_calculation/load_calculation.py:83-94, fleet_env/config/score_config.py:33-41
//   arrival/departure state machine + ScoreConfig.soc_violation_penalty
//                               fleet_env/fleet_environment.py:528-623, score_config.py:26-30
// and, in the headers this file includes (each opens with what it provides, what it restates and what it expects of its caller):
//   fleet_stamps.h       diagnostic time stamps (FLEET_STAMPS builds only)
//   fleet_wave.h         lane-group reductions, the start-row sampler, division by a reciprocal, the sigmoid penalties
//   fleet_obs.h          state addressing and stores; Observer*.get_obs + Unit/OracleNormalization.normalize_obs
//   fleet_rainflow.h     LogDataDeg.log_soc, RainflowSeiDegradation / EmpiricalDegradation.calculate_degradation
//                        ("Rainflow without a history replay" is described there)
//   fleet_reset.h        FleetEnv.reset (incl. the vec-env auto-reset) and fleet_reset_kernel
//   fleet_aux_kernels.h  dist factor, field gather, terminal-observation compaction, the two self-test kernels
//   fleet_step_plan.h    the host half: instance selection and every launcher
// This file stays the ONE translation unit (compiled into the library and, once more, into the code object of the direct-launch
// queue): it keeps the step -- ev_finish, ev_physics, the kernel-argument structs and fleet_step_kernel.
//
// Mapping.  One *group* of G lanes owns one env.  Up to 256 EVs per env every EV has a lane of its own: G = the smallest power
// of two >= N up to 64 (a 64-lane wavefront holds 64/G envs, a 256-thread workgroup 256/G), and two or four whole wavefronts of
// one workgroup for 64 < N <= 256 (kMaxGroup); beyond that lane g of a one-wavefront group walks EVs g, g+64, ...  Per-env sums
// (cashflow, reward, sum(action*there), penalty record) are reduced inside the wavefront -- lane-swap folds of four quantities at
// once for a whole wavefront, DPP row shifts / row broadcasts for smaller groups -- and, for an env of several wavefronts, the
// per-wavefront partial sums meet in the LDS behind one workgroup barrier; no atomics.  Every lane of a group tracks the per-env
// scalars (time row, episode end, sample count) redundantly in registers, so nothing written by one lane is re-read by another
// inside a launch.  No MFMA: there is no contraction on this path.
//
// Schedule columns in run-length form.  What a step needs of the (time row, EV) table -- There, time_left, SOC_on_return of
// the row it advances to -- travels with the state (`run`, struct SegRec in fleet_device.h): a lane holds the record of row
// t+1 when the launch starts, so nothing it needs to start its arithmetic depends on the env's time row, and it only touches
// the table when row t+2 crosses a schedule event of its EV (about 4 % of the EV-steps), for the NEXT launch.  The row
// flags the state machine needs travel in the env head; the physics record of the time row is requested when the head
// arrives and consumed late (money terms); the four table-derived auxiliary observation slots are computed per lane from the
// carried record (one reciprocal, no division; write_obs_ev in fleet_obs.h).
#include "fleet_device.h"
#include <cstddef>

#include "fleet_stamps.h"

namespace {

// Minimum workgroups per CU the kernels are compiled for (= waves per SIMD; register budget 512 / this).  What the instances
// need is tabulated in DESIGN.md section 4 ("Registers and occupancy", from tools/kres.sh).  The multi-step kernel wants ~150
// VGPRs; its wavefronts advance independently and are bound by their own dependent round trips, so what counts is that all of a
// 4096-env batch's wavefronts are resident at once: it is compiled for four per SIMD (128 VGPRs, a few dozen bytes of spills) --
// +21 % env-steps/s over the three its natural register count allows (profiles/r03_experiments/ab_multiwaves.log).  With several
// EVs per lane it stays at two.
constexpr int kSingleWaves = 4, kMultiWaves = 4, kMultiWideWaves = 2;
#ifndef FLEET_KBLOCK
#define FLEET_KBLOCK 256  // (a macro only because the diagnostic stamp code of fleet_stamps.h indexes its buffer with it)
#endif
constexpr int kBlock = FLEET_KBLOCK;  // threads per workgroup
// Largest lane group of one env in the single-step kernel: up to this many EVs every EV has a lane of its own.  Groups above 64
// lanes are two or four WAVEFRONTS of one workgroup: every wavefront reduces its lanes' terms as a one-wavefront env does, the
// per-wavefront partial sums meet in the LDS behind one workgroup barrier, and the group's last lane adds them up (round 5: the
// c5 shard's 200-EV envs as 4 wavefronts x 1 EV per lane instead of 1 wavefront x 4 EVs per lane walked one after the other).
constexpr int kMaxGroup = 256;
static_assert(kMaxGroup <= kBlock && kBlock % 64 == 0, "a lane group is a whole number of a workgroup's wavefronts");

}  // namespace

#include "fleet_wave.h"
#include "fleet_obs.h"
#include "fleet_rainflow.h"
#include "fleet_reset.h"

namespace {

// The tail of an EV's step: the rainflow push (second half), the linear model's daily update, the data-log row, and the
// stores of the state records that changed.
template <int DEG, bool WIDE>
__device__ __forceinline__ void ev_finish(const FleetDev& d, const EvIx& i, int c, int N, bool env_ok, bool deg_row, double dt_step, const RfReq& rq,
                                          int tail, int sgn, double soc, double soc_deg, double old_deg, float hl, uint32_t there1,
                                          bool t090, bool inplane, bool crosses, const SegRec& nr, double soh0, double a, double en, bool logs,
                                          size_t lrow, const Hot& h_in, uint32_t& err, double& sei_sample, double& sei_soh, int& sei_tail,
                                          RfTop& sei_top, bool& sei_have_top, RfAccHead& acc_c, RfTop& top_c, bool carry,
                                          bool own_b = false, bool deep = false) {
  double soh = soh0;
  RfTop top = top_c;
  if (DEG == FLEET_DEG_RAINFLOW && env_ok) {
    if (own_b) {  // (one step per launch, one EV per lane: see rf_finish_as)
      if (deep) rf_finish_win(d, i, rq, tail, top, acc_c, err);  // (the state-only twin: the second closure from the request's window)
      else rf_finish_own_b(d, i, rq, tail, top, acc_c, err);
    } else {
      rf_finish(d, i, rq, tail, top, acc_c, err);
    }
  }
  const bool pushed = rq.push;
  if (carry && pushed) top_c = top;
  if (DEG == FLEET_DEG_LINEAR && deg_row) soh = soh - linear_degradation(d, old_deg, soc_deg, dt_step);
  if (DEG == FLEET_DEG_RAINFLOW && !WIDE) {
    sei_sample = soc_deg;
    sei_soh = soh0;
    sei_tail = tail;
    sei_top = top;
    sei_have_top = pushed || carry;
  }
  if (logs) {  // action, energy, degradation, SoH (rainflow: the daily pass below overwrites the last two on its row)
    double* lev = d.log_ev + lrow * 4 * N + c;
    lev[0] = a;
    lev[N] = en;
    lev[2 * N] = soh0 - soh;
    lev[3 * N] = soh;
  }
  FLEET_STAMP(5);
  if (env_ok) {
    // soc_deg == soc whenever the EV has hours left; otherwise it keeps its previous value, which shares the record's float64
    // field with an empty slot's soc == 0.  An EV that is away and stays away leaves its record as it was: no store (what a
    // launch leaves dirty in the L2 is written back before it ends; a third of a caretaker fleet's EV-steps).
    const Hot h_out = hot_encode(d, i, soc, soc_deg, hl, tail, sgn, there1, t090, inplane);
    const bool same = (__double_as_longlong(h_out.x) == __double_as_longlong(h_in.x)) &&
                      (__float_as_uint(h_out.hl) == __float_as_uint(h_in.hl)) && (h_out.bits == h_in.bits);
    if (!same) st_rec16(ev_at(d.hot, i), h_out);
    if (crosses) st_rec16(ev_at(d.run, i), nr);  // the next launch advances into another segment of the EV's schedule
    if (DEG == FLEET_DEG_LINEAR && deg_row) *ev_at(d.soh, i) = soh;  // battery_cap = soh * init_cap is recomputed on use (:673)
  }
}

// ---------------------------------------------------------------------------------------------------------
// One EV's share of a step: EvCharger.charge (ev_charger.py:89-222) and the arrival / departure state machine
// (fleet_environment.py:528-623), without the money terms (they wait for the time row's physics record).  Shared by every
// step kernel.  `hb` = the EV's hot record, `old_deg` = its last logged SOC sample, `tb1` = the schedule columns of the row the
// step advances to, `soh0` = its state of health, `a` = its action.
// ---------------------------------------------------------------------------------------------------------
struct EvPhys {
  double soc, soc_deg;  // episode.soc / episode.soc_deg after the step
  double en;            // charged (> 0) / discharged (< 0) energy; 0 for an absent EV (:114 / :174)
  double rew;           // penalties and rewards of the EV except the price terms
  double penrec, miss;  // episode.penalty_record / cum_soc_missing contributions (:544-584)
  double a_th;          // action * there (fleet_environment.py:491)
  float hl;             // episode.hours_left
  bool pos, t090;       // action >= 0; sticky "target_soc = 0.9" (quirk Q7)
  bool event;           // EVENTS: something the reference counts into episode.events (real_time)
};
template <bool EVENTS>
__device__ __forceinline__ EvPhys ev_physics(const FleetDev& d, const Hot& hb, double old_deg, const RowRec& tb1, double soh0, double a,
                                             double dt_step, bool lunch) {
  EvPhys o;
  double rew = 0.0, penrec = 0.0, miss_sum = 0.0;
  bool ev_lane = false;
  const uint32_t th = HOT_THERE(hb.bits);  // There at the current time row, carried from the previous step / reset
  double soc = HOT_SOC(hb);
  float hl = hb.hl;
  const double cap = soh0 * d.init_cap;
  bool t090 = HOT_T090(hb.bits);
  const double tgt = t090 ? 0.9 : d.target_soc;
  const bool present = (th == 1u);

  // ---- EvCharger.charge (ev_charger.py:89-222) -----------------------------------------------------------------
  // Both action signs in ONE straight-line flow: every quantity of both branches is computed unconditionally and
  // merged with selects / min / max, so a wavefront whose lanes hold both signs (the normal case) does not walk two
  // masked branches, and there is no exec-mask bookkeeping on the hot path.
  const bool pos = (a >= 0.0);
  const double dem = d.p_avail * a * dt_step;   // demanded (dis)charge energy :101 / :162
  const double need = (tgt - soc) * cap;     // ev_total_energy_demand :100
  const double left = -1.0 * soc * cap;      // ev_total_energy_left :161
  // overcharging / over-discharging penalty :104-107 (applied even to an absent EV, clipped; quirk Q9) and
  // :165-167 (needs presence, not clipped)
  // (both products computed: a short-circuit would cost two masked regions for one multiplication)
  const bool viol_c = dem * d.eta_c > need;
  const bool viol_d = (dem * d.eta_d < left) & (th != 0u);
  const bool viol = pos ? viol_c : viol_d;
  const double x = pos ? (dem - need) : (left - dem);
  const double pen_raw = d.penalty_oc * (x * x);
  const double pen_oc = pos ? fmax(pen_raw, d.clip_oc) : pen_raw;
  rew += viol ? pen_oc : 0.0;
  const double lim = div_rcp(need, d.eta_c, d.inv_eta_c);  // need / eta_c, correctly rounded :114
  const double en_p = pos ? fmin(lim, dem) : fmax(left, dem);  // :114 / :174
  const double en = present ? en_p : 0.0;
  rew += (!present && fabs(a) > 0.05) ? d.penalty_invalid * (a * a) : 0.0;  // :120-122 / :180-182
  if (EVENTS) ev_lane = ev_lane || viol || (!present && fabs(a) > 0.05);     // episode.events :108,123,168,183
  soc = soc + div_rcp(pos ? en * d.eta_c : en, cap, rcp_newton1(cap));  // soc + energy / cap, the quotient correctly rounded :128 / :189
  o.a_th = a * (double)th;  // corrected_actions = actions * there (fleet_environment.py:491)

  // ---- arrival / departure state machine (fleet_environment.py:528-623) ----------------------------------
  const float ntl = tb1.tl;
  // departure :532, arrival :603, low state of health :615 are events too
  if (EVENTS) ev_lane = ev_lane || ((hl != 0.0f) != (ntl != 0.0f)) || (soh0 <= 0.9);
  if ((hl != 0.0f) && (ntl == 0.0f)) {  // a car just left :531
    const double target = lunch ? d.target_soc_lunch : tgt;  // :536-557
    const double missing = target - soc;
    if (missing > d.eps) {
      const double pen = soc_violation_penalty(missing);
      rew += pen;
      penrec += pen;  // episode.penalty_record (:549,566,584)
      miss_sum += missing;  // cum_soc_missing (:544,561,579), only reported through the data log
    } else {
      rew += d.fully_charged_reward;
    }
  }
  {
    const bool staying = (ntl != 0.0f) && (hl != 0.0f);  // still charging :593-594; otherwise no car in the next
    hl = staying ? (float)((double)hl - dt_step) : ntl;     // step :597-599 or a new arrival :602-606 (the reference's
    soc = staying ? soc : tb1.sor;                       // `else: raise` is unreachable)
  }
  if (soh0 <= 0.9) t090 = true;  // :613-614 sticky target (quirk Q7)
  o.soc_deg = (hl != 0.0f) ? soc : old_deg;  // :621-623
  o.soc = soc;
  o.hl = hl;
  o.en = en;
  o.rew = rew;
  o.penrec = penrec;
  o.miss = miss_sum;
  o.pos = pos;
  o.t090 = t090;
  o.event = ev_lane;
  return o;
}

// ---------------------------------------------------------------------------------------------------------
// the step (FleetEnv.step, fleet_environment.py:436-702)
//   MULTI = false: exactly one step per launch (the drop-in path: an observation is needed before the next action)
//   MULTI = true : K consecutive steps per launch from an action tape (open-loop rollouts); waves advance
//                  independently, so there is no per-step grid-wide synchronisation at all.
// For G == 64 a wavefront is one env: the env index, its time row and everything derived from them are made
// wave-uniform (readfirstlane), which moves row addressing and the table-row loads to the scalar unit.
// ---------------------------------------------------------------------------------------------------------
// The leading arguments of fleet_step_kernel as the kernel-argument segment lays them out (natural alignment, declaration
// order): where the argument block `d_arg` starts in the segment (`late_args`).
struct StepKernargPrefix {
  const Hot* p_hot;
  const SegRec* p_run;
  const double* p_soh;
  const void* p_actions;
  int p_E, p_N;
  EnvRec* p_env;
  FleetDev d_arg;
};
static_assert(offsetof(StepKernargPrefix, d_arg) == 48 && alignof(FleetDev) == 8, "twelve preloaded dwords, then the argument block");
// ... and the whole argument list as the kernel-argument segment holds it: what every step launch is given (step_args), field by field
// on a HIP stream, as one block in the AQL packets the library writes itself (fleet_describe_step, fleet_direct.hip).  Checked against
// the code object's metadata at load.
struct StepKernargs {
  const Hot* p_hot;
  const SegRec* p_run;
  const double* p_soh;
  const void* p_actions;
  int p_E, p_N;
  EnvRec* p_env;
  FleetDev d_arg;
  const void* actions;
  int act_mode, K;
  int outputs_dead;  // single-step instances: nonzero = nobody can read this launch's observation row (see the kernel, "Dead outputs")
  float* obs;
  double* reward;
  uint8_t* done;
  float* terminal_obs;
  int32_t* done_count;
  unsigned long long guard_bytes;  // placement record of the run this launch belongs to (see the kernel, "Placement guard"): byte k =
                                   // 0x80 | die of workgroups w with (w & 7) == k; 0 = no check (every launch through HIP)
  unsigned char* rec_blocks;       // the FIRST launch of a run on the library's own queue: the argument blocks of the run's other launches
  int rec_rows, rec_rotate;        // (rec_rows blocks, FleetStepLaunch::kBlockBytes apart), into which it writes that record; else nullptr
};
static_assert(offsetof(StepKernargs, d_arg) == offsetof(StepKernargPrefix, d_arg) && sizeof(StepKernargs) <= sizeof(FleetStepLaunch::args),
              "the argument block of a described launch");
static_assert(offsetof(StepKernargs, rec_rows) == offsetof(StepKernargs, rec_blocks) + 8 &&
                  offsetof(StepKernargs, rec_rotate) == offsetof(StepKernargs, rec_rows) + 4,
              "fleet_direct_prepare fills rec_blocks, rec_rows and rec_rotate as one 16-byte piece");

// What a K-step instance carries besides the action tape (MULTI only; round 5): the built-in policies and the event-skipping loop of
// real_time each cost the tape rollout scalar registers it spills and branches it never takes -- compiled per use, the tape-only
// instance runs 9 % faster (9.35e8 -> 1.02e9 env-steps/s at 4096x50, profiles/r05_experiments/ab11_kstep_kernel_per_mode.log).
// kModeAll = everything behind run-time tests (the data-log instances and the small groups, where instances are not multiplied).
constexpr int kModeAll = 0, kModeTape = 1, kModePolicy = 2, kModeRt = 3;

// The tail of the state-only twin (DEAD), three parts that can be compiled one by one for an A/B (-DFLEET_TWIN_TAIL=<bits> through
// fleetrl_amd.build.build_variant; EXPERIMENTS.md, "The twin's tail: one late argument fetch"); the product has all three (measured one by one and together there):
//   1  A: the rainflow row request's two scalars (rf_row_stride, stack_cap) are fetched with the entry's argument loads
//   2  B: ONE late fetch -- everything the rest of the step reads of the kernel-argument segment in one block of scalar loads, one wait
//   4  C: the env record's final stores through the preloaded `p_env`, the reset's flag re-read inside the reset branch
// The live instances never look at this.
#ifndef FLEET_TWIN_TAIL
#define FLEET_TWIN_TAIL 7
#endif
// What part B reads at the first `late_args` point and keeps in scalar registers to the end of the launch.
struct TwinLateTail { unsigned long long rec; unsigned char* blocks; int rows, rotate; };
struct TwinLate {
  int E, T;                                                  // the self-check of the hard-wired offset
  double evse_power, grid_connection, penalty_overload;      // the leader's overload test
  int auto_reset;
  unsigned long long rec; unsigned char* blocks; int rows, rotate;  // the placement guard's 24-byte piece
};

// DEAD: the state-only twin of a single-step instance ("Dead outputs" in the kernel): the same argument list, `outputs_dead` ignored --
// that nobody can read this launch's outputs is a compile-time fact.  Only for groups of whole wavefronts with one EV per lane
// (G = 64 / 128 / 256, the benchmark's shapes); only a run on the library's own queue ever launches it (fleet_direct.hip).
template <int G, int DEG, bool MULTI, bool WIDE, bool LOG = false, bool A64 = false, int MODE = kModeAll, bool DEAD = false>
__global__ __launch_bounds__(kBlock, MULTI ? (WIDE ? kMultiWideWaves : kMultiWaves) : kSingleWaves) void fleet_step_kernel(
    // The first twelve argument dwords are preloaded into scalar registers at wave launch (-amdgpu-kernarg-preload-count,
    // fleetrl_amd/build.py; twelve is what fits beside the other user registers): what the first loads of a wavefront need --
    // its lanes' state records and action, E and N for their addresses -- is passed here once more, ahead of the argument
    // block, so that those loads do not wait for an argument fetch.
    // (no __restrict__ on the state pointers: the same kernel stores to these arrays through the argument block)
    const Hot* p_hot, const SegRec* p_run, const double* p_soh, const void* __restrict__ p_actions, int p_E, int p_N, EnvRec* p_env,
    FleetDev d_arg, const void* __restrict__ actions, int act_mode, int K, int outputs_dead,
                                                               float* __restrict__ obs, double* __restrict__ reward,
                                                               uint8_t* __restrict__ done, float* __restrict__ terminal_obs,
                                                               int32_t* __restrict__ done_count, unsigned long long guard_bytes,
                                                               unsigned char* __restrict__ rec_blocks, int rec_rows, int rec_rotate) {
  FLEET_STAMP_RT(9);
  FLEET_STAMP(0);
  // The argument block is ~150 dwords of scalars for ~100 scalar registers.  One step per launch, one EV per lane: what the END
  // of the step needs of it (the tail store's geometry, the leader lane's constants and pointers, the head bookkeeping) is
  // re-read from the kernel-argument segment after the lane's EV is done -- scalar loads through the constant cache, behind a
  // laundered pointer so that they are not hoisted back to the entry -- instead of being fetched at entry and carried over the
  // whole step in lanes of a vector register (24 v_writelane + 22 v_readlane on every wavefront's path before; none now).
  // Re-reading in the MIDDLE of the EV's step instead stalls on those loads (+0.3 us at 2048 envs) and re-reading everything at
  // several points costs +0.7 us (profiles/r04_experiments/args_reloaded_*).  `late_args_ok` guards the hard-wired offset.
  static_assert(!DEAD || (!MULTI && !WIDE && !LOG && G >= 64 && MODE == kModeAll), "the state-only twin: one step, one EV per lane, whole wavefronts");
  const FleetDev& d = d_arg;
  // (not the rainflow twins with float64 actions: they sit at the scalar register limit, two scalars in lanes, and the late block would
  // put two more there; they keep the live instance's tail)
  constexpr bool kTail = DEAD && !(A64 && DEG == FLEET_DEG_RAINFLOW);
  constexpr bool kTailA = kTail && DEG == FLEET_DEG_RAINFLOW && (FLEET_TWIN_TAIL & 1) != 0;
  constexpr bool kTailB = kTail && (FLEET_TWIN_TAIL & 2) != 0;
  constexpr bool kTailC = kTail && (FLEET_TWIN_TAIL & 4) != 0;
  // The twin's lane body has no exec-mask region around it: every lane runs it, lanes g >= N on the env's last EV with their stores,
  // their rainflow push and their sums switched off.  One path through the body for the wait-count pass: behind it nothing of the first
  // burst is pending any more, and no `s_waitcnt vmcnt` stands between the body's stores and the env record's (EXPERIMENTS.md, "The
  // twin's lane body on one path").  The same instances as `kTail`; the live instances keep the masked region.
  constexpr bool kBody = kTail;
  typedef const __attribute__((address_space(4))) char* karg_ptr;
  auto late_args = [&]() -> const FleetDev& {
    if constexpr (!MULTI && !WIDE) {
      karg_ptr kp = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(StepKernargPrefix, d_arg);
      asm volatile("" : "+s"(kp));
      return *(const FleetDev*)(const __attribute__((address_space(4))) FleetDev*)kp;
    } else {
      return d_arg;
    }
  };
  // (B) the twin launders ONE pointer, at the first late point (`late_args_once`); the second late scope and the placement guard read
  // through the same one (`late_args_same`)
  karg_ptr late_kp = nullptr;
  auto late_args_once = [&]() -> const FleetDev& {
    late_kp = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(StepKernargPrefix, d_arg);
    asm volatile("" : "+s"(late_kp));
    return *(const FleetDev*)(const __attribute__((address_space(4))) FleetDev*)late_kp;
  };
  auto late_args_same = [&]() -> const FleetDev& { return *(const FleetDev*)(const __attribute__((address_space(4))) FleetDev*)late_kp; };
  TwinLate lt = {0, 0, 0.0, 0.0, 0.0, 0, 0ull, nullptr, 0, 0};
  uint32_t late_bad = 0;  // kTailB: nonzero = the argument block is not where `late_args` assumes it
  constexpr bool kPol = MULTI && (MODE == kModeAll || MODE == kModePolicy);  // the built-in policies are compiled in
  constexpr bool kRt = MULTI && (MODE == kModeAll || MODE == kModeRt);       // the event-skipping loop is compiled in
  // `p_N`: EVs per env in the low half; in the high half the workgroup this launch's grid starts at -- 0 for every launch through HIP;
  // a run on the library's own queues may cover the batch with two grids on two queues (fleet_direct.hip), and the second grid's
  // workgroups continue the first one's numbering.  (Here because it is needed before the first load: p_N is a preloaded argument.)
  const int N = p_N & 0xffff, E_ = p_E;
  const int wg_base = (int)((unsigned)p_N >> 16);
  const int g = threadIdx.x % G;
  const bool leader = (g == G - 1);
  int e_raw = ((int)blockIdx.x + wg_base) * (kBlock / G) + threadIdx.x / G;
  if (G >= 64) e_raw = __builtin_amdgcn_readfirstlane(e_raw);
  const bool env_ok = e_raw < E_;  // surplus groups of the last block run the arithmetic on env E-1 but store nothing
  const int e = env_ok ? e_raw : E_ - 1;

  // One launch = one step and one EV per lane (N <= G): everything the lane needs to start its arithmetic -- its state
  // records, the schedule record of the row the step advances to, its action -- has an address that does not depend on
  // the env's time row, so it is requested before the env record is even read.
  constexpr bool kEarly = !MULTI && !WIDE;
  Hot h_pre = {0.0, 0.0f, 0u};
  SegRec run_pre = {0.0, 0u, 0u};
  double soh_pre = 0.0;
  float a32_pre = 0.0f;
  double a64_pre = 0.0;
  if (kEarly) {
    // unconditional, straight-line requests (surplus lanes of the group re-read the env's last EV and drop it): no
    // exec-mask region for the compiler to close with a wait before the env record is even requested
    const EvIx i0 = {(size_t)e * N, (unsigned)(g < N ? g : N - 1)};
    // in the order the step consumes them (the memory system serves the chip-wide burst of these requests roughly first
    // come, first served, and a wavefront's wait counts its loads in issue order): what the charge arithmetic needs first
    // (full 64-bit lane addresses here: with scalar bases the four requests leave ~1 % later -- each base is a dependent
    // chain on the one scalar unit --, profiles/r03_experiments/ab_saddr.log)
    const size_t f0 = i0.flat();
    h_pre = p_hot[f0];
    soh_pre = p_soh[f0];
    if (A64) a64_pre = ((const double*)p_actions)[f0];
    else a32_pre = ((const float*)p_actions)[f0];
    run_pre = p_run[f0];
  }

  EnvHead r = p_env[e].h;
  if (G >= 64) {
    r.t = __builtin_amdgcn_readfirstlane(r.t);
    r.t_end = __builtin_amdgcn_readfirstlane(r.t_end);
    r.nsamp = __builtin_amdgcn_readfirstlane(r.nsamp);
    r.episodes = __builtin_amdgcn_readfirstlane(r.episodes);
  }
  const uint32_t head_flags = HEAD_FLAGS(r.nsamp);  // FLEET_TFLAG_* of row t + 1, left by the previous launch
  // is the sample this step logs still counted?  (EnvRec::rf_until: nothing reads what is logged after the episode's last
  // degradation row.)  One step per launch: bit 29 of the head, left by the previous launch's leader, who alone holds the row
  // itself; K steps per launch: every lane holds the row and compares per step.
  const bool head_live = HEAD_LIVE(r.nsamp);
  r.nsamp = HEAD_NSAMP(r.nsamp);
  double ep_return = 0.0, penalty_record = 0.0;
  int ep_len = 0;
  int rf_until = -1;
  if (leader) {
    const EnvRec* er = d.env + e;
    ep_return = er->ep_return;
    penalty_record = er->penalty_record;
    ep_len = er->ep_len;
    if (DEG == FLEET_DEG_RAINFLOW && !MULTI) rf_until = er->rf_until;
  }
  // (A) what rf_begin's row request and rf_finish_win read of the argument block: fetched with the entry's argument loads, under the
  // wait for the head, so that nothing scalar stands between the push decision and the four row loads.  An input of an opaque asm:
  // the fetch cannot sink to its use.  Behind the leader's loads: the compiler takes a volatile asm for a store, and a uniform load
  // behind it is no longer a scalar one.
  if constexpr (kTailA) asm volatile("" ::"s"(d_arg.rf_row_stride), "s"(d_arg.stack_cap));
  // (the same for rf_finish_win's stress_temp: the float32 rainflow twins only, as `kRfDeep` below)
  if constexpr (DEAD && !A64 && DEG == FLEET_DEG_RAINFLOW) asm volatile("" ::"s"(d_arg.stress_temp));
  if (DEG == FLEET_DEG_RAINFLOW && MULTI) {
    rf_until = p_env[e].rf_until;
    if (G >= 64) rf_until = __builtin_amdgcn_readfirstlane(rf_until);
  }
  uint32_t err = 0;
  double reward_sum = 0.0;
  int n_done = 0;
  float* const obs_row = obs + (size_t)e * d.obs_dim;
  float* const term_row = terminal_obs ? terminal_obs + (size_t)e * d.obs_dim : nullptr;
  const int steps = MULTI ? K : 1;
  // Dead outputs (single-step launches on the library's own queue, fleet_direct.hip).  Nothing a run on that queue writes is visible
  // before its last packet has retired, and every launch writes the same observation rows: what any launch but the last stores
  // there is overwritten before anybody can read it.  Those launches carry `outputs_dead` != 0 -- a kernel argument, the same for
  // every wavefront, fetched with the arguments the entry reads anyway -- and skip what feeds only the row: write_obs_ev with the
  // arithmetic of its auxiliary slots, the request for the tail row and its store, the terminal row.  With one EV per lane (`kEarly`)
  // such a launch does state work only: it stores neither `reward[e]` nor `done[e]` nor EnvRec::cashflow -- every step overwrites all
  // three, and only the last launch's values can be read --, feeds the cashflow fold a zero, and its auto-reset writes no start row
  // (the run's last launch writes every env's row).  State -- the EV records, rainflow and SEI, head, ep_return, penalty_record,
  // ep_len, the episode-end records --, the error bits and the placement guard are as ever.  Launches through HIP always carry 0;
  // the K-step instances (the data log among them) decide per step themselves and do not look.
  // The state-only twin (DEAD) is the same launch with the answer compiled in: no observation or terminal row addressing, no tail
  // request, no cashflow arithmetic (the fold's first sum is a literal zero), no leader store block, no start row from the reset --
  // and none of the registers, masks and scalar instructions that carry the run-time test through the step.
  const bool obs_live = DEAD ? false : (MULTI || outputs_dead == 0);
  const int vzero = (int)__builtin_amdgcn_mbcnt_lo(0u, 0u);  // 0 in every lane, opaque to the uniformity analysis
  // night-charging policy: the env's "charging since" row travels in a register over the K steps
  int night_st = FLEET_NIGHT_IDLE;
  if (kPol && act_mode == FLEET_ACT_POLICY_NIGHT) {
    night_st = d.cold->night_start[e];
    if (G >= 64) night_st = __builtin_amdgcn_readfirstlane(night_st);
  }

  // data log cursor of the env (rows written so far), carried in a register over the launch's steps.  The logging code lives
  // in an instance of its own (LOG, multi-step form; the launcher routes every launch of a logging batch to it), so the
  // kernels of the hot path pay nothing for it -- neither instructions nor registers.
  static_assert(!LOG || MULTI, "the data log is compiled into the multi-step kernel only");
  constexpr bool log_on = LOG;
  int lp = log_on ? d.log_pos[e] : 0;
  if (G >= 64) lp = __builtin_amdgcn_readfirstlane(lp);

  // real_time (event-skipping, fleet_environment.py:453,692-699): the launch repeats the step with the same action until
  // a relevant event happened; it reports the LAST pass's observation / reward / done.  Multi-step kernel, K == 1.
  const bool rt = kRt && (d.real_time != 0);
  // K steps per launch, one EV per lane: the head of the EV's rainflow row (closed-cycle count, sum of means, rainflow_length,
  // the two newest stack entries) is read ONCE per launch and carried in registers over the K steps -- a push updates the
  // registers and stores to the row, nothing re-reads it; the stack words are only read when a closure pops into them
  constexpr bool kRfCarry = MULTI && !WIDE && DEG == FLEET_DEG_RAINFLOW;
  // (Carrying the EV's state record, its state of health and the schedule record the same way was measured and is NOT done:
  // -14 % K-step rate -- the kernel is at the 128-register limit of four resident wavefronts per SIMD, the six extra live
  // registers spill, and those loads overlap with other wavefronts' arithmetic anyway;
  // profiles/r03_experiments/ab_stcarry.log.)
  RfAccHead acc_c = {0.0, 0, 0};
  RfTop top_c = {0.0, 0.0};
  auto carry_load = [&]() {
    const EvIx i0 = {(size_t)e * N, (unsigned)(g < N ? g : N - 1)};
    const double* row = rf_row_of(d, i0);
    acc_c = *reinterpret_cast<const RfAccHead*>(row);
    top_c = *reinterpret_cast<const RfTop*>(row + 2);
  };
  if (kRfCarry) carry_load();
  double last_rew = 0.0;
  bool last_done = false;
  uint32_t head_after = 0;   // single step: FLEET_TFLAG_* of the row after the one the launch advances to
  bool head_reset = false;   // the env was reset in this launch: its head describes the new start row
  for (int k = 0; rt || k < steps; ++k) {
    const int t = r.t;
    int t1 = t + 1;  // :508
    if (t1 > d.T - 1) { t1 = d.T - 1; err |= FLEET_DEVERR_TABLE_END; }
    const int t2 = t1 + 1 > d.T - 1 ? d.T - 1 : t1 + 1;  // the row the NEXT step advances to
    const bool is_done = (t + 1 == r.t_end);  // :627-628 -- the step that finishes the episode
    // episode.done as step() returns it (:702): sticky until the next reset.  Only without auto-reset can a step start at or past
    // the finish row (t_end = -1, an irregular-grid episode that never ends, compares as the largest row).
    const bool done_now = is_done || (!d.auto_reset && (uint32_t)(t + 1) > (uint32_t)r.t_end);
    const bool resets = is_done && d.auto_reset;
    const bool rf_live = MULTI ? (t < rf_until) : head_live;  // the sample of row t + 1 is counted
    // where this step's observation goes: with vec-env auto-reset the terminal observation is reported aside
    float* const step_row = resets ? term_row : obs_row;
    // intermediate steps of a K-step launch only need their observation when the episode ends (terminal observation)
    const bool write_step_obs = obs_live && env_ok && (step_row != nullptr) && (!MULTI || rt || resets || k == steps - 1);

    FLEET_STAMP(1);
    // ---- loads that depend on the time row: the row's physics scalars and observation tail -----------------------------
    // The 72-byte row is wave-uniform for G == 64, but keeping it in scalar registers for the whole lane loop costs 16
    // of the ~100 SGPRs (spills); a deliberately lane-indexed (vzero == 0) load puts it in vector registers instead.
    // (not in rainflow mode, where vector registers are the scarcer resource)
    // One step per launch: requested as a lane-indexed (vector) load when the head arrives and consumed last -- by the money
    // terms, after the state machine and the observation stores -- so that no wait on the scalar side stands between the
    // arrival of the state records and the charge arithmetic; the row flags the state machine needs come with the head.
    const PhysHot ph = *reinterpret_cast<const PhysHot*>(d.tab_phys + (t + ((kEarly || DEG != FLEET_DEG_RAINFLOW) ? vzero : 0)));
    // flags of the row after t1, for the head the next launch reads
    uint32_t flags_after = 0;
    if (kEarly) flags_after = reinterpret_cast<const PhysHot*>(d.tab_phys + (t1 + vzero))->flags_next;
    // hours this step spans: `get_next_dt` (:455, :994-1008) -- a constant unless the grid is irregular (real_time only)
    const double dt_step = rt ? d.tab_phys[t].dt : d.dt;
    const uint32_t flags1 = kEarly ? head_flags : ph.flags_next;
    const bool lunch = d.is_caretaker && (flags1 & FLEET_TFLAG_LUNCH);
    const bool deg_row = (DEG != FLEET_DEG_NONE) && (flags1 & FLEET_TFLAG_DEG);
    // the few wavefronts with extra work after the step (daily evaluation, episode end + reset) finish last and set the
    // launch's duration: they get issue priority over their SIMD's other wavefronts for the step itself (-3 % per launch)
    if (!MULTI && G >= 64 && ((DEG == FLEET_DEG_RAINFLOW && deg_row) || is_done)) __builtin_amdgcn_s_setprio(3);
    const size_t abase = ((size_t)(rt ? 0 : k) * d.E + e) * N;

    // data log: the step's row (not written for the step that ends the episode nor for any step past it, :679: `episode.done` is
    // sticky) -- its observation goes to the log's own buffer, so K-step launches log every step although they only return the
    // last observation
    const bool logs = log_on && env_ok && !done_now;
    const size_t lrow = logs ? (size_t)(lp % d.log_cap) * d.E + e : 0;
    float* const log_obs_row = logs ? d.log_obs + lrow * d.obs_dim : nullptr;

    const float tail_first = (write_step_obs || logs) ? tail_load<G>(d, t1, g) : 0.0f;  // consumed after the lane loop

    // Multi-step launches: an opaque per-iteration zero keeps the compiler from hoisting every lane address of the step
    // body out of the K loop (60 extra live vector registers = half the resident wavefronts); recomputing them each
    // step costs a handful of integer instructions.
    int kz = 0;
    if (MULTI) asm volatile("" : "+v"(kz));

    // Which action rule applies to this env in this step (policies only; FLEET_ACT_POLICY_NIGHT resolves to one of
    // "all zeros" / "all ones" / the distributed rule per step, benchmarking/night_charging.py:81-98)
    int pol = act_mode;
    if (kPol && act_mode == FLEET_ACT_POLICY_NIGHT) {
      const FleetCold* cd = d.cold;
      const int hm = cd->tab_hm[t];
      const int hour = hm >> 8, minute = hm & 255;
      if (d.is_caretaker && hour >= 11 && hour <= 14) {
        pol = FLEET_ACT_POLICY_DISTRIBUTED;  // :85-88, `continue`: the window bookkeeping below is skipped
      } else {
        bool charging = (night_st != FLEET_NIGHT_IDLE);
        if ((cd->night_hour <= hour && cd->night_minute <= minute) || charging) {  // :90
          if (!charging) night_st = t;  // charging_start = copy(time) :91-92
          charging = true;
          pol = FLEET_ACT_POLICY_UNCONTROLLED;  // np.ones :94
        } else {
          pol = -1;  // np.zeros :96
        }
        // :97-98  (time - charging_start).total_seconds() / 3600 > int(max_time_needed); rows are a regular grid
        if (charging && (t - night_st) * cd->step_s > cd->night_limit_s) night_st = FLEET_NIGHT_IDLE;
      }
    }

    double cash = 0.0, rew = 0.0, asum = 0.0, penrec = 0.0, miss_sum = 0.0;
    // what the daily SEI pass needs of the lane's EV, carried in registers when a lane owns one EV (no reload round trip for
    // the few wavefronts on the 14:45 row, which otherwise finish last and set the launch's duration)
    double sei_sample = 0.0, sei_soh = 0.0;
    int sei_tail = 0;
    RfTop sei_top = {0.0, 0.0};
    bool sei_have_top = false;
    bool ev_lane = false;  // real_time: something the reference counts into episode.events happened to this lane's EVs
    // Several EVs per lane, one step per launch (N > 64): the lane's NEXT EV's records are requested before the current EV is
    // worked on (software pipelining of the lane loop) -- otherwise every turn of the loop starts with a memory round trip
    constexpr bool kPipe = WIDE && !MULTI;
    // a launch whose outputs nobody can read does state work only ("Dead outputs" above; `if constexpr`, so that the other instances
    // compile to what they always did)
    constexpr bool kStateOnly = kEarly;
    Hot hb_n = {0.0, 0.0f, 0u};
    SegRec rr_n = {0.0, 0u, 0u};
    double soh_n = 0.0, act_n = 0.0;
    auto request_ev = [&](int cn) {
      const int cc = cn < N ? cn : N - 1;  // past the end: a harmless re-read of the last EV (no exec-mask region)
      const EvIx in = {(size_t)e * N, (unsigned)cc}, ia = {abase, (unsigned)cc}, it = {(size_t)t1 * N, (unsigned)cc};
      hb_n = *ev_at(d.hot, in);
      soh_n = *ev_at(d.soh, in);
      act_n = (act_mode == FLEET_ACT_F64) ? *ev_at((const double*)actions, ia) : (double)*ev_at((const float*)actions, ia);
      rr_n = *ev_at(d.seg, it);
    };
    if (kPipe) request_ev(g);
    // (the twin: no exec-mask region around the body.  Every lane runs it, a surplus lane (g >= N) on the env's last EV, whose records
    // the early loads handed it; `ev_ok` keeps it from storing, from the rainflow push and from the table read of `crosses`)
    const bool lane_ok = kBody ? g < N : true;
    const bool ev_ok = kBody ? (env_ok && lane_ok) : env_ok;
    for (int c = kBody ? (g < N ? g : N - 1) : g + kz; kBody || c < N; c += G) {
      const EvIx i = {(size_t)e * N, (unsigned)c};
      // all loads of this EV are issued before anything is consumed
      const Hot hb = kEarly ? h_pre : (kPipe ? hb_n : *ev_at(d.hot, i));
      // schedule record of row t1: carried with the state (one step per launch) or read from the table (K steps / several EVs
      // per lane: the time row is in registers there, the table read is not on anybody's critical path, and the carried
      // record is rewritten once, when the launch ends)
      const EvIx it1 = {(size_t)t1 * N, (unsigned)c};  // the table row the step advances to
      const SegRec rr = kEarly ? run_pre : (kPipe ? rr_n : *ev_at(d.seg, it1));
      const double soh0 = kEarly ? soh_pre : (kPipe ? soh_n : *ev_at(d.soh, i));
      const double act_cur = act_n;
      if (kPipe) request_ev(c + G);
      // last logged SOC sample: shares the record's float64 field with the SOC (struct Hot); the soc_deg plane only holds
      // it in a combination that does not occur inside the reference's episodes (dependent load, INPLANE)
      const bool inplane = HOT_INPLANE(hb.bits);
      double old_deg = hb.x;
      if (inplane) old_deg = d.soc_deg[i.flat()];
      RfReq rq;
      rq.push = false;
      constexpr bool kRfEarly = MULTI && DEG == FLEET_DEG_RAINFLOW;
      rq.win = false;
      if (kRfCarry) {
        rq.acc = acc_c;
        rq.top = top_c;
      } else if (kRfEarly && env_ok && rf_live) {
        rf_request(d, i, HOT_TAIL(hb.bits), rq);
      }
      double a;
      if (kPol && act_mode >= FLEET_ACT_POLICY_UNCONTROLLED) {
        // built-in open-loop policies of the reference's benchmark harnesses, evaluated in place of an action tape
        if (pol == FLEET_ACT_POLICY_UNCONTROLLED) {
          a = 1.0;  // benchmarking/uncontrolled_charging.py:51-54: np.ones(n_evs)
        } else if (pol < 0) {
          a = 0.0;
        } else {
          // benchmarking/distributed_charging.py:50-54: clip(get_dist_factor(), 0, 1), get_dist_factor =
          // hours_needed / (hours_left + 0.001) from the TABLE row of the current time (fleet_environment.py:782-799)
          const RowRec tb0 = seg_row(d.seg[(size_t)t * N + c], t, d.dt);
          const FleetCold* cd = d.cold;
          const double th0 = (double)tb0.there;
          const double cl0 = (HOT_T090(hb.bits) ? 0.9 : d.target_soc) * th0 - tb0.sor;
          const double hn0 = cl0 * cd->batt_cap_nominal / cd->hn_denominator;
          const double f = hn0 / ((double)tb0.tl + 0.001);
          a = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
        }
      } else if (kEarly) {
        // the widening must stay here: hoisted into the early-load block it would wait for every outstanding load
        float a32 = a32_pre;
        asm volatile("" : "+v"(a32));
        a = A64 ? a64_pre : (double)a32;
      } else if (kPipe) {
        a = act_cur;
      } else {
        const EvIx ia = {abase, (unsigned)c};
        a = (act_mode == FLEET_ACT_F64) ? *ev_at((const double*)actions, ia) : (double)*ev_at((const float*)actions, ia);
      }
      // the schedule record of the row AFTER next, for the next launch: only when that row starts a new segment of the EV's
      // schedule (a departure, an arrival, ...).  Nothing in this step waits for it except the store at its very end.
      const bool crosses = kEarly && (kBody ? lane_ok : true) && (t1 + 1 >= SEG_END(rr.se));
      SegRec nr = rr;
      const EvIx it2 = {(size_t)t2 * N, (unsigned)c};
      if (crosses) nr = *ev_at(d.seg, it2);
      const RowRec tb1 = seg_row(rr, t1, d.dt);
      FLEET_STAMP(2);
      const EvPhys ph_ev = ev_physics<kRt>(d, hb, old_deg, tb1, soh0, a, dt_step, lunch);
      double soc = ph_ev.soc;
      float hl = ph_ev.hl;
      const bool t090 = ph_ev.t090, pos = ph_ev.pos;
      const double en = ph_ev.en, soc_deg = ph_ev.soc_deg;
      rew += ph_ev.rew;
      penrec += ph_ev.penrec;
      miss_sum += ph_ev.miss;
      asum += ph_ev.a_th;
      if (kRt) ev_lane = ev_lane || ph_ev.event;
      // ---- SOC log (:655): the new sample of the streaming rainflow; what a cycle closure needs of the EV's row is requested
      // here and consumed after the observation stores and the money terms
      int tail = HOT_TAIL(hb.bits), sgn = HOT_SGN(hb.bits);
      // (K steps per launch: request and consumption stay together -- the registers the request holds across the observation
      // stores would cost the multi-step kernel a resident wavefront per SIMD)
      // (the state-only twin with float32 actions: the deep request, for rf_finish_win's second closure)
      constexpr bool kRfDeep = kEarly && DEAD && !A64;
      constexpr bool kSplitRf = !MULTI;
      if (kSplitRf && DEG == FLEET_DEG_RAINFLOW && ev_ok && rf_live) rf_begin(d, i, old_deg, soc_deg, tail, sgn, rq, false, kRfDeep);

      FLEET_STAMP(3);
      // ---- observation of the advanced time row (fleet_environment.py:511-518, 645-652) ------------------------
      const double tgt_obs = t090 ? 0.9 : d.target_soc;  // the target the observer sees: after this step's sticky update
      if (write_step_obs) write_obs_ev(d, step_row, c, soc, hl, tgt_obs, tb1);
      if (logs) write_obs_ev(d, log_obs_row, c, soc, hl, tgt_obs, tb1);

      // ---- money terms of EvCharger.charge: the only consumers of the time row's physics record, which was requested when
      // the env head arrived and has had the charge arithmetic, the state machine and the observation stores to get here
      {
        const double grid_e = fmax(en - ph.pv_share, 0.0);  // :142 (charging only)
        if constexpr (kStateOnly) {
          if (obs_live) cash += pos ? -(grid_e * ph.k_cost) : en * ph.k_rev;  // dead: a zero goes into the fold, same shape
        } else {
          cash += pos ? -(grid_e * ph.k_cost) : en * ph.k_rev;       // -charging_cost :149 / +discharging_revenue :196-199
        }
        rew += pos ? ph.k_charge * grid_e : ph.k_discharge * en;   // :154-156 / :204-206
      }

      FLEET_STAMP(4);
      // ---- SOC log + daily degradation (:655-673) -------------------------------------------------------------
      if (!kSplitRf && DEG == FLEET_DEG_RAINFLOW && env_ok && rf_live) rf_begin(d, i, old_deg, soc_deg, tail, sgn, rq, kRfEarly);
      ev_finish<DEG, WIDE>(d, i, c, N, ev_ok, deg_row, dt_step, rq, tail, sgn, soc, soc_deg, old_deg, hl, tb1.there, t090, inplane,
                           crosses, nr, soh0, a, en, logs, lrow, hb, err, sei_sample, sei_soh, sei_tail, sei_top, sei_have_top, acc_c,
                           top_c, kRfCarry, kEarly, kRfDeep);
      if (!WIDE) break;  // N <= G: a single pass, and no loop for the compiler to hoist rare-path constants out of
    }
    if constexpr (kBody) {  // a surplus lane adds what it added when it skipped the body: nothing
      rew = lane_ok ? rew : 0.0;
      asum = lane_ok ? asum : 0.0;
      penrec = lane_ok ? penrec : 0.0;
    }
    {  // ---- the rest of the step reads the argument block afresh (see `late_args`) ----
    const FleetDev& d = kTailB ? late_args_once() : late_args();
    if constexpr (kTailB) {
      // (B) everything the rest of the step reads of the kernel-argument segment on its common path, requested here in one block
      // through the one laundered pointer; the wait is behind the fold (the asm below)
      typedef const __attribute__((address_space(4))) TwinLateTail* tail_ptr;
      const TwinLateTail& tl = *(const TwinLateTail*)(tail_ptr)(late_kp + (offsetof(StepKernargs, guard_bytes) - offsetof(StepKernargPrefix, d_arg)));
      lt.E = d.E;
      lt.T = d.T;
      lt.evse_power = d.evse_power;
      lt.grid_connection = d.grid_connection;
      lt.penalty_overload = d.penalty_overload;
      lt.auto_reset = d.auto_reset;
      lt.rec = tl.rec;
      lt.blocks = tl.blocks;
      lt.rows = tl.rows;
      lt.rotate = tl.rotate;
      __builtin_amdgcn_sched_barrier(0);  // the block of loads is issued in FRONT of the fold and flies under it
    } else {
      if (!MULTI && !WIDE && (d.T != d_arg.T || d.E != p_E)) err |= FLEET_DEVERR_INTERNAL;  // the block is not where it is assumed to be
    }
    if (write_step_obs) tail_store<G>(d, step_row, t1, g, tail_first);
    if (logs) tail_store<G>(d, log_obs_row, t1, g, tail_first);
    if (DEG != FLEET_DEG_NONE) r.nsamp += 1;

    FLEET_STAMP(6);
    // ---- per-env reductions; totals land in the leader lane ---------------------------------------------------
    if (G >= 64) {
      wave_sum4_to_last(cash, rew, asum, penrec);  // this wavefront's lanes: totals in its last lane
      if constexpr (kTailB) {  // the one wait for the late fetch: every field is an input here, so none of the loads sinks to its use
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::"s"(lt.E), "s"(lt.T), "s"(lt.evse_power), "s"(lt.grid_connection), "s"(lt.penalty_overload), "s"(lt.auto_reset),
                     "s"(lt.rec), "s"(lt.blocks), "s"(lt.rows), "s"(lt.rotate));
        late_bad = (uint32_t)(lt.T ^ d_arg.T) | (uint32_t)(lt.E ^ p_E);  // no branch; OR-ed into `err` where the guard is
      }
      if (G > 64) {
        // an env of several wavefronts: their partial sums meet in the LDS and the group's last lane adds them in wavefront order
        // (K steps per launch: the env's wavefronts meet here once per step -- every wavefront of the workgroup runs the same K
        // steps, so the barrier is uniform; two buffers in turn, so that a wavefront already in the next step does not overwrite
        // what the leader is still adding up.  The event-skipping loop of real_time has env-dependent trip counts: never here.)
        __shared__ double s_part[2][kBlock / 64][4];
        double(*part)[4] = s_part[MULTI ? (k & 1) : 0];
        const int w = (int)threadIdx.x / 64;
        if ((threadIdx.x & 63) == 63) {
          part[w][0] = cash;
          part[w][1] = rew;
          part[w][2] = asum;
          part[w][3] = penrec;
        }
        __syncthreads();
        if (leader) {
          const int w0 = ((int)threadIdx.x / G) * (G / 64);
          double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
          for (int j = 0; j < G / 64; ++j) {
            s0 += part[w0 + j][0];
            s1 += part[w0 + j][1];
            s2 += part[w0 + j][2];
            s3 += part[w0 + j][3];
          }
          cash = s0;
          rew = s1;
          asum = s2;
          penrec = s3;
        }
      }
    } else {
      cash = group_sum_to_last<G>(cash);
      rew = group_sum_to_last<G>(rew);
      asum = group_sum_to_last<G>(asum);
      if (__any(penrec != 0.0)) penrec = group_sum_to_last<G>(penrec);  // wave-uniform branch; rare
    }
    if (log_on) miss_sum = group_sum_to_last<G>(miss_sum);  // kernel-argument-uniform branch (log_data only)
    r.t = t1;
    if (leader) {
      penalty_record += penrec;
      // LoadCalculation.check_violation (load_calculation.py:93) and the sigmoid penalty (:496-502)
      const double grid_connection = kTailB ? lt.grid_connection : d.grid_connection;
      const double head_room = grid_connection - ph.load - asum * (kTailB ? lt.evse_power : d.evse_power) + ph.pv;
      const double over = fabs(head_room < 0.0 ? head_room : 0.0);
      if (over > 0.0) {
        const double pen = overloading_penalty(over / grid_connection + 1.0, kTailB ? lt.penalty_overload : d.penalty_overload);
        rew += pen;
        penalty_record += pen;
        if (kRt) ev_lane = true;  // :499
      }
      if (logs) {
        d.log_row[lrow] = t1;  // episode.time
        double* le = d.log_env + lrow * 4;
        le[0] = rew;
        le[1] = cash;
        le[2] = over;      // grid = abs(overload_amount) (:660)
        le[3] = miss_sum;  // soc_v = abs(cum_soc_missing) (:661)
      }
      ep_return += rew;  // :637
      ep_len += 1;
      reward_sum += rew;
      last_rew = rew;
      if constexpr (kStateOnly) {
        if (env_ok && obs_live) {  // (a dead launch's three values are overwritten unseen)
          d.env[e].cashflow = cash;
          reward[e] = rew;
          done[e] = done_now ? 1 : 0;
        }
      } else if (env_ok) {
        d.env[e].cashflow = cash;  // cashflow = -charging_cost + discharging_revenue (ev_charger.py:225)
        if (!MULTI) {
          reward[e] = rew;
          done[e] = done_now ? 1 : 0;
        }
      }
    }
    FLEET_STAMP(7);
    // ---- daily SEI evaluation (:666-671) ---------------------------------------------------------------------
    // Runs in a second pass over the group's EVs, after the per-step arithmetic has retired, so that its temporaries
    // (transcendentals, accumulators) never coexist with the hot path's registers.  One step in 96, and wave-uniform for
    // G == 64.
    if (DEG == FLEET_DEG_RAINFLOW && deg_row && env_ok) {
      for (int c = g; c < N; c += G) {
        const EvIx ix = {(size_t)e * N, (unsigned)c};
        const size_t i = ix.flat();
        double deg, soh_new;
        if (!WIDE) {
          // (its scalars from the argument block the end of the step has just re-read, not from the device-resident copy: one
          // dependent round trip less on the wavefronts that end the launch, -2 % per launch at 4096 x 50)
          deg = sei_evaluate(d, ix, sei_sample, r.nsamp, sei_tail, sei_top, sei_have_top, err, dt_step,
                             kRfCarry ? &acc_c.rf_len : nullptr);
          soh_new = sei_soh - deg;
        } else {  // several EVs per lane: re-read the few words from the records this lane has just stored
          const Hot hb = d.hot[i];
          const double sample = HOT_INPLANE(hb.bits) ? d.soc_deg[i] : hb.x;
          const RfTop none = {0.0, 0.0};
          deg = sei_evaluate(*d.self, ix, sample, r.nsamp, HOT_TAIL(hb.bits), none, false, err, dt_step);
          soh_new = d.soh[i] - deg;
        }
        d.soh[i] = soh_new;
        if (logs) {
          double* lev = d.log_ev + lrow * 4 * N + c;
          lev[2 * N] = deg;
          lev[3 * N] = soh_new;
        }
        if (!WIDE) break;
      }
    }
    if (logs) lp += 1;
    head_after = flags_after;
    if (is_done) {
      n_done += 1;
      if (leader && env_ok) {
        EnvRec* er = d.env + e;
        er->last_ep_return = ep_return;
        d.cold->last_len[e] = ep_len;
        er->start_done |= (int32_t)0x80000000u;  // episode.done
      }
      r.episodes += 1;
      if (kTailB ? (lt.auto_reset != 0) : resets) {  // (inside `is_done`)
        head_reset = true;
        if (env_ok) {
          if constexpr (kStateOnly) reset_env<G, LOG>(*d.self, e, g, leader, r, obs_live ? obs_row : nullptr, lp, rf_until);
          else reset_env<G, LOG>(*d.self, e, g, leader, r, obs_row, lp, rf_until);
          if (kRfCarry) carry_load();  // the reset rewrote the row's head (same lane, same addresses: program order holds)
        } else {  // surplus group: keep its registers moving without touching memory
          r.t = choose_start(d.cold, d.E, e, r.episodes);
          r.t_end = d.tab_finish ? d.tab_finish[r.t] : r.t + d.episode_steps;
          r.nsamp = (DEG != FLEET_DEG_NONE) ? 1 : 0;
        }
        ep_return = 0.0;
        ep_len = 0;
        penalty_record = 0.0;
        if constexpr (kTailC) {
          // (C) the new start row's flags for the head, read AND waited for here, in the rare branch, so that the common path does
          // not join behind a pending load of the reset's.  (The drain in front of the env record's stores that this alone left --
          // for the flags and the time row's leader terms of the FIRST burst, pending on the path around the lane loop's body --
          // went with that path: `kBody`.)
          head_after = d.tab_phys[r.t].flags_next;
          asm volatile("" : "+v"(head_after));
        }
      }
    }
    last_done = done_now;
    if (rt) {
      // EventManager.check_event (event_manager.py:16-31): the advanced row's clock minute == 15 is an event of its own;
      // the end of the episode is one (:629) -- a step past it is not; running off the table ends the loop (the reference
      // would raise there)
      const int hm1 = d.cold->tab_hm[t1];
      const bool minute15 = ((hm1 & 255) == 15) && !(hm1 & 0x8000);  // minute == 15 and second == 0
      if (group_any<G>(ev_lane) || is_done || minute15 || (t + 1 > d.T - 1)) break;
    }
    }  // late_args scope
  }

  {  // ---- after the steps: again through the freshly read block ----
  const FleetDev& d = kTailB ? late_args_same() : late_args();
  // (only where a single-step launch that reads them can follow on the same handle: `carry_run`, i.e. up to kMaxGroup EVs per env)
  if (!kEarly && (!WIDE || d.carry_run) && env_ok) {  // the carried schedule records: the row the NEXT launch advances to
    const int rn = r.t + 1 > d.T - 1 ? d.T - 1 : r.t + 1;
    for (int c = g; c < N; c += G) d.run[(size_t)e * N + c] = d.seg[(size_t)rn * N + c];
  }
  if (leader && env_ok) {
    EnvRec* er = kTailC ? p_env + e : d.env + e;  // (C: the preloaded pointer, no argument fetch in front of the stores)
    // the head carries the row flags the next launch's state machine needs (struct EnvHead)
    uint32_t nflags = head_after;
    if (!kEarly || (head_reset && !kTailC)) nflags = d.tab_phys[r.t].flags_next;
    r.nsamp = HEAD_PACK(r.nsamp, nflags, r.t < rf_until);
    er->h = r;
    er->ep_return = ep_return;
    er->ep_len = ep_len;
    er->penalty_record = penalty_record;
    if (log_on) d.log_pos[e] = lp;
    if (MULTI) {
      reward[e] = rt ? last_rew : reward_sum;
      if (done && (rt || steps == 1)) done[e] = last_done ? 1 : 0;  // one agent step: its done flag
      if (done_count) done_count[e] = n_done;
      if (kPol && act_mode == FLEET_ACT_POLICY_NIGHT) d.cold->night_start[e] = night_st;
    }
  }
  // Placement guard (single-step launches on the library's own queue, fleet_direct.hip).  Such launches carry no release fence,
  // which is only correct while workgroup w of every launch of a run runs on the die (XCC) that ran workgroup w of the previous
  // one -- a die's L2 is the only place the env's newest state lives.  The hardware deals the workgroups of a dispatch to the dies
  // round-robin from a die that belongs to the QUEUE, but that die is not a constant: it moves by one whenever a queue is created
  // or destroyed in the process (measured: tools/ubench/xcc_map.cpp) and the platform promises nothing (MI355X_MICROARCH.md,
  // "Workgroup dispatch, XCD placement").  So the FIRST launch of every run -- which reads state that the previous run's release
  // made everybody's, and may therefore sit anywhere -- writes the dies of its first eight workgroups into the argument blocks of
  // the run's other launches (byte k of `guard_bytes` there = 0x80 | die of workgroup k; written through and drained), and every
  // other launch compares the die it finds itself on with its slot of that record -- here, at the very end, from the
  // kernel-argument segment itself: one scalar load that hits the constant cache, one s_getreg, a few scalar instructions, nothing
  // held across the step (a record carried from the entry cost 1-3 % per launch in spilled scalars, one fetched by a device-scope
  // vector load 4 %: profiles/r06_experiments/placement_guard_cost.log).  A mismatch raises FLEET_DEVERR_PLACEMENT (sticky; the
  // run's results are void, fleet_check_errors tells the caller).  Launches through HIP carry a record of zeros: no check.
  if constexpr (!MULTI) {
    typedef TwinLateTail Tail;
    static_assert(offsetof(StepKernargs, rec_blocks) == offsetof(StepKernargs, guard_bytes) + 8, "one 24-byte piece of the argument block");
    Tail tl_b = {lt.rec, lt.blocks, lt.rows, lt.rotate};  // (B: fetched with the late block, from the same launch's segment)
    karg_ptr kp = nullptr;
    if constexpr (!kTailB) {
      kp = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(StepKernargs, guard_bytes);
      asm volatile("" : "+s"(kp));  // (not hoisted to the entry: see late_args)
    }
    const Tail& tl = kTailB ? tl_b : *(const Tail*)(const __attribute__((address_space(4))) Tail*)kp;
    if constexpr (kTailB) { if (late_bad) err |= FLEET_DEVERR_INTERNAL; }
    const unsigned w = blockIdx.x + (unsigned)wg_base;
    const unsigned have = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (3 << 11));  // HW_REG_XCC_ID, bits [3:0]
    const unsigned slot = (unsigned)(tl.rec >> (8u * (w & 7u))) & 0xffu;
    if ((slot & 0x80u) && (slot & 0xfu) != have) err |= FLEET_DEVERR_PLACEMENT;
    if (tl.blocks != nullptr && blockIdx.x < 8 && threadIdx.x < 64) {  // the run's first launch: its first eight workgroups record
      // (the blocks are FleetStepLaunch::kBlockBytes apart; `rotate`: 0 -- or, test hook of the guard's negative test, the record
      // shifted by that many workgroups)
      unsigned char* at = tl.blocks + offsetof(StepKernargs, guard_bytes) + ((w + (unsigned)tl.rotate) & 7u);
      for (int r = (int)threadIdx.x; r < tl.rows; r += 64)
        __hip_atomic_store(at + (size_t)r * sizeof(FleetStepLaunch::args), (unsigned char)(0x80u | have), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    (void)guard_bytes; (void)rec_blocks; (void)rec_rows; (void)rec_rotate;
  }
  if (err && env_ok) {  // FLEET_DEVERR_*: per env, and OR-ed into the one word the host-pointer step brings back with its results
    atomicOr(&d.env[e].err, err);
    atomicOr(d.self->err_any, err);
  }
  }  // late_args scope
  FLEET_STAMP(8);
  FLEET_STAMP_RT(10);
  FLEET_STAMP_WHERE();
}

}  // namespace

#include "fleet_aux_kernels.h"

// What fleet_direct_open launches on its queue before it accepts the mode: every workgroup writes down the die it runs on
// (HW_REG_XCC_ID, all bits).  A symbol with C linkage: resolved by name in the code object the HSA loader holds.
extern "C" __global__ void fleet_probe_xcc_kernel(uint32_t* __restrict__ out) {
  if (threadIdx.x == 0) out[blockIdx.x] = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));
}
// Which sources this code was compiled from (fleetrl_amd/build.py passes the hash of the sources and flags to BOTH artefacts):
// fleet_direct_open reads the code object's copy through the HSA loader and refuses a code object that is not the library's twin.
#ifndef FLEET_SRC_SHA
#define FLEET_SRC_SHA "unversioned"
#endif
extern "C" __device__ __attribute__((used)) const char fleet_src_sha[32] = FLEET_SRC_SHA;
const char* fleet_kernels_src_sha() { return FLEET_SRC_SHA; }

#include "fleet_step_plan.h"
