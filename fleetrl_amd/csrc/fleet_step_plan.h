// fleet_step_plan.h -- the host half of fleet_kernels.hip: which instance of fleet_step_kernel a launch takes, and the launchers.
//
// Provides: StepPlan / step_instance / plan_step_gd / plan_step_g (the ONE place an instance is selected -- for a HIP stream, a
// captured graph and the library's own queue alike), step_args (the argument block), FLEET_DISPATCH_G, and the functions
// fleet_device.h declares: fleet_launch_*, fleet_describe_step, fleet_describe_step_instance, fleet_step_has_twin,
// fleet_max_evs_per_lane_group.
// Restates nothing of the reference.
// Expects of its includer: it comes last in fleet_kernels.hip, after kBlock / kMaxGroup, kModeAll ... kModeRt, StepKernargs and
// fleet_step_kernel.  Every instance and grid the selection returns is pinned by tests/test_step_instances_cpu.py.
#pragma once
#include "fleet_aux_kernels.h"
#include "fleet_device.h"
#include "fleet_reset.h"
#include <cstddef>
#include <cstdio>
#include <cstring>

namespace {

int group_size(int N) {
  int G = 1;
  while (G < N && G < 64) G <<= 1;
  return G;
}

// The launch a step configuration takes: the instance of fleet_step_kernel, its grid of kBlock-thread workgroups, and whether it is
// the single-step instance (the only kind fleet_describe_step writes down).  Every instance has the same signature.
using StepKernelFn = decltype(&fleet_step_kernel<1, FLEET_DEG_NONE, false, false>);
struct StepPlan {
  StepKernelFn fn;
  unsigned grid;
  bool single;
  const FleetStepInstance* id;  // the template arguments of `fn` (fleet_step_instance: which kernel a configuration takes)
  StepKernelFn fn_dead;         // the state-only twin of `fn` (fleet_step_kernel, DEAD), nullptr where there is none
};
// The one place that takes an instance's address: the description is formed from the same template arguments as the pointer, so
// the two cannot disagree.
template <int G, int DEG, bool MULTI, bool WIDE, bool LOG = false, bool A64 = false, int MODE = kModeAll>
StepPlan step_instance(unsigned grid, bool single) {
  static constexpr FleetStepInstance id{G, DEG, MULTI, WIDE, LOG, A64, MODE};
  // ... and the state-only twin from the same template arguments: single-step, one EV per lane, groups of whole wavefronts.  Smaller
  // groups and the several-EVs-per-lane instance keep the run-time `outputs_dead` flag (not the benchmark's shapes: 54 more instances
  // would cost build time for nothing).  Never selected by plan_step: only fleet_describe_step hands it out.
  StepKernelFn dead = nullptr;
  if constexpr (!MULTI && !WIDE && !LOG && G >= 64 && MODE == kModeAll) dead = &fleet_step_kernel<G, DEG, false, false, false, A64, kModeAll, true>;
  return {&fleet_step_kernel<G, DEG, MULTI, WIDE, LOG, A64, MODE>, grid, single, &id, dead};
}

// Instance selection.  G (EVs per env rounded up to a power of two, at most 64) and DEG come from the switches of plan_step; an env
// of 65 ... kMaxGroup EVs re-enters with a group of two or four wavefronts (G = 128 / 256), one of more EVs than lanes (or that needs
// the real_time or data-log code) with WIDE: every lane walks several EVs.  The `if constexpr` tests keep kernels that a (G, WIDE)
// never launches from being instantiated at all.
template <int G, int DEG, bool WIDE = false>
StepPlan plan_step_gd(const FleetDev& d, int act_mode, int K, bool has_done_count) {
  if constexpr (G == 64 && !WIDE) {
    if (d.N > kMaxGroup || (d.N > 64 && (d.real_time || d.log_pos))) return plan_step_gd<64, DEG, true>(d, act_mode, K, has_done_count);
    if (d.N > 128) return plan_step_gd<256, DEG>(d, act_mode, K, has_done_count);
    if (d.N > 64) return plan_step_gd<128, DEG>(d, act_mode, K, has_done_count);
  }
  const int epb = kBlock / G;
  const unsigned grid = (unsigned)((d.E + epb - 1) / epb);
  // the single-step kernel carries neither the policies, nor the event-skipping loop, nor the data-log code; with WIDE it reads
  // either action dtype at run time
  if (K == 1 && !has_done_count && act_mode < FLEET_ACT_POLICY_UNCONTROLLED && !d.real_time && !d.log_pos) {
    if constexpr (!WIDE)
      if (act_mode == FLEET_ACT_F64) return step_instance<G, DEG, false, false, false, true>(grid, true);
    return step_instance<G, DEG, false, WIDE>(grid, true);
  }
  // K steps per launch: the data log (groups of one wavefront or less); from 32 lanes on the instance that carries what the launch
  // uses -- the event-skipping loop, the built-in policies, or the tape only; smaller groups keep ONE instance with everything behind
  // run-time tests
  if constexpr (G <= 64)
    if (d.log_pos) return step_instance<G, DEG, true, WIDE, true>(grid, false);
  if constexpr (G >= 32) {
    if (d.real_time) return step_instance<G, DEG, true, WIDE, false, false, kModeRt>(grid, false);
    if (act_mode >= FLEET_ACT_POLICY_UNCONTROLLED) return step_instance<G, DEG, true, WIDE, false, false, kModePolicy>(grid, false);
    return step_instance<G, DEG, true, WIDE, false, false, kModeTape>(grid, false);
  }
  // (no `else` above: this instance stays instantiated for every group, and kModeRt for G = 128 / 256, though no launch takes them --
  // the set of instances this selection has always compiled)
  return step_instance<G, DEG, true, WIDE, false, false, kModeAll>(grid, false);
}

template <int G>
StepPlan plan_step_g(const FleetDev& d, int act_mode, int K, bool has_done_count) {
  switch (d.deg_mode) {
    case FLEET_DEG_NONE: return plan_step_gd<G, FLEET_DEG_NONE>(d, act_mode, K, has_done_count);
    case FLEET_DEG_LINEAR: return plan_step_gd<G, FLEET_DEG_LINEAR>(d, act_mode, K, has_done_count);
    default: return plan_step_gd<G, FLEET_DEG_RAINFLOW>(d, act_mode, K, has_done_count);
  }
}

// The argument block of a step launch, as issued on a HIP stream (`outputs_dead` = 0: every launch's outputs can be read); a run on
// the library's own queue fills in the placement record's fields and `outputs_dead` itself (fleet_direct_prepare).
StepKernargs step_args(const FleetDev& d, const void* actions, int act_mode, int K, float* obs, double* reward, uint8_t* done,
                       float* terminal_obs, int32_t* done_count) {
  StepKernargs a{};
  a.p_hot = d.hot; a.p_run = d.run; a.p_soh = d.soh; a.p_actions = actions; a.p_E = d.E; a.p_N = d.N; a.p_env = d.env;
  a.d_arg = d; a.actions = actions; a.act_mode = act_mode; a.K = K;
  a.obs = obs; a.reward = reward; a.done = done; a.terminal_obs = terminal_obs; a.done_count = done_count;
  return a;
}

template <int G>
hipError_t launch_reset_g(const FleetDev& d, const uint8_t* mask, float* obs, hipStream_t s) {
  const int epb = kBlock / G;
  hipLaunchKernelGGL((fleet_reset_kernel<G>), dim3((d.E + epb - 1) / epb), dim3(kBlock), 0, s, d, mask, obs);
  return hipGetLastError();
}

}  // namespace

#define FLEET_DISPATCH_G(N, CALL)          \
  switch (group_size(N)) {                 \
    case 1: return CALL(1);                \
    case 2: return CALL(2);                \
    case 4: return CALL(4);                \
    case 8: return CALL(8);                \
    case 16: return CALL(16);              \
    case 32: return CALL(32);              \
    default: return CALL(64);              \
  }

// Up to this many EVs per env a single-step launch gives every EV a lane of its own (groups of 1 ... 4 wavefronts per env) and reads
// the carried schedule records; beyond it the lanes walk several EVs each and read the table.
int fleet_max_evs_per_lane_group() { return kMaxGroup; }

hipError_t fleet_launch_reset(const FleetDev& d, const uint8_t* mask, float* obs, hipStream_t s) {
#define CALL(Gv) launch_reset_g<Gv>(d, mask, obs, s)
  FLEET_DISPATCH_G(d.N, CALL)
#undef CALL
}

static StepPlan plan_step(const FleetDev& d, int act_mode, int K, bool has_done_count) {
#define CALL(Gv) plan_step_g<Gv>(d, act_mode, K, has_done_count)
  FLEET_DISPATCH_G(d.N, CALL)
#undef CALL
}

hipError_t fleet_launch_step(const FleetDev& d, const void* actions, int act_dtype, int K, float* obs, double* reward,
                             uint8_t* done, float* terminal_obs, int32_t* done_count, hipStream_t s) {
  const StepPlan p = plan_step(d, act_dtype, K, done_count != nullptr);
  const StepKernargs a = step_args(d, actions, act_dtype, K, obs, reward, done, terminal_obs, done_count);
  hipLaunchKernelGGL(p.fn, dim3(p.grid), dim3(kBlock), 0, s, a.p_hot, a.p_run, a.p_soh, a.p_actions, a.p_E, a.p_N, a.p_env, a.d_arg,
                     a.actions, a.act_mode, a.K, a.outputs_dead, a.obs, a.reward, a.done, a.terminal_obs, a.done_count, a.guard_bytes, a.rec_blocks,
                     a.rec_rows, a.rec_rotate);
  return hipGetLastError();
}

// "G64.rainflow.multi.policy": lanes per env (with `w` where every lane walks several EVs), degradation model, single step or K
// steps per launch, then what the instance carries -- the data log, or the part of the K-step code it was cut to (`all`: everything
// behind run-time tests); a single-step instance the action dtype it reads (`any`: either, chosen at run time).  Combinations of
// template arguments no launch takes today get every tag that applies, so that two instances never share a name.
int fleet_describe_step_instance(const FleetDev& d, int act_mode, int K, bool has_done_count, char* name, size_t name_bytes,
                                 unsigned* grid) {
  const StepPlan p = plan_step(d, act_mode, K, has_done_count);
  const FleetStepInstance& i = *p.id;
  static const char* const deg[] = {"none", "linear", "rainflow"};
  static const char* const mode[] = {".all", ".tape", ".policy", ".rt"};
  const char* dtype = i.a64 ? ".f64" : i.multi ? "" : i.wide ? ".any" : ".f32";
  const char* part = (i.multi && !i.log) || i.mode != kModeAll ? mode[i.mode] : "";
  *grid = p.grid;
  return snprintf(name, name_bytes, "G%d%s.%s.%s%s%s%s", i.G, i.wide ? "w" : "", deg[i.deg], i.multi ? "multi" : "single",
                  i.log ? ".log" : "", part, dtype);
}

bool fleet_step_has_twin(const FleetDev& d, int act_mode, int K, bool has_done_count) {
  const StepPlan p = plan_step(d, act_mode, K, has_done_count);
  return p.single && p.fn_dead != nullptr;
}

hipError_t fleet_describe_step(const FleetDev& d, const void* actions, int act_dtype, float* obs, double* reward, uint8_t* done,
                               float* terminal_obs, FleetStepLaunch* out) {
  const StepPlan p = plan_step(d, act_dtype, 1, false);
  if (!p.single) return hipErrorNotSupported;
  const StepKernargs a = step_args(d, actions, act_dtype, 1, obs, reward, done, terminal_obs, nullptr);
  out->host_fn = (const void*)p.fn; out->host_fn_dead = (const void*)p.fn_dead; out->grid = p.grid; out->block = kBlock; out->args_bytes = (unsigned)sizeof a;
  out->actions_offset[0] = (unsigned)offsetof(StepKernargs, p_actions); out->actions_offset[1] = (unsigned)offsetof(StepKernargs, actions);
  out->packed_n_offset = (unsigned)offsetof(StepKernargs, p_N);
  out->guard_offset = (unsigned)offsetof(StepKernargs, guard_bytes);
  out->rec_offset = (unsigned)offsetof(StepKernargs, rec_blocks);  // (then rec_rows and rec_rotate)
  out->dead_offset = (unsigned)offsetof(StepKernargs, outputs_dead);
  memcpy(out->args, &a, sizeof a);
  return hipSuccess;
}

hipError_t fleet_launch_term_compact(const FleetDev& d, const uint8_t* done, const float* term, int32_t* idx, int32_t* count,
                                     double* ep_ret, int32_t* ep_len, float* compact, hipStream_t s) {
  hipLaunchKernelGGL(fleet_term_scan_kernel, dim3(1), dim3(1024), 0, s, done, d.E, idx, count, d.env, d.cold, ep_ret, ep_len);
  hipLaunchKernelGGL(fleet_term_gather_kernel, dim3(256), dim3(256), 0, s, term, d.obs_dim, idx, count, compact);
  return hipGetLastError();
}

hipError_t fleet_launch_dist_factor(const FleetDev& d, double* out, hipStream_t s) {
  const size_t n = (size_t)d.E * d.N;
  hipLaunchKernelGGL(fleet_dist_factor_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, out);
  return hipGetLastError();
}

hipError_t fleet_launch_gather_field(const FleetDev& d, int field, void* out, hipStream_t s) {
  const size_t n = (size_t)d.E * d.N;
  hipLaunchKernelGGL(fleet_gather_field_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, field, out);
  return hipGetLastError();
}

hipError_t fleet_launch_selftest_stress(unsigned long long n, unsigned long long seed, unsigned long long* worst_dev, hipStream_t s) {
  hipLaunchKernelGGL(fleet_selftest_stress_kernel, dim3(2048), dim3(256), 0, s, n, seed, worst_dev);
  return hipGetLastError();
}

hipError_t fleet_launch_selftest_division(unsigned long long n, unsigned long long seed, unsigned long long* bad_dev, hipStream_t s) {
  hipLaunchKernelGGL(fleet_selftest_division_kernel, dim3(2048), dim3(256), 0, s, n, seed, bad_dev);
  return hipGetLastError();
}
