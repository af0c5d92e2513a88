/* fleet_hip_sac_loop.h -- SAC's collect_rollouts and EvalCallback on the device, one enqueue-only call each (fleet_collect.hip,
 * fleet_eval.hip; DESIGN.md "SAC's loop on the device").
 * (entries added under FLEET_ABI_VERSION 11: nothing that existed before changes, so the number stays.  include/fleet_hip.h is as it
 * was, byte for byte; every entry here is declared `FLEET_API int` or `FLEET_API const char*` and starts with fleet_saccollect_ or
 * fleet_saceval_.)
 * With these, SAC's loop is what PPO's and TD3's are: collect, train (fleet_sactrain_sac_dev) and, every so often, evaluate, each one
 * call that only enqueues.  The handles are the EXISTING ones: fleet_saccollect_create returns a fleet_collect_handle and
 * fleet_saceval_create a fleet_eval_handle, as fleet_sac_create returns a fleet_qtarget_handle; what differs is the actor they borrow --
 * the squashed-Gaussian networks of fleet_sac_create instead of a policy.  Everything in the two sections of fleet_hip.h holds for such
 * a handle unless it is said otherwise here.
 *
 * ---- the uniform draw without a policy
 * SB3's warm-up (num_timesteps < learning_starts) samples the action space; fleet_explore_act_dev's UNIFORM mode does that on a policy
 * handle, which a SAC agent does not have.  fleet_saccollect_uniform_dev is the SAME kernel (explore_uniform, fleet_policy.hip) through
 * the same one launch site, on the networks handle's stream, over E x act_dim: under one (seed, step, env_id_offset + e) the bits are
 * those of fleet_explore_act_dev UNIFORM DRAW -- a[e][j] = lo + (hi - lo) * u kept below hi, u the top 24 bits of word j % 4 of the
 * Philox block (env_id_offset + e, j / 4, step lo, step hi) under key (seed lo, seed hi), times 2^-24.
 *
 * ---- the collector
 * fleet_saccollect_sac_dev is fleet_collect_offpolicy_dev's loop -- the same code -- with another actor.  Per env step t, with
 * s = first_step + t:
 *   1. s < learning_starts: fleet_saccollect_uniform_dev over [noise_lo, noise_hi]; else fleet_sac_act_dev with deterministic = 0,
 *      noise_mode DRAW, key (seed, env_id_offset, step = s), norm NULL (the carry observation is already normalised), no optional
 *      output.  Either launch writes the handle's env_actions.
 *   2. fleet_step_dev   3. fleet_norm_step_dev (not without a normaliser)
 *   4. fleet_replay_add_dev(raw cur, raw next, the action the env got, the raw reward as F64, done, the raw terminal rows, NULL)
 *   5. the episode launch; the sides swap
 * then the closing launch: 5 n_steps + 1 launches with a normaliser, 4 n_steps + 1 without; FleetCollectInfo.launches reports them.
 * One deviation from SB3: during the warm-up SB3 stores scale_action(sample) -- 2 * ((a - low) / (high - low)) - 1 -- which over
 * [-1, 1] can differ from the sample in the last bit.  Here the buffer gets the action the env got, as in the TD3 collector.
 * fleet_collect_describe, _reset_dev, _episodes_dev, _finish_dev, _episodes_read and _destroy serve the handle unchanged;
 * FleetCollectInfo keeps its 152 bytes (last_values is not written).  fleet_collect_ppo_dev and fleet_collect_offpolicy_dev REFUSE such
 * a handle, naming fleet_saccollect_sac_dev, and fleet_saccollect_sac_dev refuses a handle fleet_collect_create made; nothing is launched.
 *
 * ---- the evaluation
 * fleet_eval_run_dev on a handle of fleet_saceval_create takes its action from fleet_sac_act_dev with deterministic = 1 -- tanhf(mu); no
 * noise is read or written -- and norm NULL.  Everything around the action is the code of the evaluation section: reset, clear, the
 * step, the normaliser's step, the quota launch, the closing launch and the gated copy; 4 n_steps + 5 launches with a normaliser,
 * 3 n_steps + 4 without, one more with sync_from.  The snapshot is the WHOLE image of the networks handle -- the actor and the critics,
 * what SB3's best_model.zip holds.  fleet_eval_best_export_dev serves it unchanged: the tensors come in the image's order, W, b per
 * layer of the actor (the last pair the ONE [2A, H] / [2A] pair), then of critic 0, then of critic 1.  fleet_eval_best_load_dev REFUSES
 * such a handle, naming fleet_saceval_best_load_dev, which in turn refuses a handle fleet_eval_create made.
 * Out of scope: gSDE, an action_noise on top of SAC's own sampling, train_freq in episodes, the time-limit bootstrap, stochastic
 * evaluation, a one-call learn() that alternates collect and train. */
#ifndef FLEET_HIP_SAC_LOOP_H
#define FLEET_HIP_SAC_LOOP_H

#include "fleet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FleetSacUniformArgs {
  int32_t struct_bytes;          /* sizeof(FleetSacUniformArgs) */
  int32_t env_id_offset;         /* global id of row 0; >= 0 */
  float lo, hi;                  /* the action space: lo <= hi */
  uint64_t seed;                 /* Philox key */
  uint64_t step;                 /* the noise counter */
  float* actions;                /* device f32[E, act_dim] */
} FleetSacUniformArgs;
typedef struct FleetSacCollectArgs {
  int32_t struct_bytes;          /* sizeof(FleetSacCollectArgs) */
  int32_t n_steps;               /* >= 1 */
  int32_t env_id_offset;         /* >= 0 */
  int32_t reserved;              /* 0 */
  uint64_t learning_starts;      /* global steps below it draw uniform actions */
  fleet_replay_handle replay;    /* E, D, A as the handle's */
  float noise_lo, noise_hi;      /* the action space of the warm-up's draw: noise_lo <= noise_hi */
  uint64_t seed;
  uint64_t first_step;           /* env steps taken before this call */
  double* stats;                 /* device f64[FLEET_COLLECT_STATS] */
} FleetSacCollectArgs;

/* h may be NULL: the last failed fleet_saccollect_* call without a handle, the string fleet_collect_last_error(NULL) returns.  With a
 * handle: fleet_collect_last_error(h). */
FLEET_API const char* fleet_saccollect_last_error(fleet_collect_handle h);
/* One launch on the networks handle's stream.  The arguments are looked at before the handle is: FLEET_ERR_INVALID, with the reason in
 * fleet_saccollect_last_error(NULL), for a null or wrongly sized FleetSacUniformArgs, E < 1, a null actions, a negative env_id_offset,
 * lo > hi or a NaN bound, a null handle; with the handle, and the reason in fleet_sac_last_error(nets): networks that fleet_sac_create
 * did not make. */
FLEET_API int fleet_saccollect_uniform_dev(fleet_qtarget_handle nets, int E, const FleetSacUniformArgs* a);
/* Everything is refused BEFORE the device is touched (fleet_saccollect_last_error(NULL) says why, starting with the entry's name):
 * whatever fleet_collect_create refuses, networks that are not squashed (fleet_sac_create makes them), a device that differs from the
 * env's, an obs_dim that differs from the env's, an act_dim that differs from the env's EVs, a normaliser that does not fit. */
FLEET_API int fleet_saccollect_create(fleet_handle env, fleet_norm_handle norm, fleet_qtarget_handle nets, const FleetCollectParams* p,
                                      fleet_collect_handle* out);
/* Only enqueues, on the stream env, normaliser, networks and replay buffer launch on -- they must launch on ONE stream.  Everything
 * refusable is refused before the first launch, in the words of the entry that would refuse: a null or wrongly sized
 * FleetSacCollectArgs, n_steps < 1, a reserved that is not 0, a negative env_id_offset, a null replay or stats, noise_lo > noise_hi or
 * a NaN bound (with h NULL the reason, or "null handle", goes to fleet_saccollect_last_error(NULL)), and -- these need the handle -- a
 * handle fleet_collect_create made, a replay buffer whose E, D or A differ or that lies on another device, handles on other streams
 * ("the networks launch on another stream than the env: fleet_qtarget_set_stream them to the env's first"). */
FLEET_API int fleet_saccollect_sac_dev(fleet_collect_handle h, const FleetSacCollectArgs* a);

/* Refuses what fleet_eval_create refuses, before the device is touched (fleet_eval_last_error(NULL) says why, starting with this entry's
 * name), and networks that are not squashed. */
FLEET_API int fleet_saceval_create(fleet_handle env, fleet_norm_handle norm, fleet_qtarget_handle nets, const FleetEvalParams* p,
                                   fleet_eval_handle* out);
/* The snapshot into another fleet_sac_create handle of the same layout, one launch (no gate).  Its refusals are
 * fleet_eval_best_load_dev's: a null handle, a destination that is no networks handle, that fleet_sac_create did not make, that lies on
 * another device, whose layout differs or that launches on another stream; a handle fleet_eval_create made; FLEET_ERR_STATE before any
 * evaluation has run. */
FLEET_API int fleet_saceval_best_load_dev(fleet_eval_handle h, fleet_qtarget_handle dst);

#ifdef __cplusplus
}
#endif
#endif /* FLEET_HIP_SAC_LOOP_H */
