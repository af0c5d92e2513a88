"""ctypes mirror of include/fleet_hip.h (struct layouts, constants) and the libfleet_hip.so loader.

There is deliberately NO CPU fallback: if the HIP library is missing or no GPU is visible, every
product entry point raises (`FleetHipError`).  The CPU restatement under oracle/ is test
infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

ABI_VERSION = 11

OK, ERR_INVALID, ERR_HIP, ERR_STATE, ERR_NODEVICE, ERR_UNSUPPORTED = 0, 1, 2, 3, 4, 5
DEG_NONE, DEG_LINEAR, DEG_RAINFLOW = 0, 1, 2
PICK_STATIC, PICK_RANDOM, PICK_EVAL = 0, 1, 2
ACT_F32, ACT_F64 = 0, 1
# fleet_run_tape_dev / fleet_time_regions_begin: how the launches reach the GPU (include/fleet_hip.h FLEET_LAUNCH_*)
LAUNCH_EAGER, LAUNCH_GRAPH, LAUNCH_DIRECT, LAUNCH_DIRECT_ONE_QUEUE = 0, 1, 2, 3
POLICY_UNCONTROLLED, POLICY_DISTRIBUTED, POLICY_NIGHT = 2, 3, 4
# fleet_lp_plan_dev status bits per (env, EV) (include/fleet_hip.h FLEET_LP_*)
LP_UNREACHABLE, LP_NEG_RETURN, LP_ABOVE_TARGET, LP_GRID_NEGATIVE = 1, 2, 4, 8

DEVERR_OBS_FORMAT, DEVERR_NEG_LIFE, DEVERR_SOH_MISMATCH, DEVERR_DOD_RANGE, DEVERR_TABLE_END, DEVERR_INTERNAL, DEVERR_PLACEMENT = 1, 2, 4, 8, 16, 32, 64

# fleet_get fields: name -> (id, dtype, per_car)
FIELDS = {
    "soc": (0, np.float64, True),
    "hours_left": (1, np.float32, True),
    "soh": (2, np.float64, True),
    "soc_deg": (3, np.float64, True),
    "target_soc": (4, np.float64, True),
    "time_idx": (5, np.int32, False),
    "start_idx": (6, np.int32, False),
    "cashflow": (7, np.float64, False),
    "ep_return": (8, np.float64, False),
    "ep_len": (9, np.int32, False),
    "last_ep_return": (10, np.float64, False),
    "last_ep_len": (11, np.int32, False),
    "rf_len": (12, np.int32, True),
    "fd_cyc": (13, np.float64, True),
    "fd_cal": (14, np.float64, True),
    "sei_l": (15, np.float64, True),
    "error_bits": (16, np.uint32, False),
    "done": (17, np.uint8, False),
    "episodes": (18, np.int32, False),
    "penalty_record": (19, np.float64, False),
    "last_ep_len_f64": (20, np.float64, False),
    "rf_cycles": (21, np.int32, True),
    "rf_stack": (22, np.int32, True),
    "rf_until": (23, np.int32, False),
}

_I32_FIELDS = (
    "abi_version", "struct_bytes", "num_envs", "num_cars", "table_rows", "episode_steps", "price_lookahead",
    "bl_pv_lookahead", "steps_per_hour", "hour_phase", "include_building", "include_pv", "aux", "normalize",
    "is_caretaker", "deg_mode", "picker_mode", "start_lo", "start_hi", "auto_reset", "env_id_offset", "log_data",
    "real_time", "log_capacity",
)
_F64_FIELDS = (
    "dt", "evse_power", "obc_max_power", "batt_cap_nominal", "init_battery_cap", "grid_connection",
    "charging_eff", "discharging_eff", "fixed_markup", "variable_multiplier", "feed_in_deduction",
    "price_multiplier", "penalty_invalid_action", "penalty_overcharging", "clip_overcharging",
    "penalty_overloading", "fully_charged_reward", "target_soc", "target_soc_lunch", "eps", "def_soc",
    "min_laxity", "init_soh", "temperature", "max_time_left", "max_price", "min_price", "max_tariff",
    "min_tariff", "max_building", "max_pv", "max_soc", "max_hours_needed", "max_laxity", "max_evse", "max_grid",
)


class FleetParams(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in _I32_FIELDS] + [("seed", C.c_uint64)] + [(n, C.c_double) for n in _F64_FIELDS])

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


_TABLE_FIELDS = (
    ("there", C.POINTER(C.c_uint8)), ("time_left", C.POINTER(C.c_float)), ("soc_on_return", C.POINTER(C.c_double)),
    ("delu", C.POINTER(C.c_double)), ("tariff", C.POINTER(C.c_double)), ("prc", C.POINTER(C.c_double)),
    ("trc", C.POINTER(C.c_double)), ("load", C.POINTER(C.c_double)), ("pv", C.POINTER(C.c_double)),
    ("hour", C.POINTER(C.c_uint8)), ("minute", C.POINTER(C.c_uint8)), ("month", C.POINTER(C.c_uint8)),
    ("weekday", C.POINTER(C.c_uint8)), ("time_feat", C.POINTER(C.c_float)),
    # irregular time grids (real_time), all NULL / 0 otherwise
    ("dt_row", C.POINTER(C.c_double)), ("finish_row", C.POINTER(C.c_int32)), ("lookahead_row", C.POINTER(C.c_int32)),
    ("lookahead_cols", C.c_int32), ("reserved0", C.c_int32), ("second", C.POINTER(C.c_uint8)),
    ("pick_rows", C.POINTER(C.c_int32)), ("n_pick_rows", C.c_int32), ("reserved1", C.c_int32),
)


class FleetNormParams(C.Structure):
    """include/fleet_hip.h FleetNormParams (the running normaliser, fleet_norm_*)."""
    _fields_ = [("struct_bytes", C.c_int32), ("num_envs", C.c_int32), ("obs_dim", C.c_int32), ("training", C.c_int32),
                ("norm_obs", C.c_int32), ("norm_reward", C.c_int32), ("clip_obs", C.c_double), ("clip_reward", C.c_double),
                ("gamma", C.c_double), ("epsilon", C.c_double)]


class FleetTablesC(C.Structure):
    _fields_ = list(_TABLE_FIELDS)


# ---- rollout buffer (include/fleet_hip.h "rollout buffer on the device", fleet_rollout_*) -----------------------------------------
ROLLOUT_ALIGN = 256
ROLLOUT_ARRAY_NAMES = ("obs", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")


class FleetRolloutParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("num_envs", C.c_int32), ("n_steps", C.c_int32), ("obs_dim", C.c_int32),
                ("act_dim", C.c_int32), ("reserved", C.c_int32), ("gamma", C.c_double), ("gae_lambda", C.c_double)]


class FleetRolloutLayout(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("alignment", C.c_int32), ("total_bytes", C.c_uint64),
                ("offset", C.c_uint64 * len(ROLLOUT_ARRAY_NAMES)), ("bytes", C.c_uint64 * len(ROLLOUT_ARRAY_NAMES)),
                ("row_bytes", C.c_uint64 * len(ROLLOUT_ARRAY_NAMES)), ("error_offset", C.c_uint64)]


class FleetRolloutArrays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ROLLOUT_ARRAY_NAMES]


class FleetRolloutSlot(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "actions", "reward", "episode_start", "value", "log_prob")]


# ---- replay buffer (include/fleet_hip.h "replay buffer on the device", fleet_replay_*) ------------------------------------------
REPLAY_ALIGN = 256
REPLAY_ARRAY_NAMES = ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")


class FleetReplayParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("num_envs", C.c_int32), ("buffer_size", C.c_int32), ("obs_dim", C.c_int32),
                ("act_dim", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


class FleetReplayLayout(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("alignment", C.c_int32), ("rows", C.c_int32), ("reserved", C.c_int32),
                ("total_bytes", C.c_uint64), ("offset", C.c_uint64 * len(REPLAY_ARRAY_NAMES)),
                ("bytes", C.c_uint64 * len(REPLAY_ARRAY_NAMES)), ("row_bytes", C.c_uint64 * len(REPLAY_ARRAY_NAMES)),
                ("error_offset", C.c_uint64)]


class FleetReplayArrays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in REPLAY_ARRAY_NAMES]


# ---- MLP policy (include/fleet_hip.h "MLP policy on the device", fleet_policy_*) -------------------------------------------------
POLICY_MAX_HEADS, POLICY_MAX_LAYERS, POLICY_MAX_WIDTH, POLICY_MAX_OBS_DIM = 2, 4, 512, 8192
POLICY_ACT_TANH, POLICY_ACT_RELU = 0, 1
POLICY_OUT_NONE, POLICY_OUT_CLIP, POLICY_OUT_TANH = 0, 1, 2


class FleetPolicyHead(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("width", C.c_int32 * POLICY_MAX_LAYERS), ("activation", C.c_int32), ("output", C.c_int32),
                ("reserved", C.c_int32), ("lo", C.c_float), ("hi", C.c_float)]


class FleetPolicyParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("obs_dim", C.c_int32), ("n_heads", C.c_int32), ("tile_rows", C.c_int32),
                ("head", FleetPolicyHead * POLICY_MAX_HEADS)]


# ---- exploration actions (include/fleet_hip.h "exploration actions on the device", fleet_explore_*) ---------------------------------
EXPLORE_GAUSSIAN, EXPLORE_ACTION_NOISE, EXPLORE_UNIFORM = 0, 1, 2
EXPLORE_NOISE_DRAW, EXPLORE_NOISE_GIVEN = 0, 1


class FleetExploreArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("mode", C.c_int32), ("noise_mode", C.c_int32), ("reserved0", C.c_int32),
                ("seed", C.c_uint64), ("step", C.c_uint64), ("env_id_offset", C.c_int32), ("reserved1", C.c_int32),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("noise_lo", C.c_float), ("noise_hi", C.c_float),
                ("noise", C.c_void_p), ("actions", C.c_void_p), ("env_actions", C.c_void_p), ("log_prob", C.c_void_p),
                ("values", C.c_void_p), ("mean", C.c_void_p)]


# ---- correlated action noise (include/fleet_hip.h "correlated action noise on the device", fleet_noise_*) ---------------------------
NOISE_PINK, NOISE_OU = 0, 1
NOISE_MAX_ACT_DIM, NOISE_MAX_SEQ_LEN = 512, 4096


class FleetNoiseParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("kind", C.c_int32), ("num_envs", C.c_int32), ("act_dim", C.c_int32),
                ("env_id_offset", C.c_int32), ("seq_len", C.c_int32), ("seed", C.c_uint64), ("beta", C.c_double), ("theta", C.c_double),
                ("dt", C.c_double), ("mu", C.c_void_p), ("sigma", C.c_void_p), ("cache_bytes", C.c_uint64)]


# ---- TD3 / DDPG learning targets (include/fleet_hip.h "TD3 / DDPG learning targets on the device", fleet_qtarget_*) ----------------
class FleetQTargetParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("obs_dim", C.c_int32), ("n_critics", C.c_int32), ("tile_rows", C.c_int32),
                ("actor", FleetPolicyHead), ("critic", FleetPolicyHead * 2)]


class FleetQTargetArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("noise_mode", C.c_int32), ("seed", C.c_uint64), ("step", C.c_uint64),
                ("row_offset", C.c_int32), ("reserved", C.c_int32), ("gamma", C.c_float), ("noise_clip", C.c_float),
                ("act_lo", C.c_float), ("act_hi", C.c_float), ("sigma", C.c_void_p), ("noise", C.c_void_p), ("target_q", C.c_void_p),
                ("next_actions", C.c_void_p), ("q", C.c_void_p)]


# ---- SAC's actor and soft targets (include/fleet_hip.h "SAC on the device", fleet_sac_*) ----------------------------------------------
class FleetSacParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("obs_dim", C.c_int32), ("n_critics", C.c_int32), ("reserved", C.c_int32),
                ("actor", FleetPolicyHead), ("critic", FleetPolicyHead * 2)]


class FleetSacActArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("noise_mode", C.c_int32), ("deterministic", C.c_int32), ("env_id_offset", C.c_int32),
                ("seed", C.c_uint64), ("step", C.c_uint64), ("noise", C.c_void_p), ("actions", C.c_void_p),
                ("gaussian_actions", C.c_void_p), ("log_prob", C.c_void_p), ("mean", C.c_void_p), ("log_std", C.c_void_p)]


class FleetSacTargetArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("noise_mode", C.c_int32), ("seed", C.c_uint64), ("step", C.c_uint64),
                ("row_offset", C.c_int32), ("gamma", C.c_float), ("ent_coef", C.c_void_p), ("noise", C.c_void_p),
                ("target_q", C.c_void_p), ("next_actions", C.c_void_p), ("next_log_prob", C.c_void_p), ("q", C.c_void_p)]


# ---- SAC's actor and entropy-coefficient gradients (include/fleet_hip.h "SAC actor and entropy-coefficient gradients on the device") --
class FleetSacActorArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("B", C.c_int32), ("noise_mode", C.c_int32), ("row_offset", C.c_int32),
                ("seed", C.c_uint64), ("step", C.c_uint64), ("obs", C.c_void_p), ("ent_coef", C.c_void_p), ("noise", C.c_void_p),
                ("log_ent_coef", C.c_void_p), ("log_ent_coef_grad", C.c_void_p), ("target_entropy", C.c_float), ("reserved", C.c_int32),
                ("actions_out", C.c_void_p), ("log_prob_out", C.c_void_p), ("q_out", C.c_void_p), ("dheads_out", C.c_void_p),
                ("stats", C.c_void_p)]


# ---- PPO minibatch gradients (include/fleet_hip.h "PPO minibatch gradients on the device", fleet_ppo_*) ------------------------------
class FleetPpoParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("max_batch", C.c_int32)]


class FleetPpoGradArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("B", C.c_int32), ("obs", C.c_void_p), ("actions", C.c_void_p), ("old_log_prob", C.c_void_p),
                ("advantages", C.c_void_p), ("returns", C.c_void_p), ("log_std", C.c_void_p), ("clip_range", C.c_float),
                ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("reserved", C.c_int32), ("values", C.c_void_p), ("log_prob", C.c_void_p),
                ("stats", C.c_void_p)]


class FleetPpoGradVclipArgs(C.Structure):  # fleet_ppo_grad_vclip_dev: the same with SB3's clip_range_vf
    _fields_ = [("struct_bytes", C.c_int32), ("clip_range_vf", C.c_float), ("old_values", C.c_void_p), ("base", FleetPpoGradArgs)]


class FleetPpoGate(C.Structure):  # two device words and the threshold of early stopping on approx_kl
    _fields_ = [("skip", C.c_void_p), ("decided", C.c_void_p), ("threshold", C.c_double)]


class FleetPpoGradGatedArgs(C.Structure):  # fleet_ppo_grad_gated_dev: either of the above behind a gate (clip_range_vf 0: no value clip)
    _fields_ = [("struct_bytes", C.c_int32), ("clip_range_vf", C.c_float), ("old_values", C.c_void_p), ("gate", FleetPpoGate),
                ("base", FleetPpoGradArgs)]


# ---- Adam and clip_grad_norm_ (include/fleet_hip.h "Adam and clip_grad_norm_ on the device", fleet_adam_*) ------------------------------
ADAM_MAX_EXTRA = 2
ADAM_STATE_EXPORT, ADAM_STATE_LOAD = 0, 1


class FleetAdamParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("first_net", C.c_int32), ("n_nets", C.c_int32), ("n_extra", C.c_int32),
                ("extra_len", C.c_int32 * ADAM_MAX_EXTRA)]


class FleetAdamStepArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("max_grad_norm", C.c_double), ("norm_out", C.c_void_p)]


class FleetAdamInfo(C.Structure):
    _fields_ = [("state_bytes", C.c_uint64), ("n_elements", C.c_uint64), ("step", C.c_int64), ("n_tensors", C.c_int32),
                ("norm_chunk", C.c_int32), ("step_tile", C.c_int32), ("reserved", C.c_int32)]


# ---- PPO's whole update (include/fleet_hip.h "PPO's whole update on the device", fleet_train_*) ------------------------------------------
TRAIN_ROUNDS, TRAIN_MIN_HALF_BITS, TRAIN_STATS = 8, 4, 16


class FleetTrainPpoArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_epochs", C.c_int32), ("batch_size", C.c_int32), ("normalize_advantage", C.c_int32),
                ("clip_range", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float), ("reserved", C.c_int32), ("lr", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_grad_norm", C.c_double), ("seed", C.c_uint64),
                ("first_epoch", C.c_uint64), ("stats", C.c_void_p)]


class FleetTrainInfo(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("n_steps", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("max_batch", C.c_int32),
                ("n_tensors", C.c_int32), ("rounds", C.c_int32), ("min_half_bits", C.c_int32), ("tile_rows", C.c_int32),
                ("cache_rows", C.c_int32), ("staging_bytes", C.c_uint64), ("staging", C.c_void_p)]


class FleetTrainPpoVclipArgs(C.Structure):  # fleet_train_ppo_vclip_dev: the same with SB3's clip_range_vf
    _fields_ = [("struct_bytes", C.c_int32), ("clip_range_vf", C.c_float), ("base", FleetTrainPpoArgs)]


class FleetTrainPpoKlArgs(C.Structure):  # fleet_train_ppo_kl_dev: the same with SB3's target_kl (clip_range_vf 0: no value clip)
    _fields_ = [("struct_bytes", C.c_int32), ("clip_range_vf", C.c_float), ("target_kl", C.c_double), ("base", FleetTrainPpoArgs)]


# ---- TD3 / DDPG's whole update (include/fleet_hip.h "TD3 / DDPG's whole update on the device", fleet_offpolicy_*) ------------------------
OFFPOLICY_MAX_STEPS, OFFPOLICY_SLOT_FLOATS = 65536, 16


class FleetOffpolicyParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("max_steps", C.c_int32)]


class FleetOffpolicyArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("gradient_steps", C.c_int32), ("batch_size", C.c_int32), ("policy_delay", C.c_int32),
                ("reserved", C.c_int32), ("gamma", C.c_float), ("tau", C.c_double), ("noise_clip", C.c_float), ("act_lo", C.c_float),
                ("act_hi", C.c_float), ("sigma", C.c_void_p), ("lr", C.c_double), ("beta1", C.c_double * 2), ("beta2", C.c_double * 2),
                ("eps", C.c_double * 2), ("max_grad_norm", C.c_double * 2), ("seed", C.c_uint64), ("first_update", C.c_uint64),
                ("norm", C.c_void_p), ("stats", C.c_void_p)]


class FleetOffpolicyInfo(C.Structure):
    _fields_ = [("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_critics", C.c_int32), ("max_batch", C.c_int32), ("max_steps", C.c_int32),
                ("n_actor_tensors", C.c_int32), ("n_critic_tensors", C.c_int32), ("reserved", C.c_int32), ("staging_bytes", C.c_uint64),
                ("staging", C.c_void_p), ("slots", C.c_void_p)]


# ---- SAC's whole update (include/fleet_hip.h "SAC's whole update on the device", fleet_sactrain_*) ----------------------------------------
SACTRAIN_MAX_STEPS, SACTRAIN_SLOT_FLOATS, SACTRAIN_SCALE_CHUNK = 65536, 16, 1024


class FleetSacTrainParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("max_steps", C.c_int32)]


class FleetSacTrainArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("gradient_steps", C.c_int32), ("batch_size", C.c_int32), ("target_update_interval", C.c_int32),
                ("gamma", C.c_float), ("target_entropy", C.c_float), ("tau", C.c_double), ("loss_scale", C.c_double), ("lr", C.c_double),
                ("beta1", C.c_double * 3), ("beta2", C.c_double * 3), ("eps", C.c_double * 3), ("max_grad_norm", C.c_double * 3),
                ("seed", C.c_uint64), ("target_seed", C.c_uint64), ("first_update", C.c_uint64), ("ent_coef", C.c_void_p),
                ("log_ent_coef", C.c_void_p), ("log_ent_coef_grad", C.c_void_p), ("norm", C.c_void_p), ("stats", C.c_void_p)]


class FleetSacTrainInfo(C.Structure):
    _fields_ = [("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_critics", C.c_int32), ("max_batch", C.c_int32), ("max_steps", C.c_int32),
                ("n_actor_tensors", C.c_int32), ("n_critic_tensors", C.c_int32), ("learned_alpha", C.c_int32), ("scale_chunks", C.c_int32),
                ("reserved", C.c_int32), ("staging_bytes", C.c_uint64), ("staging", C.c_void_p), ("alpha", C.c_void_p), ("slots", C.c_void_p)]


# ---- rollout collection (include/fleet_hip.h "collect_rollouts on the device", fleet_collect_*) ----------------------------------------
COLLECT_MAX_WINDOW, COLLECT_STATS = 4096, 16


class FleetCollectParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("stats_window", C.c_int32)]


class FleetCollectPpoArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_steps", C.c_int32), ("env_id_offset", C.c_int32), ("reserved", C.c_int32),
                ("buffer", C.c_void_p), ("log_std", C.c_void_p), ("seed", C.c_uint64), ("first_step", C.c_uint64), ("stats", C.c_void_p)]


class FleetCollectOffpolicyArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_steps", C.c_int32), ("env_id_offset", C.c_int32), ("reserved", C.c_int32),
                ("learning_starts", C.c_uint64), ("replay", C.c_void_p), ("sigma", C.c_void_p), ("shift", C.c_void_p),
                ("noise_lo", C.c_float), ("noise_hi", C.c_float), ("noise", C.c_void_p), ("seed", C.c_uint64), ("first_step", C.c_uint64),
                ("stats", C.c_void_p)]


class FleetCollectInfo(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("stats_window", C.c_int32), ("has_norm", C.c_int32),
                ("cur", C.c_int32), ("launches", C.c_int32), ("reserved", C.c_int32), ("block_bytes", C.c_uint64),
                ("carry_obs", C.c_void_p * 2), ("raw_obs", C.c_void_p * 2), ("carry_start", C.c_void_p * 2), ("raw_terminal", C.c_void_p),
                ("raw_reward", C.c_void_p), ("reward", C.c_void_p), ("env_actions", C.c_void_p), ("last_values", C.c_void_p),
                ("ring_return", C.c_void_p), ("ring_length", C.c_void_p), ("ring_count", C.c_void_p)]


# ---- SAC's collector (include/fleet_hip_sac_loop.h, fleet_saccollect_*) -----------------------------------------------------------------
class FleetSacUniformArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("env_id_offset", C.c_int32), ("lo", C.c_float), ("hi", C.c_float), ("seed", C.c_uint64),
                ("step", C.c_uint64), ("actions", C.c_void_p)]


class FleetSacCollectArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_steps", C.c_int32), ("env_id_offset", C.c_int32), ("reserved", C.c_int32),
                ("learning_starts", C.c_uint64), ("replay", C.c_void_p), ("noise_lo", C.c_float), ("noise_hi", C.c_float),
                ("seed", C.c_uint64), ("first_step", C.c_uint64), ("stats", C.c_void_p)]


# ---- evaluation of the agent (include/fleet_hip.h "evaluation of the agent on the device", fleet_eval_*) -------------------------------
EVAL_MAX_EPISODES, EVAL_STATS = 65536, 16


class FleetEvalParams(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("max_episodes", C.c_int32)]


class FleetEvalArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("n_eval_episodes", C.c_int32), ("n_steps", C.c_int32), ("reward_source", C.c_int32),
                ("sync_from", C.c_void_p), ("reserved", C.c_uint64), ("num_timesteps", C.c_uint64), ("stats", C.c_void_p)]


class FleetEvalInfo(C.Structure):
    _fields_ = [("num_envs", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("max_episodes", C.c_int32), ("has_norm", C.c_int32),
                ("launches", C.c_int32), ("block_bytes", C.c_uint64), ("snapshot_floats", C.c_uint64)] + \
               [(n, C.c_void_p) for n in ("obs", "raw_obs", "actions", "raw_reward", "reward", "done", "sums", "lengths", "counts", "ep_reward",
                                          "ep_length", "listed", "best_mean_reward", "evaluations", "gate", "snapshot")]


# ---- TD3 / DDPG minibatch gradients (include/fleet_hip.h "TD3 / DDPG minibatch gradients on the device", fleet_td3_*) -------------------
class FleetTd3Params(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("max_batch", C.c_int32)]


class FleetTd3CriticArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("B", C.c_int32), ("obs", C.c_void_p), ("actions", C.c_void_p), ("target_q", C.c_void_p),
                ("q", C.c_void_p), ("stats", C.c_void_p), ("reserved", C.c_uint64)]


class FleetTd3ActorArgs(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("B", C.c_int32), ("obs", C.c_void_p), ("actions_out", C.c_void_p), ("q", C.c_void_p),
                ("stats", C.c_void_p), ("reserved", C.c_uint64)]


# ---- the data log summarised on the device (include/fleet_hip.h fleet_log_summary_dev) ----------------------------------------
LOG_SUMMARY_SCALARS = ("rows", "reward", "cashflow", "penalty", "overload", "soc_violation", "violations", "deg_rows")
LOG_SUMMARY_MAX_BINS = 256


class FleetLogSummaryArgs(C.Structure):
    _fields_ = [("drop_last", C.c_int32), ("bins", C.c_int32), ("hist_ev", C.c_int32), ("reserved", C.c_int32),
                ("lo", C.c_double), ("hi", C.c_double), ("scal", C.c_void_p), ("deg_sum", C.c_void_p), ("soh_last", C.c_void_p),
                ("prof_sum", C.c_void_p), ("prof_cnt", C.c_void_p), ("hist", C.c_void_p)]


# ---- env state (include/fleet_hip.h "env state": FleetStateLayout / FleetStateHeader, FLEET_SEC_*) ---------------------------
STATE_MAGIC = 0x4554415453544C46
STATE_ALIGN = 256
STATE_SECTIONS = 16
# section id -> (name, dtype, shape as a function of the header's numbers)
STATE_SECTION_NAMES = ("hot", "run", "soh", "soc_deg", "sei", "env", "night_start", "last_len", "rf_rows", "log_pos", "log_row",
                       "log_env", "log_ev", "log_obs", "sched")
SEC_SCHED = 14


class FleetStateSection(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint64)]


class FleetStateLayout(C.Structure):
    _fields_ = [("struct_bytes", C.c_int32), ("alignment", C.c_int32), ("header_bytes", C.c_uint64), ("total_bytes", C.c_uint64),
                ("num_envs", C.c_int32), ("num_cars", C.c_int32), ("obs_dim", C.c_int32), ("stack_cap", C.c_int32),
                ("rf_row_stride", C.c_int32), ("log_cap", C.c_int32), ("sec", FleetStateSection * STATE_SECTIONS)]


class FleetStateFingerprint(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_cars", "table_rows", "episode_steps", "deg_mode", "real_time", "price_lookahead",
                                          "bl_pv_lookahead", "include_building", "include_pv", "aux", "normalize", "stack_cap",
                                          "rf_row_stride", "log_cap", "picker_mode", "reserved")] + \
               [("seed", C.c_uint64), ("dt", C.c_double), ("table_hash", C.c_uint64)]


class FleetStateHeader(C.Structure):
    _fields_ = [("magic", C.c_uint64), ("abi_version", C.c_int32), ("header_bytes", C.c_int32), ("fp", FleetStateFingerprint)] + \
               [(n, C.c_int32) for n in ("num_envs", "env_id_offset", "obs_dim", "night_hour", "night_minute", "night_limit_s",
                                          "rf_count_all", "sched_n")] + \
               [("total_bytes", C.c_uint64), ("sec", FleetStateSection * STATE_SECTIONS)]


def pack_tables(tables, time_feat: np.ndarray | None):
    """Returns (FleetTablesC, keepalive list).  Arrays are made contiguous with the ABI's dtypes."""
    keep = []

    def ptr(a, dtype, ctype):
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ctype))

    t = FleetTablesC()
    t.there = ptr(tables.there, np.uint8, C.c_uint8)
    t.time_left = ptr(tables.time_left, np.float32, C.c_float)
    t.soc_on_return = ptr(tables.soc_on_return, np.float64, C.c_double)
    for name in ("delu", "tariff", "prc", "trc", "load", "pv"):
        setattr(t, name, ptr(np.nan_to_num(getattr(tables, name), nan=0.0), np.float64, C.c_double))
    for name in ("hour", "minute", "month", "weekday"):
        setattr(t, name, ptr(getattr(tables, name), np.uint8, C.c_uint8))
    if time_feat is not None:
        t.time_feat = ptr(time_feat, np.float32, C.c_float)
    else:
        t.time_feat = C.POINTER(C.c_float)()
    irr = getattr(tables, "meta", {}).get("irregular")
    if irr is not None:  # attached by fleetrl_amd.params.make_params for a real_time config on an irregular grid
        t.dt_row = ptr(irr["dt_row"], np.float64, C.c_double)
        t.finish_row = ptr(irr["finish_row"], np.int32, C.c_int32)
        t.lookahead_row = ptr(irr["lookahead_row"], np.int32, C.c_int32)
        t.lookahead_cols = int(irr["lookahead_row"].shape[1])
        t.second = ptr(irr["second"], np.uint8, C.c_uint8)
        t.pick_rows = ptr(irr["pick_rows"], np.int32, C.c_int32)
        t.n_pick_rows = int(irr["pick_rows"].size)
    return t, keep


class FleetHipError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"fleet_hip status {status}: {message}")
        self.status = status


_LIB = None
LIB_NAME = "libfleet_hip.so"


def lib_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)


def load_library():
    """Load the in-tree HIP library; raises (never falls back) when it is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    # not built yet (fresh checkout) or older than its sources: compile it now if the ROCm toolchain is here -- still the HIP
    # library, never a substitute for it.  Without hipcc an existing library is used as it is.
    why = ""
    try:
        from . import build as _build

        have_hipcc = True
        try:
            _build.hipcc()
        except RuntimeError:
            have_hipcc = False
        if have_hipcc and _build.needs_build():
            _build.build()
    except Exception as exc:  # compile error: say so instead of reporting a merely "missing" library
        why = f"  Building it failed: {exc}"
        if os.path.isfile(path):
            raise FleetHipError(ERR_INVALID, f"{path} is older than its sources and rebuilding it failed: {exc}") from exc
    if not os.path.isfile(path):
        raise FleetHipError(ERR_NODEVICE, f"{path} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                                          f"(hipcc --offload-arch=gfx950).  There is no CPU fallback.{why}")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 and only finds the GPU if that copy is the one
    # that gets loaded; loading this library first would pull in /opt/rocm's copy instead ("No HIP GPUs are available"
    # on the first torch.cuda call afterwards).  Importing torch first makes the order deterministic.
    try:
        import torch  # noqa: F401
    except ImportError:  # pure C-ABI use without PyTorch: the system runtime is the only one
        pass
    lib = C.CDLL(path)
    vp, i32p, u8p, f32p, f64p = C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p
    lib.fleet_obs_dim.argtypes = [C.POINTER(FleetParams)]
    lib.fleet_obs_dim.restype = C.c_int
    lib.fleet_create.argtypes = [C.POINTER(FleetParams), C.POINTER(FleetTablesC), C.c_int, C.POINTER(vp)]
    lib.fleet_destroy.argtypes = [vp]
    lib.fleet_last_error.argtypes = [vp]
    lib.fleet_last_error.restype = C.c_char_p
    lib.fleet_set_stream.argtypes = [vp, vp]
    lib.fleet_get_stream.argtypes = [vp, C.POINTER(vp)]
    lib.fleet_use_own_stream.argtypes = [vp]
    lib.fleet_stream_query.argtypes = [vp]
    lib.fleet_stream_query.restype = C.c_int
    lib.fleet_log_dropped.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.fleet_log_capacity.argtypes = [vp]
    lib.fleet_log_read.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.fleet_log_clear.argtypes = [vp]
    lib.fleet_log_summary_dev.argtypes = [vp, C.POINTER(FleetLogSummaryArgs), C.c_size_t]
    lib.fleet_synchronize.argtypes = [vp]
    lib.fleet_set_start_schedule.argtypes = [vp, vp, C.c_int]
    lib.fleet_reset_dev.argtypes = [vp, u8p, f32p]
    lib.fleet_step_dev.argtypes = [vp, vp, C.c_int, f32p, f64p, u8p, f32p]
    lib.fleet_step_many_dev.argtypes = [vp, C.c_int, vp, C.c_int, f32p, f64p, vp]
    lib.fleet_rollout_policy_dev.argtypes = [vp, C.c_int, C.c_int, f32p, f64p, vp]
    lib.fleet_set_night_policy.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.fleet_lp_plan_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    if hasattr(lib, "fleet_set_rainflow_count_all"):  # (absent from the older libraries the A/B scripts run beside the tree's)
        lib.fleet_set_rainflow_count_all.argtypes = [vp, C.c_int]
        lib.fleet_set_rainflow_count_all.restype = C.c_int
    lib.fleet_reset_host.argtypes = [vp, u8p, f32p]
    lib.fleet_step_host.argtypes = [vp, vp, C.c_int, f32p, f64p, u8p, f32p]
    lib.fleet_get.argtypes = [vp, C.c_int, vp]
    lib.fleet_get_dev.argtypes = [vp, C.c_int, vp]
    lib.fleet_get_dist_factor.argtypes = [vp, vp]
    lib.fleet_check_errors.argtypes = [vp]
    lib.fleet_last_step_error_bits.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.fleet_timer_start.argtypes = [vp]
    lib.fleet_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    lib.fleet_last_step_episodes.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_double)),
                                             C.POINTER(C.POINTER(C.c_int32))]
    lib.fleet_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    lib.fleet_host_free.argtypes = [vp]
    lib.fleet_timer_mark.argtypes = [vp]
    lib.fleet_timer_read.argtypes = [vp, C.POINTER(C.c_float)]
    lib.fleet_run_tape_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, f32p, f64p, u8p, C.c_int]
    lib.fleet_time_steps_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, f32p, f64p, u8p, vp]
    lib.fleet_time_regions_begin.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, f32p, f64p, u8p, C.c_int]
    lib.fleet_time_regions_read.argtypes = [vp, vp]
    lib.fleet_rccl_unique_id.argtypes = [vp]
    lib.fleet_rccl_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.fleet_rccl_comm_destroy.argtypes = [vp]
    lib.fleet_gather_episode_stats_rccl.argtypes = [vp, vp, C.c_int, vp]
    if hasattr(lib, "fleet_direct_queues"):  # (absent from older libraries the A/B scripts run beside the tree's)
        lib.fleet_direct_queues.argtypes = [vp]
        lib.fleet_direct_queues.restype = C.c_int
    if hasattr(lib, "fleet_direct_placement"):  # (ABI 9; absent from older libraries the A/B scripts run beside the tree's)
        lib.fleet_direct_placement.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.fleet_direct_split_plan.argtypes = [C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]
        lib.fleet_debug_direct_fault.argtypes = [vp, C.c_int, C.c_int]
        for name in ("fleet_direct_placement", "fleet_direct_split_plan", "fleet_debug_direct_fault"):
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "fleet_step_instance"):  # (absent from older libraries the A/B scripts run beside the tree's)
        lib.fleet_step_instance.argtypes = [C.c_int] * 8 + [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]
        lib.fleet_step_instance.restype = C.c_int
        lib.fleet_max_evs_per_lane_group.argtypes = []
        lib.fleet_max_evs_per_lane_group.restype = C.c_int
    if hasattr(lib, "fleet_set_direct_state_only"):  # (absent from older libraries the A/B scripts run beside the tree's)
        lib.fleet_set_direct_state_only.argtypes = [vp, C.c_int]
        lib.fleet_direct_packet_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.fleet_step_has_state_only.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_int32)]
        for name in ("fleet_set_direct_state_only", "fleet_direct_packet_counts", "fleet_step_has_state_only"):
            getattr(lib, name).restype = C.c_int
    if hasattr(lib, "fleet_selftest_stress"):
        lib.fleet_selftest_stress.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]
        lib.fleet_selftest_stress.restype = C.c_int
    if hasattr(lib, "fleet_selftest_division"):  # (absent from the round-4 library the A/B scripts run beside the tree's)
        lib.fleet_selftest_division.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        lib.fleet_selftest_division.restype = C.c_int
    # env state (fleet_state.hip)
    lib.fleet_state_layout.argtypes = [C.POINTER(FleetParams), C.POINTER(FleetStateLayout)]
    lib.fleet_state_table_hash.argtypes = [C.POINTER(FleetParams), C.POINTER(FleetTablesC), C.POINTER(C.c_uint64)]
    lib.fleet_state_check.argtypes = [C.POINTER(FleetParams), C.c_uint64, vp, C.c_uint64]
    lib.fleet_state_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
    for name in ("fleet_state_save_dev", "fleet_state_load_dev", "fleet_state_save_host", "fleet_state_load_host"):
        getattr(lib, name).argtypes = [vp, vp, C.c_uint64]
    lib.fleet_fork_envs.argtypes = [vp, vp, vp, vp, C.c_int]
    for name in STATE_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    # the running normaliser (fleet_norm.hip)
    dp = C.POINTER(C.c_double)
    lib.fleet_norm_create.argtypes = [C.c_int, C.POINTER(FleetNormParams), C.POINTER(vp)]
    lib.fleet_norm_destroy.argtypes = [vp]
    lib.fleet_norm_last_error.argtypes = [vp]
    lib.fleet_norm_set_stream.argtypes = [vp, vp]
    lib.fleet_norm_configure.argtypes = [vp, C.POINTER(FleetNormParams)]
    lib.fleet_norm_reset_dev.argtypes = [vp, f32p, f32p]
    lib.fleet_norm_step_dev.argtypes = [vp, f32p, f64p, u8p, f32p, f32p, f64p, f32p]
    lib.fleet_norm_get_state.argtypes = [vp, vp, vp, dp, dp, dp, dp, vp]
    lib.fleet_norm_set_state.argtypes = [vp, vp, vp, dp, dp, dp, dp, vp]
    lib.fleet_norm_original_host.argtypes = [vp, vp, vp]
    lib.fleet_reset_host_norm.argtypes = [vp, vp, f32p]
    lib.fleet_step_host_norm.argtypes = [vp, vp, vp, C.c_int, f32p, f64p, u8p, f32p]
    # the rollout buffer (fleet_rollout.hip)
    lib.fleet_rollout_layout.argtypes = [C.POINTER(FleetRolloutParams), C.POINTER(FleetRolloutLayout)]
    lib.fleet_rollout_create.argtypes = [C.c_int, C.POINTER(FleetRolloutParams), C.POINTER(vp)]
    lib.fleet_rollout_destroy.argtypes = [vp]
    lib.fleet_rollout_last_error.argtypes = [vp]
    lib.fleet_rollout_set_stream.argtypes = [vp, vp]
    lib.fleet_rollout_arrays.argtypes = [vp, C.POINTER(FleetRolloutArrays)]
    lib.fleet_rollout_slot.argtypes = [vp, C.c_int, C.POINTER(FleetRolloutSlot)]
    lib.fleet_rollout_add_dev.argtypes = [vp, C.c_int, f32p, f32p, vp, C.c_int, u8p, f32p, f32p, f32p, u8p]
    lib.fleet_rollout_finish_dev.argtypes = [vp, f32p, u8p]
    lib.fleet_rollout_gather_dev.argtypes = [vp, vp, C.c_int, f32p, f32p, f32p, f32p, f32p, f32p]
    lib.fleet_rollout_check_errors.argtypes = [vp]
    # the replay buffer (fleet_replay.hip)
    lib.fleet_replay_layout.argtypes = [C.POINTER(FleetReplayParams), C.POINTER(FleetReplayLayout)]
    lib.fleet_replay_create.argtypes = [C.c_int, C.POINTER(FleetReplayParams), C.POINTER(vp)]
    lib.fleet_replay_destroy.argtypes = [vp]
    lib.fleet_replay_last_error.argtypes = [vp]
    lib.fleet_replay_set_stream.argtypes = [vp, vp]
    lib.fleet_replay_arrays.argtypes = [vp, C.POINTER(FleetReplayArrays)]
    lib.fleet_replay_add_dev.argtypes = [vp, f32p, f32p, f32p, vp, C.c_int, u8p, f32p, u8p]
    lib.fleet_replay_gather_dev.argtypes = [vp, vp, vp, C.c_int, vp, f32p, f32p, f32p, f32p, f32p]
    lib.fleet_replay_sample_dev.argtypes = [vp, C.c_int, vp, f32p, f32p, f32p, f32p, f32p, vp, vp]
    lib.fleet_replay_check_errors.argtypes = [vp]
    lib.fleet_replay_size.argtypes = [vp, i32p, i32p, i32p, C.POINTER(C.c_uint64)]
    lib.fleet_replay_set_position.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint64]
    # the MLP policy (fleet_policy.hip)
    lib.fleet_policy_create.argtypes = [C.c_int, C.POINTER(FleetPolicyParams), f32p, C.POINTER(vp)]
    lib.fleet_policy_destroy.argtypes = [vp]
    lib.fleet_policy_last_error.argtypes = [vp]
    lib.fleet_policy_set_stream.argtypes = [vp, vp]
    lib.fleet_policy_load_host.argtypes = [vp, f32p]
    lib.fleet_policy_load_dev.argtypes = [vp, C.POINTER(vp), C.c_int]
    lib.fleet_policy_forward_dev.argtypes = [vp, f32p, C.c_int, vp, f32p, f32p]
    lib.fleet_policy_describe.argtypes = [vp, C.POINTER(FleetPolicyParams)]
    lib.fleet_explore_act_dev.argtypes = [vp, f32p, C.c_int, vp, C.POINTER(FleetExploreArgs)]
    lib.fleet_explore_act_dev.restype = C.c_int
    # the correlated noise processes (fleet_noise.hip)
    lib.fleet_noise_pink_tables.argtypes = [C.c_int, C.c_double, f32p, f32p]
    lib.fleet_noise_create.argtypes = [C.c_int, C.POINTER(FleetNoiseParams), C.POINTER(vp)]
    lib.fleet_noise_destroy.argtypes = [vp]
    lib.fleet_noise_last_error.argtypes = [vp]
    lib.fleet_noise_set_stream.argtypes = [vp, vp]
    lib.fleet_noise_next_dev.argtypes = [vp, u8p, f32p]
    lib.fleet_noise_reset_dev.argtypes = [vp, u8p]
    lib.fleet_noise_get_state_dev.argtypes = [vp, vp, vp, f32p, C.POINTER(C.c_uint64)]
    lib.fleet_noise_set_state_dev.argtypes = [vp, vp, vp, f32p, C.c_uint64]
    lib.fleet_noise_describe.argtypes = [vp, C.POINTER(FleetNoiseParams)]
    # the TD3 / DDPG target networks (fleet_qtarget.hip)
    lib.fleet_qtarget_create.argtypes = [C.c_int, C.POINTER(FleetQTargetParams), f32p, C.POINTER(vp)]
    lib.fleet_qtarget_destroy.argtypes = [vp]
    lib.fleet_qtarget_last_error.argtypes = [vp]
    lib.fleet_qtarget_set_stream.argtypes = [vp, vp]
    lib.fleet_qtarget_load_host.argtypes = [vp, f32p]
    lib.fleet_qtarget_load_dev.argtypes = [vp, C.POINTER(vp), C.c_int]
    lib.fleet_qtarget_polyak_dev.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_double]
    lib.fleet_qtarget_export_dev.argtypes = [vp, C.POINTER(vp), C.c_int]
    lib.fleet_qtarget_target_dev.argtypes = [vp, f32p, f32p, f32p, C.c_int, C.POINTER(FleetQTargetArgs)]
    lib.fleet_qtarget_describe.argtypes = [vp, C.POINTER(FleetQTargetParams)]
    # PPO's minibatch gradients (fleet_ppo.hip)
    lib.fleet_ppo_create.argtypes = [vp, C.POINTER(FleetPpoParams), C.POINTER(vp)]
    lib.fleet_ppo_destroy.argtypes = [vp]
    lib.fleet_ppo_last_error.argtypes = [vp]
    lib.fleet_ppo_describe.argtypes = [vp, C.POINTER(FleetPpoParams), C.POINTER(C.c_uint64), i32p]
    lib.fleet_ppo_grad_dev.argtypes = [vp, C.POINTER(FleetPpoGradArgs), C.POINTER(vp), C.c_int]
    lib.fleet_ppo_grad_vclip_dev.argtypes = [vp, C.POINTER(FleetPpoGradVclipArgs), C.POINTER(vp), C.c_int]
    # TD3's minibatch gradients (fleet_td3.hip)
    lib.fleet_td3_create.argtypes = [vp, C.POINTER(FleetTd3Params), C.POINTER(vp)]
    lib.fleet_td3_destroy.argtypes = [vp]
    lib.fleet_td3_last_error.argtypes = [vp]
    lib.fleet_td3_describe.argtypes = [vp, C.POINTER(FleetTd3Params), C.POINTER(C.c_uint64), i32p]
    lib.fleet_td3_critic_grad_dev.argtypes = [vp, C.POINTER(FleetTd3CriticArgs), C.POINTER(vp), C.c_int]
    lib.fleet_td3_actor_grad_dev.argtypes = [vp, C.POINTER(FleetTd3ActorArgs), C.POINTER(vp), C.c_int]
    # Adam on a weight image (fleet_adam.hip)
    lib.fleet_adam_create_policy.argtypes = [vp, C.POINTER(FleetAdamParams), C.POINTER(vp)]
    lib.fleet_adam_create_qtarget.argtypes = [vp, C.POINTER(FleetAdamParams), C.POINTER(vp)]
    lib.fleet_adam_destroy.argtypes = [vp]
    lib.fleet_adam_last_error.argtypes = [vp]
    lib.fleet_adam_describe.argtypes = [vp, C.POINTER(FleetAdamParams), C.POINTER(FleetAdamInfo)]
    lib.fleet_adam_step_dev.argtypes = [vp, C.POINTER(FleetAdamStepArgs), C.POINTER(vp), C.POINTER(vp), C.c_int]
    lib.fleet_adam_state_dev.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(C.c_int64)]
    lib.fleet_adam_export_image_dev.argtypes = [vp, C.POINTER(vp), C.c_int]
    # PPO's whole update (fleet_train.hip)
    lib.fleet_train_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
    lib.fleet_train_destroy.argtypes = [vp]
    lib.fleet_train_last_error.argtypes = [vp]
    lib.fleet_train_describe.argtypes = [vp, C.POINTER(FleetTrainInfo)]
    lib.fleet_train_ppo_dev.argtypes = [vp, C.POINTER(FleetTrainPpoArgs), C.POINTER(vp), C.POINTER(vp), C.c_int]
    lib.fleet_train_indices_dev.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, vp]
    lib.fleet_train_ppo_vclip_dev.argtypes = [vp, C.POINTER(FleetTrainPpoVclipArgs), C.POINTER(vp), C.POINTER(vp), C.c_int]
    lib.fleet_train_describe_vclip.argtypes = [vp, C.POINTER(C.c_uint64)]
    for name in VCLIP_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    # early stopping on approx_kl (fleet_ppo.hip, fleet_adam.hip, fleet_train.hip)
    lib.fleet_ppo_grad_gated_dev.argtypes = [vp, C.POINTER(FleetPpoGradGatedArgs), C.POINTER(vp), C.c_int]
    lib.fleet_adam_step_gated_dev.argtypes = [vp, C.POINTER(FleetAdamStepArgs), C.POINTER(vp), C.POINTER(vp), C.c_int, vp]
    lib.fleet_adam_settle_dev.argtypes = [vp, C.c_int64, vp]
    lib.fleet_train_ppo_kl_dev.argtypes = [vp, C.POINTER(FleetTrainPpoKlArgs), C.POINTER(vp), C.POINTER(vp), C.c_int]
    for name in KL_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    # TD3 / DDPG's whole update (fleet_offpolicy.hip)
    lib.fleet_offpolicy_create.argtypes = [vp, vp, vp, vp, vp, C.POINTER(FleetOffpolicyParams), C.POINTER(vp)]
    lib.fleet_offpolicy_destroy.argtypes = [vp]
    lib.fleet_offpolicy_last_error.argtypes = [vp]
    lib.fleet_offpolicy_describe.argtypes = [vp, C.POINTER(FleetOffpolicyInfo)]
    lib.fleet_offpolicy_td3_dev.argtypes = [vp, C.POINTER(FleetOffpolicyArgs), C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(vp),
                                            C.POINTER(vp), C.c_int]
    lib.fleet_offpolicy_polyak_dev.argtypes = [vp, C.c_double]
    # SAC's actor and soft targets (fleet_sac.hip), on a fleet_qtarget handle
    lib.fleet_sac_create.argtypes = [C.c_int, C.POINTER(FleetSacParams), f32p, C.POINTER(vp)]
    lib.fleet_sac_last_error.argtypes = [vp]
    lib.fleet_sac_act_dev.argtypes = [vp, f32p, C.c_int, vp, C.POINTER(FleetSacActArgs)]
    lib.fleet_sac_target_dev.argtypes = [vp, vp, f32p, f32p, f32p, C.c_int, C.POINTER(FleetSacTargetArgs)]
    for name in SAC_SYMBOLS:
        getattr(lib, name).restype = C.c_char_p if name == "fleet_sac_last_error" else C.c_int
    # SAC's actor and entropy-coefficient gradients (fleet_td3.hip), on a fleet_td3 handle
    lib.fleet_sac_actor_grad_dev.argtypes = [vp, C.POINTER(FleetSacActorArgs), C.POINTER(vp), C.c_int]
    for name in SAC_GRAD_SYMBOLS:
        getattr(lib, name).restype = C.c_int
    # SAC's whole update (fleet_sactrain.hip)
    lib.fleet_sactrain_create.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(FleetSacTrainParams), C.POINTER(vp)]
    lib.fleet_sactrain_destroy.argtypes = [vp]
    lib.fleet_sactrain_last_error.argtypes = [vp]
    lib.fleet_sactrain_describe.argtypes = [vp, C.POINTER(FleetSacTrainInfo)]
    lib.fleet_sactrain_alpha_dev.argtypes = [vp, vp, vp]
    lib.fleet_sactrain_scale_dev.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_double]
    lib.fleet_sactrain_polyak_dev.argtypes = [vp, C.c_double]
    lib.fleet_sactrain_sac_dev.argtypes = [vp, C.POINTER(FleetSacTrainArgs), C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(vp),
                                           C.POINTER(vp), C.c_int]
    for name in SACTRAIN_SYMBOLS:
        getattr(lib, name).restype = C.c_char_p if name == "fleet_sactrain_last_error" else C.c_int
    # rollout collection (fleet_collect.hip)
    lib.fleet_collect_create.argtypes = [vp, vp, vp, C.POINTER(FleetCollectParams), C.POINTER(vp)]
    lib.fleet_collect_destroy.argtypes = [vp]
    lib.fleet_collect_last_error.argtypes = [vp]
    lib.fleet_collect_describe.argtypes = [vp, C.POINTER(FleetCollectInfo)]
    lib.fleet_collect_reset_dev.argtypes = [vp, C.c_int]
    lib.fleet_collect_ppo_dev.argtypes = [vp, C.POINTER(FleetCollectPpoArgs)]
    lib.fleet_collect_offpolicy_dev.argtypes = [vp, C.POINTER(FleetCollectOffpolicyArgs)]
    lib.fleet_collect_episodes_dev.argtypes = [vp, vp, vp, vp, C.c_int]
    lib.fleet_collect_finish_dev.argtypes = [vp, C.c_uint64, C.c_int32, vp]
    lib.fleet_collect_episodes_read.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64)]
    for name in COLLECT_SYMBOLS:
        getattr(lib, name).restype = C.c_char_p if name == "fleet_collect_last_error" else C.c_int
    # evaluation of the agent (fleet_eval.hip)
    lib.fleet_eval_create.argtypes = [vp, vp, vp, C.POINTER(FleetEvalParams), C.POINTER(vp)]
    lib.fleet_eval_destroy.argtypes = [vp]
    lib.fleet_eval_last_error.argtypes = [vp]
    lib.fleet_eval_describe.argtypes = [vp, C.POINTER(FleetEvalInfo)]
    lib.fleet_eval_sync_norm_dev.argtypes = [vp, vp]
    lib.fleet_eval_run_dev.argtypes = [vp, C.POINTER(FleetEvalArgs)]
    lib.fleet_eval_episodes_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int]
    lib.fleet_eval_clear_dev.argtypes = [vp]
    lib.fleet_eval_best_load_dev.argtypes = [vp, vp]
    lib.fleet_eval_best_export_dev.argtypes = [vp, C.POINTER(vp), C.c_int]
    lib.fleet_eval_episodes_read.argtypes = [vp, vp, vp, C.POINTER(C.c_uint64)]
    for name in EVAL_SYMBOLS:
        getattr(lib, name).restype = C.c_char_p if name == "fleet_eval_last_error" else C.c_int
    # SAC's collector and evaluation (include/fleet_hip_sac_loop.h; fleet_collect.hip, fleet_eval.hip), on the collect and eval handles
    lib.fleet_saccollect_last_error.argtypes = [vp]
    lib.fleet_saccollect_uniform_dev.argtypes = [vp, C.c_int, C.POINTER(FleetSacUniformArgs)]
    lib.fleet_saccollect_create.argtypes = [vp, vp, vp, C.POINTER(FleetCollectParams), C.POINTER(vp)]
    lib.fleet_saccollect_sac_dev.argtypes = [vp, C.POINTER(FleetSacCollectArgs)]
    lib.fleet_saceval_create.argtypes = [vp, vp, vp, C.POINTER(FleetEvalParams), C.POINTER(vp)]
    lib.fleet_saceval_best_load_dev.argtypes = [vp, vp]
    for name in SACCOLLECT_SYMBOLS + SACEVAL_SYMBOLS:
        getattr(lib, name).restype = C.c_char_p if name == "fleet_saccollect_last_error" else C.c_int
    for prefix, names in (("norm", NORM_SYMBOLS), ("rollout", ROLLOUT_SYMBOLS), ("replay", REPLAY_SYMBOLS), ("policy", POLICY_SYMBOLS),
                          ("noise", NOISE_SYMBOLS), ("qtarget", QTARGET_SYMBOLS), ("ppo", PPO_SYMBOLS),
                          ("td3", TD3_SYMBOLS), ("adam", ADAM_SYMBOLS), ("train", TRAIN_SYMBOLS), ("offpolicy", OFFPOLICY_SYMBOLS)):
        for name in names:
            getattr(lib, name).restype = C.c_char_p if name == f"fleet_{prefix}_last_error" else C.c_int
    for name in ("fleet_create", "fleet_destroy", "fleet_set_stream", "fleet_get_stream", "fleet_use_own_stream", "fleet_log_dropped",
                 "fleet_log_capacity", "fleet_log_read",
                 "fleet_log_clear", "fleet_log_summary_dev", "fleet_synchronize", "fleet_set_start_schedule",
                 "fleet_reset_dev", "fleet_step_dev", "fleet_step_many_dev", "fleet_rollout_policy_dev", "fleet_set_night_policy",
                 "fleet_reset_host", "fleet_step_host", "fleet_get", "fleet_get_dev", "fleet_get_dist_factor", "fleet_check_errors", "fleet_timer_start",
                 "fleet_timer_stop", "fleet_timer_mark", "fleet_timer_read", "fleet_run_tape_dev", "fleet_time_steps_dev",
                 "fleet_host_alloc", "fleet_host_free", "fleet_last_step_episodes", "fleet_last_step_error_bits",
                 "fleet_time_regions_begin", "fleet_time_regions_read", "fleet_rccl_unique_id", "fleet_rccl_comm_create",
                 "fleet_rccl_comm_destroy", "fleet_gather_episode_stats_rccl"):
        getattr(lib, name).restype = C.c_int
    _LIB = lib
    return lib


NORM_SYMBOLS = (
    "fleet_norm_create", "fleet_norm_destroy", "fleet_norm_last_error", "fleet_norm_set_stream", "fleet_norm_configure",
    "fleet_norm_reset_dev", "fleet_norm_step_dev", "fleet_norm_get_state", "fleet_norm_set_state", "fleet_norm_original_host",
    "fleet_reset_host_norm", "fleet_step_host_norm",
)

STATE_SYMBOLS = (
    "fleet_state_layout", "fleet_state_table_hash", "fleet_state_check", "fleet_state_bytes", "fleet_state_save_dev",
    "fleet_state_load_dev", "fleet_state_save_host", "fleet_state_load_host", "fleet_fork_envs",
)

ROLLOUT_SYMBOLS = (
    "fleet_rollout_layout", "fleet_rollout_create", "fleet_rollout_destroy", "fleet_rollout_last_error", "fleet_rollout_set_stream",
    "fleet_rollout_arrays", "fleet_rollout_slot", "fleet_rollout_add_dev", "fleet_rollout_finish_dev", "fleet_rollout_gather_dev",
    "fleet_rollout_check_errors",
)

REPLAY_SYMBOLS = (
    "fleet_replay_layout", "fleet_replay_create", "fleet_replay_destroy", "fleet_replay_last_error", "fleet_replay_set_stream",
    "fleet_replay_arrays", "fleet_replay_add_dev", "fleet_replay_gather_dev", "fleet_replay_sample_dev", "fleet_replay_check_errors",
    "fleet_replay_size", "fleet_replay_set_position",
)

POLICY_SYMBOLS = (
    "fleet_policy_create", "fleet_policy_destroy", "fleet_policy_last_error", "fleet_policy_set_stream", "fleet_policy_load_host",
    "fleet_policy_load_dev", "fleet_policy_forward_dev", "fleet_policy_describe",
)

EXPLORE_SYMBOLS = ("fleet_explore_act_dev",)

NOISE_SYMBOLS = (
    "fleet_noise_pink_tables", "fleet_noise_create", "fleet_noise_destroy", "fleet_noise_last_error", "fleet_noise_set_stream",
    "fleet_noise_next_dev", "fleet_noise_reset_dev", "fleet_noise_get_state_dev", "fleet_noise_set_state_dev", "fleet_noise_describe",
)

QTARGET_SYMBOLS = (
    "fleet_qtarget_create", "fleet_qtarget_destroy", "fleet_qtarget_last_error", "fleet_qtarget_set_stream", "fleet_qtarget_load_host",
    "fleet_qtarget_load_dev", "fleet_qtarget_polyak_dev", "fleet_qtarget_export_dev", "fleet_qtarget_target_dev", "fleet_qtarget_describe",
)

PPO_SYMBOLS = ("fleet_ppo_create", "fleet_ppo_destroy", "fleet_ppo_last_error", "fleet_ppo_describe", "fleet_ppo_grad_dev")

TD3_SYMBOLS = ("fleet_td3_create", "fleet_td3_destroy", "fleet_td3_last_error", "fleet_td3_describe", "fleet_td3_critic_grad_dev",
               "fleet_td3_actor_grad_dev")

ADAM_SYMBOLS = ("fleet_adam_create_policy", "fleet_adam_create_qtarget", "fleet_adam_destroy", "fleet_adam_last_error", "fleet_adam_describe",
                "fleet_adam_step_dev", "fleet_adam_state_dev", "fleet_adam_export_image_dev")

TRAIN_SYMBOLS = ("fleet_train_create", "fleet_train_destroy", "fleet_train_last_error", "fleet_train_describe", "fleet_train_ppo_dev",
                 "fleet_train_indices_dev")

# value-function clipping on the fleet_ppo and fleet_train handles: the header declares these `extern`, behind the two families' own
# (closed) entry lists, so they stand in a list of their own here as well
VCLIP_SYMBOLS = ("fleet_ppo_grad_vclip_dev", "fleet_train_ppo_vclip_dev", "fleet_train_describe_vclip")

# early stopping on approx_kl (target_kl) on the fleet_ppo, fleet_adam and fleet_train handles: the header declares these `FLEET_API int`,
# behind the three families' own (closed) entry lists
KL_SYMBOLS = ("fleet_ppo_grad_gated_dev", "fleet_adam_step_gated_dev", "fleet_adam_settle_dev", "fleet_train_ppo_kl_dev")

OFFPOLICY_SYMBOLS = ("fleet_offpolicy_create", "fleet_offpolicy_destroy", "fleet_offpolicy_last_error", "fleet_offpolicy_describe",
                     "fleet_offpolicy_td3_dev", "fleet_offpolicy_polyak_dev")

SAC_SYMBOLS = ("fleet_sac_create", "fleet_sac_last_error", "fleet_sac_act_dev", "fleet_sac_target_dev")

# SAC's actor and entropy-coefficient gradients on the fleet_td3 handle: the header declares the entry `extern FLEET_API int`, behind the SAC
# family's own (closed) entry list, so it stands in a list of its own here as well
SAC_GRAD_SYMBOLS = ("fleet_sac_actor_grad_dev",)

# SAC's whole update: the header declares these `FLEET_API extern`, behind every closed entry list, so they stand in a list of their own
SACTRAIN_SYMBOLS = ("fleet_sactrain_create", "fleet_sactrain_destroy", "fleet_sactrain_last_error", "fleet_sactrain_describe",
                    "fleet_sactrain_alpha_dev", "fleet_sactrain_scale_dev", "fleet_sactrain_polyak_dev", "fleet_sactrain_sac_dev")

COLLECT_SYMBOLS = ("fleet_collect_create", "fleet_collect_destroy", "fleet_collect_last_error", "fleet_collect_describe",
                   "fleet_collect_reset_dev", "fleet_collect_ppo_dev", "fleet_collect_offpolicy_dev", "fleet_collect_episodes_dev",
                   "fleet_collect_finish_dev", "fleet_collect_episodes_read")

EVAL_SYMBOLS = ("fleet_eval_create", "fleet_eval_destroy", "fleet_eval_last_error", "fleet_eval_describe", "fleet_eval_sync_norm_dev",
                "fleet_eval_run_dev", "fleet_eval_episodes_dev", "fleet_eval_clear_dev", "fleet_eval_best_load_dev", "fleet_eval_best_export_dev",
                "fleet_eval_episodes_read")

# SAC's collector and evaluation: declared in a header of their own, include/fleet_hip_sac_loop.h (fleet_hip.h and its closed entry lists
# stay as they are), so they stand in lists of their own, outside EXPORTED_SYMBOLS
SACCOLLECT_SYMBOLS = ("fleet_saccollect_last_error", "fleet_saccollect_uniform_dev", "fleet_saccollect_create", "fleet_saccollect_sac_dev")

SACEVAL_SYMBOLS = ("fleet_saceval_create", "fleet_saceval_best_load_dev")

EXPORTED_SYMBOLS = (
    "fleet_obs_dim", "fleet_create", "fleet_destroy", "fleet_last_error", "fleet_set_stream", "fleet_get_stream", "fleet_use_own_stream",
    "fleet_synchronize", "fleet_stream_query", "fleet_log_capacity", "fleet_log_dropped", "fleet_log_read", "fleet_log_clear",
    "fleet_log_summary_dev", "fleet_set_start_schedule", "fleet_reset_dev", "fleet_step_dev", "fleet_step_many_dev", "fleet_rollout_policy_dev",
    "fleet_set_night_policy", "fleet_reset_host",
    "fleet_step_host", "fleet_get", "fleet_get_dev", "fleet_get_dist_factor", "fleet_check_errors", "fleet_timer_start",
    "fleet_timer_stop", "fleet_timer_mark", "fleet_timer_read", "fleet_run_tape_dev", "fleet_time_steps_dev",
    "fleet_host_alloc", "fleet_host_free", "fleet_last_step_episodes", "fleet_last_step_error_bits",
    "fleet_time_regions_begin", "fleet_time_regions_read", "fleet_rccl_unique_id", "fleet_rccl_comm_create",
    "fleet_rccl_comm_destroy", "fleet_gather_episode_stats_rccl", "fleet_selftest_division", "fleet_direct_queues", "fleet_selftest_stress",
    "fleet_direct_placement", "fleet_direct_split_plan", "fleet_debug_direct_fault", "fleet_set_rainflow_count_all",
    "fleet_lp_plan_dev", "fleet_step_instance", "fleet_max_evs_per_lane_group",
    "fleet_set_direct_state_only", "fleet_direct_packet_counts", "fleet_step_has_state_only",
) + NORM_SYMBOLS + STATE_SYMBOLS + ROLLOUT_SYMBOLS + REPLAY_SYMBOLS + POLICY_SYMBOLS + EXPLORE_SYMBOLS + NOISE_SYMBOLS + QTARGET_SYMBOLS + PPO_SYMBOLS + TD3_SYMBOLS + ADAM_SYMBOLS + TRAIN_SYMBOLS + OFFPOLICY_SYMBOLS + SAC_SYMBOLS + COLLECT_SYMBOLS + EVAL_SYMBOLS


def step_instance(num_envs: int, num_cars: int, deg_mode: int, real_time: bool, log_data: bool, act_mode: int = ACT_F32, K: int = 1,
                  has_done_count: bool = False) -> tuple[str, int]:
    """(name, grid) of the step-kernel instance a launch of this kind takes (include/fleet_hip.h fleet_step_instance; needs the
    library, but no GPU)."""
    name = C.create_string_buffer(64)
    grid = C.c_uint32()
    rc = load_library().fleet_step_instance(int(num_envs), int(num_cars), int(deg_mode), int(bool(real_time)), int(bool(log_data)),
                                            int(act_mode), int(K), int(bool(has_done_count)), name, len(name), C.byref(grid))
    if rc != OK:
        raise FleetHipError(rc, "fleet_step_instance: argument out of range")
    return name.value.decode(), int(grid.value)


def step_has_state_only(num_envs: int, num_cars: int, deg_mode: int, real_time: bool, log_data: bool, act_mode: int = ACT_F32, K: int = 1,
                        has_done_count: bool = False) -> bool:
    """Whether a launch of this kind has a state-only twin, which a run on the library's own queue takes for every launch but its
    last (include/fleet_hip.h fleet_step_has_state_only; needs the library, but no GPU)."""
    out = C.c_int32()
    rc = load_library().fleet_step_has_state_only(int(num_envs), int(num_cars), int(deg_mode), int(bool(real_time)), int(bool(log_data)),
                                                  int(act_mode), int(K), int(bool(has_done_count)), C.byref(out))
    if rc != OK:
        raise FleetHipError(rc, "fleet_step_has_state_only: argument out of range")
    return bool(out.value)


def _layout(prefix: str, params, out):
    """fleet_<prefix>_layout of `params` into `out`."""
    lib = load_library()
    rc = getattr(lib, f"fleet_{prefix}_layout")(C.byref(params), C.byref(out))
    if rc != OK:
        raise FleetHipError(rc, getattr(lib, f"fleet_{prefix}_last_error")(None).decode())
    return out


def pink_tables(seq_len: int, beta: float = 1.0):
    """fleet_noise_pink_tables: (gain f32 [seq_len // 2 + 1], twiddle f32 [seq_len, 2]) as the library builds them (no GPU)."""
    lib = load_library()
    gain, twiddle = np.zeros(max(int(seq_len), 0) // 2 + 1, np.float32), np.zeros((max(int(seq_len), 0), 2), np.float32)
    rc = lib.fleet_noise_pink_tables(int(seq_len), float(beta), gain.ctypes.data, twiddle.ctypes.data)
    if rc != OK:
        raise FleetHipError(rc, lib.fleet_noise_last_error(None).decode())
    return gain, twiddle


def rollout_layout(num_envs: int, n_steps: int, obs_dim: int, act_dim: int, gamma: float = 0.99,
                   gae_lambda: float = 0.95) -> FleetRolloutLayout:
    """fleet_rollout_layout: bytes and offsets of the rollout buffer's arrays (needs the library, no GPU)."""
    p = FleetRolloutParams(C.sizeof(FleetRolloutParams), int(num_envs), int(n_steps), int(obs_dim), int(act_dim), 0, float(gamma),
                           float(gae_lambda))
    return _layout("rollout", p, FleetRolloutLayout())


def replay_layout(buffer_size: int, num_envs: int, obs_dim: int, act_dim: int) -> FleetReplayLayout:
    """fleet_replay_layout: rows, bytes and offsets of the replay buffer's arrays (needs the library, no GPU)."""
    p = FleetReplayParams(C.sizeof(FleetReplayParams), int(num_envs), int(buffer_size), int(obs_dim), int(act_dim), 0, 0)
    return _layout("replay", p, FleetReplayLayout())


def state_layout(params: FleetParams) -> FleetStateLayout:
    """fleet_state_layout: sizes and offsets of every section of a state blob for these parameters (needs the library, no GPU)."""
    out = FleetStateLayout()
    lib = load_library()
    if lib.fleet_state_layout(C.byref(params), C.byref(out)) != OK:
        raise FleetHipError(ERR_INVALID, lib.fleet_last_error(None).decode())
    return out


def state_table_hash(params: FleetParams, tables, time_feat=None) -> int:
    """fleet_state_table_hash: the hash of the table contents a handle created from them carries in its fingerprint (no GPU)."""
    tc, keep = pack_tables(tables, time_feat)
    out = C.c_uint64()
    lib = load_library()
    rc = lib.fleet_state_table_hash(C.byref(params), C.byref(tc), C.byref(out))
    del keep
    if rc != OK:
        raise FleetHipError(rc, lib.fleet_last_error(None).decode())
    return int(out.value)


def state_check(params: FleetParams, table_hash: int, blob: np.ndarray) -> None:
    """fleet_state_check: raises FleetHipError (ERR_INVALID, naming the field) unless the host blob fits these parameters and tables."""
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    lib = load_library()
    rc = lib.fleet_state_check(C.byref(params), int(table_hash), b.ctypes.data, b.size)
    if rc != OK:
        raise FleetHipError(rc, lib.fleet_last_error(None).decode())


# dtypes of the structured sections (fleetrl_amd/csrc/fleet_device.h: Hot, SegRec, SeiRec, EnvRec)
HOT_DTYPE = np.dtype([("x", "<f8"), ("hl", "<f4"), ("bits", "<u4")])
RUN_DTYPE = np.dtype([("sor", "<f8"), ("tlx", "<u4"), ("se", "<u4")])
SEI_DTYPE = np.dtype([("fd_cyc", "<f8"), ("fd_cal", "<f8"), ("sei_l", "<f8"), ("sei_soh", "<f8")])
ENV_DTYPE = np.dtype([("t", "<i4"), ("t_end", "<i4"), ("nsamp", "<i4"), ("episodes", "<i4"), ("ep_len", "<i4"), ("rf_until", "<i4"),
                      ("err", "<u4"), ("start_done", "<i4"), ("ep_return", "<f8"), ("last_ep_return", "<f8"), ("cashflow", "<f8"),
                      ("penalty_record", "<f8")])


def state_header(blob: np.ndarray) -> FleetStateHeader:
    b = np.ascontiguousarray(blob[:C.sizeof(FleetStateHeader)], dtype=np.uint8)
    if b.size < C.sizeof(FleetStateHeader):
        raise FleetHipError(ERR_INVALID, "the blob is shorter than a header")
    h = FleetStateHeader.from_buffer_copy(b.tobytes())
    if h.magic != STATE_MAGIC:
        raise FleetHipError(ERR_INVALID, "magic: not a fleet state blob")
    return h


def state_views(blob: np.ndarray) -> dict:
    """Named NumPy views of a host blob's sections, shaped by the blob's own header: {"header": u8 view of the header bytes,
    "hot": [E,N] records, "run", "soh", "soc_deg", "sei", "env": [E] records, "night_start", "last_len", "rf_rows": [E,N,stride]
    f64, "log_*", "sched": [n,E] i32}; absent sections are left out.  Views: writing to them edits the blob."""
    if blob.dtype != np.uint8 or blob.ndim != 1 or not blob.flags.c_contiguous:
        raise ValueError("a state blob is a contiguous 1-d uint8 array")
    h = state_header(blob)
    if h.total_bytes > blob.size:
        raise FleetHipError(ERR_INVALID, "the blob is shorter than its header says")
    E, N, D, cap, stride = h.num_envs, h.fp.num_cars, h.obs_dim, h.fp.log_cap, h.fp.rf_row_stride
    shapes = {"hot": (HOT_DTYPE, (E, N)), "run": (RUN_DTYPE, (E, N)), "soh": (np.float64, (E, N)), "soc_deg": (np.float64, (E, N)),
              "sei": (SEI_DTYPE, (E, N)), "env": (ENV_DTYPE, (E,)), "night_start": (np.int32, (E,)), "last_len": (np.int32, (E,)),
              "rf_rows": (np.float64, (E, N, stride)), "log_pos": (np.int32, (E,)), "log_row": (np.int32, (cap, E)),
              "log_env": (np.float64, (cap, E, 4)), "log_ev": (np.float64, (cap, E, 4, N)), "log_obs": (np.float32, (cap, E, D)),
              "sched": (np.int32, (h.sched_n, E))}
    out = {"header": blob[:C.sizeof(FleetStateHeader)]}
    for s, name in enumerate(STATE_SECTION_NAMES):
        off, n = int(h.sec[s].offset), int(h.sec[s].bytes)
        if not n:
            continue
        dtype, shape = shapes[name]
        if off % STATE_ALIGN or off + n > blob.size or n != int(np.prod(shape)) * np.dtype(dtype).itemsize:
            raise FleetHipError(ERR_INVALID, f"section {name!r} of the blob does not match its header")
        out[name] = blob[off:off + n].view(dtype).reshape(shape)
    return out


def state_from_views(d: dict) -> np.ndarray:
    """The blob a `state_views` dict describes, rebuilt from the arrays (which may be copies, e.g. read back from an .npz)."""
    hb = np.ascontiguousarray(d["header"], dtype=np.uint8).reshape(-1)
    h = state_header(hb)
    blob = np.zeros(int(h.total_bytes), dtype=np.uint8)
    blob[:hb.size] = hb
    views = state_views(blob)
    for name, v in views.items():
        if name == "header":
            continue
        if name not in d:
            raise FleetHipError(ERR_INVALID, f"the state lacks section {name!r}")
        a = np.asarray(d[name])
        if a.dtype != v.dtype or a.shape != v.shape:
            raise FleetHipError(ERR_INVALID, f"section {name!r}: expected {v.dtype} {v.shape}, got {a.dtype} {a.shape}")
        v[...] = a
    return blob
