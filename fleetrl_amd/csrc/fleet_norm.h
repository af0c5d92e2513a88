// fleet_norm.h -- what the env's host path (fleet_capi.hip) needs of the normaliser (fleet_norm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/fleet_hip.h"

// FLEET_OK, or FLEET_ERR_INVALID with the reason in *why, when the normaliser does not fit a batch of E envs with D-wide
// observations on `device`
int fleet_norm_check_fit(fleet_norm_handle n, int E, int D, int device, std::string* why);
// the normaliser's own [E,D] output buffer (the host path lands normalised observations there: the env's staging buffer keeps
// the raw ones for fleet_norm_original_host)
float* fleet_norm_out_buffer(fleet_norm_handle n);
// fleet_norm_reset_dev / fleet_norm_step_dev on stream `s` instead of the normaliser's own (errors are returned as hipError_t)
hipError_t fleet_norm_enqueue_reset(fleet_norm_handle n, const float* raw_obs, float* obs, hipStream_t s);
hipError_t fleet_norm_enqueue_step(fleet_norm_handle n, const float* raw_obs, const double* raw_reward, const uint8_t* done,
                                   const float* raw_terminal, float* obs, double* reward, float* terminal, hipStream_t s);
