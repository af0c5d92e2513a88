// fleet_norm.h -- what the env's host path (fleet_hostpath.hip) needs of the normaliser (fleet_norm.hip).
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
// fleet_eval_sync_norm_dev (fleet_eval.hip): FLEET_OK, or FLEET_ERR_INVALID with the reason in *why, when src's statistics cannot go
// into dst (a null handle, another D, another device); and the copy itself, one launch on dst's stream behind src's last launch
int fleet_norm_check_sync(fleet_norm_handle dst, fleet_norm_handle src, std::string* why);
hipError_t fleet_norm_enqueue_sync(fleet_norm_handle dst, fleet_norm_handle src);

// ---- what a reader of the statistics needs (fleet_replay.hip: the sample-time normalisation of the replay buffer) -----------------
// The arithmetic of norm_apply, shared instead of restated: obs' = (float)clip(((double)x - mean) / sd, +-clip_obs) and
// r' = clip(r / ret_sd, +-clip_reward), both in float64.
__device__ inline double fleet_norm_clip(double v, double c) { return v < -c ? -c : (v > c ? c : v); }
__device__ inline float fleet_norm_obs1(float x, double m, double s, double c) { return (float)fleet_norm_clip(((double)x - m) / s, c); }
__device__ inline double fleet_norm_reward1(double r, double ret_sd, double c) { return fleet_norm_clip(r / ret_sd, c); }

struct FleetNormView {
  const double* obs_mean;  // [D]
  const double* obs_sd;    // [D]: sqrt(var + epsilon)
  const double* ret_stat;  // {mean, var, sd, -} of the returns
  double clip_obs, clip_reward;
  int norm_obs, norm_reward;
  int E, D, device;
};
// Device pointers to the statistics and the settings as they are now, for kernels enqueued on stream `s`: when the normaliser's
// last launch went to another stream, `s` is made to wait for it (an event, no host synchronisation).
hipError_t fleet_norm_begin_read(fleet_norm_handle n, hipStream_t s, FleetNormView* out);
// ... and after the reader's last launch: the normaliser's next enqueue on another stream waits for it before it updates.
hipError_t fleet_norm_end_read(fleet_norm_handle n, hipStream_t s);
