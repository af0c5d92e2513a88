"""The reference's fourth benchmark, `LinearOptimization` (benchmarking/linear_optimization.py:55-247): a perfect-foresight
charging plan, replayed through the env.

The reference builds one pyomo MILP for one env and hands it to glpk.  The model splits into independent problems per (env, EV),
and here every one of them is solved exactly on the GPU (`fleet_lp_plan_dev`, fleetrl_amd/csrc/fleet_lp.hip): the LP
relaxation's optimum (`bound`, a lower bound on the MILP), realised with one-sided actions that satisfy every MILP constraint
(`plan_cost`, the MILP objective of the tape; `gap = plan_cost - bound`).  DESIGN.md section 8 states the model and the four
decisions where the reference's model cannot be run as it stands (start state, exclusivity, unreachable targets, same episode).
"""
from __future__ import annotations

import numpy as np

from . import _capi

__all__ = ["plan_linear_optimization", "run_linear_optimization"]


def _batch_of(env_or_batch):
    """The FleetBatch behind a FleetBatch, FleetCore, FleetVecEnv, FleetVectorEnv or FleetEnv."""
    for obj in (env_or_batch, getattr(env_or_batch, "core", None)):
        if obj is None:
            continue
        if hasattr(obj, "lp_plan_dev"):
            return obj
        if hasattr(getattr(obj, "batch", None), "lp_plan_dev"):
            return obj.batch
    raise TypeError(f"no FleetBatch behind {type(env_or_batch).__name__}")


def _plan_dev(batch, horizon: int, act_dtype: int):
    """The plan in device tensors (actions [H,E,N], soc_plan [H+1,E,N], bound [E], plan_cost [E], status [E,N])."""
    import torch

    H, E, N = int(horizon), batch.E, batch.N
    dev = torch.device("cuda", batch.device)
    batch.use_torch_stream(dev)
    act = torch.empty((H, E, N), device=dev, dtype=torch.float64 if act_dtype == _capi.ACT_F64 else torch.float32)
    soc = torch.empty((H + 1, E, N), device=dev, dtype=torch.float64)
    bound = torch.empty(E, device=dev, dtype=torch.float64)
    cost = torch.empty(E, device=dev, dtype=torch.float64)
    status = torch.empty((E, N), device=dev, dtype=torch.int32)
    batch.lp_plan_dev(H, act.data_ptr(), soc.data_ptr(), bound.data_ptr(), cost.data_ptr(), status.data_ptr(), act_dtype=act_dtype)
    return act, soc, bound, cost, status


def plan_linear_optimization(env_or_batch, horizon: int, *, act_dtype: str = "f64") -> dict:
    """Plan the next `horizon` rows of every env from its live state (time row, SOC of the plugged-in EVs).

    Returns NumPy arrays: `actions` [H,E,N] (float64, or float32 with act_dtype="f32"), `soc_plan` [H+1,E,N] (0 while an EV is
    away), `bound`, `plan_cost`, `gap` [E] in EUR (summed over the env's EVs) and `status` [E,N] (the `_capi.LP_*` bits).
    Raises `FleetHipError` when an env has fewer than `horizon` rows left in its running episode."""
    dt = {"f64": _capi.ACT_F64, "f32": _capi.ACT_F32}[act_dtype]
    batch = _batch_of(env_or_batch)
    act, soc, bound, cost, status = _plan_dev(batch, horizon, dt)
    out = {"actions": act.cpu().numpy(), "soc_plan": soc.cpu().numpy(), "bound": bound.cpu().numpy(),
           "plan_cost": cost.cpu().numpy(), "status": status.cpu().numpy()}
    out["gap"] = out["plan_cost"] - out["bound"]
    return out


def run_linear_optimization(env, horizon: int, *, chunk: int = 96):
    """Plan `horizon` rows from every env's live state and replay the plan on the same episode (decision 4): returns what
    `fleetrl_amd.policies.run_policy` returns -- (obs f32 [E, obs_dim] after the last step, reward_sum f64 [E], done_count i32
    [E]).  With `log_data` on, `env.get_log()` then holds the reference's `lin_log` rows.  The float64 tape is replayed by
    `fleet_step_many_dev` (auto-reset batches, `chunk` rows per launch) or row by row with `fleet_step_dev` (a `FleetEnv`)."""
    import torch

    batch = _batch_of(env)
    H, E = int(horizon), batch.E
    act, _soc, _b, _c, _s = _plan_dev(batch, H, _capi.ACT_F64)
    dev = act.device
    obs = torch.zeros((E, batch.obs_dim), device=dev, dtype=torch.float32)
    rtot = torch.zeros(E, device=dev, dtype=torch.float64)
    dtot = torch.zeros(E, device=dev, dtype=torch.int32)
    if batch.params.auto_reset:
        rsum = torch.zeros(E, device=dev, dtype=torch.float64)
        dcnt = torch.zeros(E, device=dev, dtype=torch.int32)
        row = 0
        while row < H:
            k = min(H - row, int(chunk))
            batch.step_many_dev(k, act[row].data_ptr(), obs.data_ptr(), rsum.data_ptr(), dcnt.data_ptr(), act_dtype=_capi.ACT_F64)
            rtot += rsum
            dtot += dcnt
            row += k
    else:
        rew = torch.zeros(E, device=dev, dtype=torch.float64)
        done = torch.zeros(E, device=dev, dtype=torch.uint8)
        for row in range(H):
            batch.step_dev(act[row].data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), act_dtype=_capi.ACT_F64)
            rtot += rew
            dtot += done.to(torch.int32)
    batch.check_errors()
    return obs.cpu().numpy(), rtot.cpu().numpy(), dtot.cpu().numpy()
