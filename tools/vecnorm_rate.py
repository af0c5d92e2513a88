"""Cost of VecNormalize on the device (fleet_norm.hip) at the bench workloads; prints one JSON line.

Per config (c3, c5; c5 = its three fleet groups, one normaliser each, stepped one after the other on one stream):
  step_us            device time per step of fleet_step_dev alone (HIP events around `steps` launches on torch's stream)
  step_norm_us       the same plus fleet_norm_step_dev (training, norm_obs, norm_reward, terminal rows)
  step_torch_ops_us  the same plus a straightforward torch-ops version of the same math
  norm_us            fleet_norm_step_dev alone on fixed inputs; norm_roof_frac = algorithmic bytes (obs read twice, written once;
                     the terminal rows of done envs read and written) / norm_us / 8 TB/s
and at c3 the host path's wall time per step: FleetVecEnv.step, FleetVecEnv.step + the NumPy VecNormalize model (what SB3's
VecNormalize costs on this host), FleetVecNormalize.step.
    python tools/vecnorm_rate.py [--steps 300] [--configs c3,c5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8.0e12


def torch_ops_norm(torch, st, x, r, done, term, gamma=0.99, eps=1e-8, clip=10.0):
    """VecNormalize's step in plain torch ops (float64 statistics); `st` holds mean, var, count, rmean, rvar, rcount, returns."""
    E = x.shape[0]
    xd = x.double()
    bm, bv = xd.mean(0), xd.var(0, unbiased=False)
    d = bm - st["mean"]
    tot = st["count"] + E
    st["mean"] = st["mean"] + d * E / tot
    st["var"] = (st["var"] * st["count"] + bv * E + d * d * st["count"] * E / tot) / tot
    st["count"] = tot
    sd = torch.sqrt(st["var"] + eps)
    out = ((xd - st["mean"]) / sd).clamp(-clip, clip).float()
    rf = r.float().double()
    st["returns"] = st["returns"] * gamma + rf
    rbm, rbv = st["returns"].mean(), st["returns"].var(unbiased=False)
    rd = rbm - st["rmean"]
    rtot = st["rcount"] + E
    st["rmean"] = st["rmean"] + rd * E / rtot
    st["rvar"] = (st["rvar"] * st["rcount"] + rbv * E + rd * rd * st["rcount"] * E / rtot) / rtot
    st["rcount"] = rtot
    rn = (rf / torch.sqrt(st["rvar"] + eps)).clamp(-clip, clip)
    db = done.bool()
    tn = torch.where(db[:, None], ((term.double() - st["mean"]) / sd).clamp(-clip, clip).float(), term)
    st["returns"] = torch.where(db, torch.zeros_like(st["returns"]), st["returns"])
    return out, rn, tn


def device_config(torch, name, steps):
    from bench import CONFIGS, Group
    from fleetrl_amd.distributed import shard_range
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    spec = CONFIGS[name]
    dev = torch.device("cuda", 0)
    E, N = spec["envs"], spec["evs"]
    groups, off = [], 0
    for k, uc in enumerate(spec["groups"]):
        lo, hi = shard_range(E, len(spec["groups"]), k)
        groups.append(Group(torch, dev, uc, hi - lo, N, spec, 0, off, 16, 1 + k))
        off += hi - lo
    for g in groups:
        g.batch.use_torch_stream(dev)
        g.norm = DeviceNormalizer(g.E, g.batch.obs_dim)
        g.norm.use_torch_stream(dev)
        g.term = torch.zeros_like(g.obs)
        g.nobs, g.nrew, g.nterm = torch.empty_like(g.obs), torch.empty_like(g.reward), torch.empty_like(g.obs)
        g.st = {"mean": torch.zeros(g.batch.obs_dim, device=dev, dtype=torch.float64),
                "var": torch.ones(g.batch.obs_dim, device=dev, dtype=torch.float64), "count": 1e-4,
                "rmean": torch.zeros((), device=dev, dtype=torch.float64), "rvar": torch.ones((), device=dev, dtype=torch.float64),
                "rcount": 1e-4, "returns": torch.zeros(g.E, device=dev, dtype=torch.float64)}
        g.batch.reset_dev(g.obs.data_ptr())

    def one(i, mode):
        for g in groups:
            g.batch.step_dev(g.tape[i % g.L].data_ptr(), g.obs.data_ptr(), g.reward.data_ptr(), g.done.data_ptr(), g.term.data_ptr())
            if mode == "norm":
                g.norm.step_dev(g.obs.data_ptr(), g.reward.data_ptr(), g.done.data_ptr(), g.term.data_ptr(), g.nobs.data_ptr(),
                                g.nrew.data_ptr(), g.nterm.data_ptr())
            elif mode == "torch":
                torch_ops_norm(torch, g.st, g.obs, g.reward, g.done, g.term)

    def norm_only(i, _):
        for g in groups:
            g.norm.step_dev(g.obs.data_ptr(), g.reward.data_ptr(), g.done.data_ptr(), g.term.data_ptr(), g.nobs.data_ptr(),
                            g.nrew.data_ptr(), g.nterm.data_ptr())

    def timed(fn, mode, reps=3):
        for i in range(20):
            fn(i, mode)
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(steps):
                fn(i, mode)
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / steps)
        return float(np.median(out)), [round(v, 2) for v in out]

    res = {}
    for mode in ("plain", "norm", "torch", "plain"):  # plain twice: the spread of the baseline itself
        key = {"plain": "step_us", "norm": "step_norm_us", "torch": "step_torch_ops_us"}[mode]
        med, all_ = timed(one, mode)
        res.setdefault(key, med)
        res.setdefault(key + "_runs", []).extend(all_)
    res["step_us"] = float(np.median(res["step_us_runs"]))
    med, all_ = timed(norm_only, None)
    # obs read twice and written once; the terminal rows of the last step's done envs read and written once
    nbytes = sum(g.E * g.batch.obs_dim * 4 * 3 + int(g.done.sum().item()) * g.batch.obs_dim * 8 for g in groups)
    res.update(norm_us=med, norm_us_runs=all_, norm_algorithmic_bytes=nbytes, norm_roof_us=nbytes / HBM_PEAK * 1e6,
               norm_roof_frac=nbytes / HBM_PEAK / (med * 1e-6), norm_added_us=res["step_norm_us"] - res["step_us"],
               torch_ops_added_us=res["step_torch_ops_us"] - res["step_us"],
               speedup_vs_torch_ops=(res["step_torch_ops_us"] - res["step_us"]) / max(res["step_norm_us"] - res["step_us"], 1e-9),
               envs=E, evs=N, obs_dims=[g.batch.obs_dim for g in groups])
    for g in groups:
        g.norm.close()
        g.batch.close()
    return res


def host_path(steps):
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables
    from vecnorm_model import VecNormModel

    E, N = 4096, 50
    env = FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N))
    rng = np.random.default_rng(0)
    acts = rng.uniform(-1, 1, size=(8, E, N)).astype(np.float32)

    def run(step):
        for i in range(20):
            step(acts[i % 8])
        t0 = time.perf_counter()
        for i in range(steps):
            step(acts[i % 8])
        return (time.perf_counter() - t0) / steps * 1e6

    res = {}
    env.reset()
    res["host_step_us"] = run(env.step)
    model = VecNormModel(E, env.core.obs_dim)
    model.reset(env.reset())

    def with_model(a):
        o, r, d, info = env.step(a)
        term = np.zeros_like(o)
        for i in np.flatnonzero(d):
            term[i] = info[i]["terminal_observation"]
        return model.step(o, r, d, term)

    res["host_step_numpy_vecnormalize_us"] = run(with_model)
    vn = FleetVecNormalize(env)
    vn.reset()
    res["host_step_fleet_vecnormalize_us"] = run(vn.step)
    res["host_step_again_us"] = run(env.step)
    res["host_norm_ratio"] = res["host_step_fleet_vecnormalize_us"] / min(res["host_step_us"], res["host_step_again_us"])
    vn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--configs", default="c3,c5")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"steps": args.steps}
    for name in args.configs.split(","):
        out[name] = device_config(torch, name, args.steps)
    if not args.no_host:
        out["c3_host"] = host_path(args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
