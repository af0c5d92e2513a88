"""One linear-optimisation plan (`fleet_lp_plan_dev`, fleetrl_amd/csrc/fleet_lp.hip) of bench.py's c3 workload: 4096 envs x 50
caretaker EVs with building load, PV and rainflow degradation on the bench's synthetic tables, 192 rows from each env's first
reset.  Prints one JSON line: wall time per plan (first call with the scratch allocation, then the mean of `--reps` calls, each
synchronised), whether every output is finite, the status-bit counts.  `--dump DIR --dump-envs 0,17,4095` writes the plan of those
envs and the state it was made from (`time_idx`, `soc`) to DIR/lp_plan_dump.npz (tests/test_lp_plan_gpu.py holds them against
the model).  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/lp_plan_bench.py` for the kernel time (profiles/lp_plan_4096x50x192/)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--evs", type=int, default=50)
    ap.add_argument("--horizon", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dump", default=None, help="directory for lp_plan_dump.npz")
    ap.add_argument("--dump-envs", default="0", help="comma-separated env indices to dump")
    args = ap.parse_args()
    import numpy as np
    import torch

    from bench import bench_config
    from fleetrl_amd import _capi
    from fleetrl_amd.batch import FleetBatch
    from fleetrl_amd.config import resolve_config
    from fleetrl_amd.lp_benchmark import _plan_dev
    from fleetrl_amd.params import make_params, time_features
    from fleetrl_amd.synth import synth_tables

    E, N, H = args.envs, args.evs, args.horizon
    rc = resolve_config(bench_config(E, N, "ct", True, True, "rainflow"))
    tables = synth_tables("ct", N, seed=1234, include_building=True, include_pv=True, price_year="2020", feed_in="spot")
    batch = FleetBatch(make_params(rc, tables, E, auto_reset=True, seed=0), tables, time_features(tables), device=0)
    batch.reset()
    state = (batch.get("time_idx"), batch.get("soc"))  # what the plans below are made from (planning does not change it)
    t = time.perf_counter()
    out = _plan_dev(batch, H, _capi.ACT_F64)
    torch.cuda.synchronize()
    first = time.perf_counter() - t
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter()
        out2 = _plan_dev(batch, H, _capi.ACT_F64)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    act, soc, bound, cost, status = (x.cpu().numpy() for x in out2)
    same = all(torch.equal(a, b) for a, b in zip(out, out2))
    st = status.reshape(-1)
    if args.dump:
        envs = np.array(sorted(int(x) for x in args.dump_envs.split(",")), dtype=np.int64)
        os.makedirs(args.dump, exist_ok=True)
        np.savez(os.path.join(args.dump, "lp_plan_dump.npz"), envs=envs, time_idx=state[0][envs], soc=state[1][envs],
                 actions=act[:, envs], soc_plan=soc[:, envs], bound=bound[envs], plan_cost=cost[envs], status=status[envs])
    print(json.dumps({"envs": E, "evs": N, "horizon": H, "first_call_s": round(first, 4), "wall_s_per_plan": round(float(np.mean(ts)), 4),
                      "reps": args.reps, "finite": bool(all(np.isfinite(x).all() for x in (act, soc, bound, cost))),
                      "bit_identical": bool(same), "gap_mean_eur": float(np.mean(cost - bound)), "bound_mean_eur": float(np.mean(bound)),
                      "status_counts": {str(b): int(((st & b) != 0).sum()) for b in (1, 2, 4, 8)}}))


if __name__ == "__main__":
    main()
