"""Time of the evaluation's numbers from the data log, on the device (`summarize_log`: fleet_log_summary_dev, two launches over the
ring) against the host route (`get_log()` and the reference's pandas sums per env); prints one JSON line and writes it to --out
(default profiles/log_summary_rate.json).

Shape: 4096 envs x 50 EVs, the ring of the default capacity (two episodes and their reset rows) filled once over by the uncontrolled
strategy.  Device arm: HIP events on torch's stream around --inner back-to-back enqueue-only calls (`as_torch=True`), and a host clock
around the whole call that ends with the arrays in NumPy (the launches, the copies of a few kilobytes per env, the synchronise);
medians of --reps rounds after warm-up.  Host arm: a host clock around `get_log()` plus, per env, the sums, the violation count, the
time-of-day means and the histogram of agent_eval/basic_evaluation.py; it copies the whole ring and builds a DataFrame per env in a
Python loop, so it runs at --host-envs envs (default 64) and the JSON states that count and the time per env of both arms.

    python tools/log_summary_rate.py [--envs 4096] [--evs 50] [--host-envs 64] [--reps 9] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def filled_env(E, N, tables):
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv
    from fleetrl_amd.policies import run_policy

    venv = FleetVecEnv(dict(bench_config(E, N, "ct"), log_data=True), E, tables=tables, seed=0)
    venv.reset()
    cap = venv.core.batch.log_capacity()
    run_policy(venv.core.batch, "uncontrolled", cap, chunk=96)  # cap + 1 rows written: every slot holds a row
    return venv, cap


def host_route(venv):
    """What a user does today: the DataFrames, then the reference's arithmetic on each."""
    out = []
    for lg in venv.env_method("get_log"):
        socv = lg["SOC violation"]
        hid = lg["Time"].dt.hour + lg["Time"].dt.minute / 60
        energy = np.stack(lg["Charging energy"].values).mean(axis=1)
        out.append((lg["Reward"].sum(), lg["Cashflow"].sum(), lg["Degradation"].sum(), lg["Grid overloading"].sum(), socv.sum(),
                    socv[socv > 0].size, lg["SOH"].iloc[-1], lg.assign(e=energy).groupby(hid)["e"].mean().values * 4,
                    np.histogram(np.stack(lg["Action"].values)[:, 0], bins=50, range=(-1, 1))[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--evs", type=int, default=50)
    ap.add_argument("--host-envs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "log_summary_rate.json"))
    args = ap.parse_args()
    import warnings

    import torch

    from fleetrl_amd import summarize_log
    from fleetrl_amd.synth import synth_tables

    E, N = args.envs, args.evs
    tables = synth_tables("ct", N)
    venv, cap = filled_env(E, N, tables)
    for _ in range(3):  # warm-up: code objects, the handle's scratch
        summarize_log(venv)
    torch.cuda.synchronize()
    enq, whole = [], []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            s = summarize_log(venv, as_torch=True)
        b.record()
        b.synchronize()
        enq.append(a.elapsed_time(b) * 1e3 / args.inner)
        t0 = time.perf_counter()
        s = summarize_log(venv)
        whole.append((time.perf_counter() - t0) * 1e6)
    rows = int(s.rows[0])
    ring_bytes = rows * E * (4 + 32 + 16 * N)  # row word, env scalars, action and energy per EV: what the reduction must read
    venv.close()

    hE = min(args.host_envs, E)
    hvenv, _ = filled_env(hE, N, tables)
    host = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # get_log says that the ring has wrapped: it has, by design of this run
        host_route(hvenv)
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            host_route(hvenv)
            host.append((time.perf_counter() - t0) * 1e6)
    hvenv.close()

    dev_us, dev_whole_us, host_us = float(np.median(enq)), float(np.median(whole)), float(np.median(host))
    out = {"device": torch.cuda.get_device_name(0), "envs": E, "evs": N, "log_capacity": cap, "window_rows": rows, "reps": args.reps,
           "inner": args.inner,
           "device_launches_us": dev_us, "device_launches_runs_us": [round(x, 1) for x in enq],
           "device_to_numpy_us": dev_whole_us, "device_to_numpy_runs_us": [round(x, 1) for x in whole],
           "ring_bytes_read": ring_bytes, "device_launches_gb_per_s": ring_bytes / dev_us / 1e3,
           "host_envs": hE, "host_route_us": host_us, "host_route_runs_us": [round(x, 1) for x in host],
           "device_to_numpy_us_per_env": dev_whole_us / E, "host_route_us_per_env": host_us / hE,
           "host_over_device_per_env": (host_us / hE) / (dev_whole_us / E),
           "note": "the host route ran at host_envs envs, not at envs: its time per env is what compares"}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
