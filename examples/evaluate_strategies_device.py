#!/usr/bin/env python3
"""The last stage of the reference's workflow (agent_eval/basic_evaluation.py) for a whole batch of fleets: a trained agent and the
benchmark strategies each run the same episodes on an env of their own, and every env's data log is reduced to the evaluation's
numbers on the device (`evaluate_strategies` -> `summarize_log`, two launches per log; nothing but a few kilobytes per env comes
back).  `compare` then prints the reference's table and the time-of-day charging power, for one env or averaged over all.

    python examples/evaluate_strategies_device.py [--envs 256] [--hours 24] [--normalize STATS.npz] [--env mean]

The agent is the reference's example agent (tests/golden/ppo_lmd_arbitrage_policy.npz: an MlpPolicy 45 -> 64 -> 64 -> 1 for one
last-mile-delivery vehicle with building load and PV).  STATS.npz is a normaliser state written by `FleetVecNormalize.save`; without
it the agent sees raw observations, which is not what it was trained on: the table then shows that the pieces fit, not how good
the agent is.  Inputs are synthetic.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import DevicePolicy, compare, evaluate_strategies  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--hours", type=int, default=24, help="episode length; every strategy runs one episode")
    ap.add_argument("--normalize", help="normaliser state written by FleetVecNormalize.save")
    ap.add_argument("--env", default="mean", help="the env whose table is printed, or 'mean'")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    E, N = args.envs, 1
    with np.load(os.path.join(ROOT, "tests", "golden", "ppo_lmd_arbitrage_policy.npz")) as z:
        policy = DevicePolicy.from_state_dict({k: z[k] for k in z.files})
    cfg = dict(bench_config(E, N, "lmd"), episode_length=args.hours)
    steps = args.hours * 4 - 1  # the step that ends an episode is not logged (fleet_environment.py:679)
    out = evaluate_strategies(cfg, ("uncontrolled", "distributed", "night", "lp", policy), E, steps, normalizer=args.normalize,
                              tables=synth_tables("lmd", N), seed=args.seed)
    env = args.env if args.env == "mean" else int(args.env)
    for name in ("uncontrolled", "distributed", "night", "lp"):
        res = compare(out["policy"], out[name], env=env)
        print(f"\n== the agent against {name} charging, env {env}: {int(out[name].rows[0])} log rows per env ==")
        for row, (rl, bench) in res["table"].items():
            print(f"{row:28s} {rl:14.5f} {bench:14.5f}")
        peak = np.nanargmax(res["power"]["benchmark charging"])
        print(f"{'peak mean power [kW] at':28s} {'%02d:%02d' % divmod(int(peak) * 15, 60):>14s} {res['power']['benchmark charging'][peak]:14.3f}")
    h = out["policy"].hist.sum(axis=0)
    print("\nthe agent's actions (50 bins over [-1, 1], all envs):", " ".join(str(int(x)) for x in h))
    policy.close()


if __name__ == "__main__":
    main()
