"""Host wall time of SAC's collect and evaluate as ONE call each against the Python loops they replace, on one
MI355X; prints one JSON line and writes profiles/sac_collect_rate.json with --write.

  collect   `DeviceSACCollect.collect` of 64 env steps past the warm-up against the loop of examples/sac_device_train.py --
            `DeviceSACNetworks.act`, `FleetVecNormalize.step_torch`, `original_torch`, `DeviceReplayBuffer.add` per step -- at 256 envs x
            5 EVs and at 4096 x 50, with 64-64 and 256-256 trunks; microseconds per env step
  evaluate  `DeviceEvalCallback.evaluate` of 5 episodes of 192 steps on 5 envs against `evaluate_policy` driven through an adapter whose
            `act` is the networks' deterministic action; milliseconds per evaluation
Both arms of a pair run in one process, each on an env of its own, alternated --reps times after a warm-up; a window is timed on the
host from its first enqueue to the end of its final synchronise.

    python tools/sac_collect_rate.py [--reps 7] [--write]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, SEED = 64, 0xAC7


def summary(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "all": [float(x) for x in xs]}


def make_env(E, N, seed, hours=None):
    from bench import bench_config
    from fleetrl_amd import FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    cfg = bench_config(E, N, "ct") if hours is None else dict(bench_config(E, N, "ct"), episode_length=hours)
    return FleetVecNormalize(FleetVecEnv(cfg, E, tables=synth_tables("ct", N), seed=seed), clip_reward=10.0)


def make_nets(torch, D, N, hidden):
    from fleetrl_amd import DeviceSACNetworks

    gen = torch.Generator().manual_seed(D + N + hidden)

    def chain(*dims):
        return [(torch.randn((o, i), generator=gen) / i ** 0.5, torch.zeros(o)) for i, o in zip(dims[:-1], dims[1:])]

    return DeviceSACNetworks(chain(D, hidden, hidden, 2 * N), [chain(D + N, hidden, hidden, 1) for _ in range(2)], activation="relu")


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure_collect(torch, E, N, hidden, reps, rollouts):
    from fleetrl_amd import DeviceReplayBuffer, DeviceSACCollect

    dev = torch.device("cuda", 0)
    envs = [make_env(E, N, 5) for _ in range(2)]
    D = envs[0].norm.D
    nets = make_nets(torch, D, N, hidden)
    bufs = [DeviceReplayBuffer(STEPS * E, E, D, N, seed=1) for _ in range(2)]
    col = DeviceSACCollect(envs[1], nets, stats_window=100)
    obs, last_raw, terminal = (torch.empty((E, D), device=dev) for _ in range(3))
    act, reward, done = torch.empty((E, N), device=dev), torch.empty(E, device=dev, dtype=torch.float64), torch.empty(E, device=dev, dtype=torch.uint8)
    stats = torch.zeros(16, device=dev, dtype=torch.float64)
    envs[0].reset_torch(obs_out=obs)
    last_raw.copy_(envs[0].original_torch().obs)
    col.reset()
    step = [0, 0]

    def loop():  # the parent's path: examples/sac_device_train.py
        for _ in range(rollouts * STEPS):
            nets.act(obs, seed=SEED, step=step[0], actions_out=act)
            envs[0].step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
            raw = envs[0].original_torch()
            bufs[0].add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
            last_raw.copy_(raw.obs)
            step[0] += 1

    def call():
        for _ in range(rollouts):
            col.collect(bufs[1], STEPS, learning_starts=0, seed=SEED, first_step=step[1], stats_out=stats)
            step[1] += STEPS

    loop(), call()  # warm-up; both arms took the same steps from the same state
    torch.cuda.synchronize()
    same = bool(torch.equal(bufs[0].actions.view(torch.int32), bufs[1].actions.view(torch.int32)) and
                torch.equal(col.carry_obs.view(torch.int32), obs.view(torch.int32)))
    a, b = [], []
    for _ in range(reps):
        a.append(timed(torch, loop) * 1e6 / (rollouts * STEPS))
        b.append(timed(torch, call) * 1e6 / (rollouts * STEPS))
    launches = col.describe()["launches"]
    for h in (col, nets, *bufs, *envs):
        h.close()
    return {"what": "sac collection, microseconds per env step", "envs": E, "evs": N, "obs_dim": D, "trunk": [hidden, hidden], "steps": STEPS,
            "rollouts_per_window": rollouts, "arms_bit_equal_after_warm_up": same, "launches_per_call": launches, "A_python_loop": summary(a),
            "B_one_call": summary(b), "B_over_A": float(np.median(b) / np.median(a))}


class Deterministic:
    def __init__(self, nets):
        self.nets, self.obs_dim, self.act_dim = nets, nets.obs_dim, nets.act_dim

    def act(self, obs, out):
        return self.nets.act(obs, deterministic=True, actions_out=out)


def measure_eval(torch, N, hidden, reps, E=5, n_eval=5):
    from fleetrl_amd import DeviceEvalCallback, evaluate_policy

    envs = [make_env(E, N, 7, hours=48) for _ in range(2)]
    D = envs[0].norm.D
    nets = make_nets(torch, D, N, hidden)
    cb = DeviceEvalCallback(nets, envs[1], n_eval_episodes=n_eval, monitor=False)
    adapter = Deterministic(nets)
    out = {}

    def loop():
        out["A"] = evaluate_policy(adapter, envs[0], n_eval_episodes=n_eval, return_episode_rewards=True)

    def call():
        cb.evaluate(0)

    loop(), call()
    rewards, lengths = cb.episodes()
    same = bool(np.array_equal(np.array(out["A"][0], np.float64).view(np.int64), rewards.view(np.int64)))
    a, b = [], []
    for _ in range(reps):
        a.append(timed(torch, loop) * 1e3)
        b.append(timed(torch, call) * 1e3)
    res = {"what": "sac evaluation, milliseconds per evaluation", "envs": E, "evs": N, "obs_dim": D, "trunk": [hidden, hidden], "episodes": n_eval,
           "steps": cb.n_steps(), "episode_lengths": [int(x) for x in lengths], "lists_bit_equal_after_warm_up": same,
           "launches_per_call": cb.describe()["launches"], "A_evaluate_policy": summary(a), "B_one_call": summary(b),
           "B_over_A": float(np.median(b) / np.median(a))}
    for h in (cb, nets, *envs):
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    res = {"what": "tools/sac_collect_rate.py on one MI355X, one process: arm A the Python loop, arm B the one call, alternated; host wall time "
                   "from the first enqueue to the end of the final synchronise", "device": torch.cuda.get_device_name(0), "reps": args.reps, "runs": []}
    for E, N, rollouts in ((256, 5, 10), (4096, 50, 4)):
        for hidden in (64, 256):
            res["runs"].append(measure_collect(torch, E, N, hidden, args.reps, rollouts))
            print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    for N in (5, 50):
        for hidden in (64, 256):
            res["runs"].append(measure_eval(torch, N, hidden, args.reps))
            print(json.dumps(res["runs"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(res))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sac_collect_rate.json"), "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
