"""Wall time of one evaluation of the training agent -- SB3's EvalCallback: 5 deterministic episodes of 192 steps on a validation env
with a normaliser, tanh trunks 64-64 -- at 256 envs x 5 EVs and 4096 envs x 50 EVs; prints one JSON line and writes it to
profiles/eval_rate.json with --write.

Two arms on ONE evaluation env, policy and training normaliser, alternating --reps times in one process; host wall time from the first
enqueue to the end of the final synchronisation, after one untimed evaluation of each arm; medians with min .. max reported:
  pieces    `sync_normalization(train, eval)` then `evaluate_policy(policy, eval, 5)`: the host copies the statistics through get_state /
            set_state, runs the Python loop of about ten torch launches per env step and reads the block's dones and sums back
  one_call  `DeviceEvalCallback.evaluate`: fleet_eval_run_dev, enqueue only; then `torch.cuda.synchronize()`
Both arms take the same env steps (one block of episode_steps steps: 5 episodes < num_envs), so the device work differs only by the
bookkeeping.  `enqueue_ms` is the one call's host time before the synchronisation: what a training loop pays when it does not wait.

    python tools/eval_rate.py [--reps 5] [--write]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((256, 5), (4096, 50))
EPISODES, HIDDEN = 5, (64, 64)


def measure(torch, E, N, reps):
    from bench import bench_config

    from fleetrl_amd import DeviceEvalCallback, DeviceNormalizer, DevicePolicy, FleetVecEnv, FleetVecNormalize, evaluate_policy, sync_normalization
    from fleetrl_amd.synth import synth_tables

    dev = torch.device("cuda", 0)
    env = FleetVecNormalize(FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=1), clip_reward=10.0)
    D = env.norm.D
    rng = np.random.default_rng(0)
    sizes = (D, *HIDDEN, N)
    layers = [(rng.uniform(-1, 1, (o, i)).astype(np.float32) / np.sqrt(i), np.zeros(o, np.float32)) for i, o in zip(sizes[:-1], sizes[1:])]
    pol = DevicePolicy(layers, activation="tanh", output="clip")
    train = DeviceNormalizer(E, D)  # the training env's normaliser: statistics of three batches
    train.use_torch_stream()
    for _ in range(3):
        train.step_torch(torch.randn((E, D), device=dev), torch.randn(E, device=dev, dtype=torch.float64), torch.zeros(E, device=dev, dtype=torch.uint8))

    class TrainStats:  # what sync_normalization reads of a VecNormalize
        obs_rms = property(lambda self: train.get_state().obs_rms)
        ret_rms = property(lambda self: train.get_state().ret_rms)

    cb = DeviceEvalCallback(pol, env, n_eval_episodes=EPISODES, monitor=False, train_normalizer=train)
    enqueue = []

    def pieces():
        sync_normalization(TrainStats(), env)
        evaluate_policy(pol, env, n_eval_episodes=EPISODES)

    def one_call():
        t0 = time.perf_counter()
        cb.evaluate(0)
        enqueue.append((time.perf_counter() - t0) * 1e3)

    times = {"pieces": [], "one_call": []}
    for name, arm in (("pieces", pieces), ("one_call", one_call)):  # untimed: allocations, code objects
        arm()
        torch.cuda.synchronize()
    enqueue.clear()
    for _ in range(reps):
        for name, arm in (("pieces", pieces), ("one_call", one_call)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    cb.check_errors()
    out = {"envs": E, "evs": N, "obs_dim": D, "env_steps": cb.n_steps(), "launches_one_call": cb.describe()["launches"]}
    for name, xs in (*times.items(), ("enqueue", enqueue)):
        s = sorted(xs)
        out[name + "_ms"] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "all": xs}
    out["one_call_over_pieces"] = out["one_call_ms"]["median"] / out["pieces_ms"]["median"]
    for h in (cb, train, pol, env):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"what": "one evaluation (5 episodes, tanh 64-64, with a normaliser), host wall milliseconds, first enqueue to end of synchronisation",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "shapes": [measure(torch, E, N, args.reps) for E, N in SHAPES]}
    print(json.dumps(out), flush=True)
    if args.write:
        with open(os.path.join(ROOT, "profiles", "eval_rate.json"), "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
