#!/usr/bin/env python3
"""The loop of examples/ppo_device_collect.py with SB3's EvalCallback as ONE call as well: an iteration is `DevicePPOCollect.collect`,
`DevicePPOTrain.train` and, every `--eval-every` iterations, `DeviceEvalCallback.evaluate` -- three enqueue-only calls and nothing in
between that waits for the device.

`evaluate` enqueues what the reference's training pipeline has EvalCallback do: the training env's normalisation statistics to the
validation env (`sync_envs_normalization`), `--eval-episodes` deterministic episodes there (`evaluate_policy`), their mean and std, and
the copy of the agent's weights into the handle's snapshot when the mean beats the best so far -- decided on the device.  `results()`
is where the host looks.  It shows that the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/ppo_device_eval.py [--iterations 4] [--eval-every 2] [--envs 256] [--eval-envs 8] [--evs 5] [--steps 64]

Prints one JSON line per iteration and one per evaluation.  `--time` measures the evaluation alone instead: `sync_normalization` +
`evaluate_policy` (arm A) against the one call (arm B), alternated `--repeats` times, in milliseconds per evaluation.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import (DeviceAdam, DeviceEvalCallback, DevicePolicy, DevicePPOCollect, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer,  # noqa: E402
                         FleetVecEnv, FleetVecNormalize, evaluate_policy, sync_normalization)
from fleetrl_amd.synth import synth_tables  # noqa: E402
from fleetrl_amd.train import SB3_NAMES  # noqa: E402
from ppo_device_collect import ActorCritic, rollout_names  # noqa: E402


def time_arms(args, train_env, eval_env, pol, callback):
    """Arm A (the existing pieces) and arm B (the one call), alternated; a window is one evaluation from its first enqueue to the end
    of the synchronisation behind it, after a warm-up evaluation of the same arm."""

    def arm_a():
        sync_normalization(train_env, eval_env)
        evaluate_policy(pol, eval_env, n_eval_episodes=args.eval_episodes)

    def arm_b():
        callback.evaluate(0)

    per_eval = {"A": [], "B": []}
    for _ in range(args.repeats):
        for name, arm in (("A", arm_a), ("B", arm_b)):
            arm()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm()
            torch.cuda.synchronize()
            per_eval[name].append((time.perf_counter() - t0) * 1e3)
    out = {"what": "one evaluation, milliseconds", "eval_envs": args.eval_envs, "evs": args.evs, "eval_episodes": args.eval_episodes,
           "env_steps": callback.n_steps()}
    for name, xs in per_eval.items():
        xs = sorted(xs)
        out[name] = {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": per_eval[name]}
    out["B_over_A"] = out["B"]["median"] / out["A"]["median"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--eval-every", type=int, default=2, help="iterations between evaluations (SB3's eval_freq, in rollouts)")
    ap.add_argument("--eval-episodes", type=int, default=5)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--eval-envs", type=int, default=8)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--episode-hours", type=int, default=None, help="episode length in hours (default: the benchmark's 48)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time one evaluation: the existing pieces against the one call")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    E, N, K = args.envs, args.evs, args.steps
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    def make(num_envs, seed):
        cfg = bench_config(num_envs, N, "ct")
        if args.episode_hours is not None:
            cfg = dict(cfg, episode_length=args.episode_hours)
        return FleetVecNormalize(FleetVecEnv(cfg, num_envs, tables=synth_tables("ct", N), seed=seed), clip_reward=10.0)

    env, eval_env = make(E, args.seed), make(args.eval_envs, args.seed + 1)  # (the reference validates on another table; here: other starts)
    D = env.norm.D
    net = ActorCritic(D, N).to(dev)
    params = net.linear_parameters()
    layers = lambda ps: [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]  # noqa: E731
    pol = DevicePolicy(layers(params[:6]), critic_layers=layers(params[6:]), activation="tanh", output="clip")
    # monitor=True: make_vec_env wraps the reference's envs in Monitor, so SB3's evaluation reports the raw episode returns
    callback = DeviceEvalCallback(pol, eval_env, n_eval_episodes=args.eval_episodes, monitor=True, train_normalizer=env)
    if args.time:
        time_arms(args, env, eval_env, pol, callback)
        for h in (callback, pol, eval_env, env):
            h.close()
        return
    buf = DeviceRolloutBuffer(E, K, D, N, gamma=0.99, gae_lambda=0.95)
    collector = DevicePPOCollect(env, pol)
    grad = DevicePPOGrad(pol, min(args.batch_size, E * K))
    into = params + [net.log_std]
    opt = DeviceAdam(pol, into, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    trainer = DevicePPOTrain(buf, grad, opt)
    steps = epochs = n_updates = 0

    collector.reset()
    for it in range(args.iterations):
        # the iteration: collect, train and every so often evaluate, all enqueue only
        rollout = collector.collect(buf, net.log_std, seed=args.seed, first_step=steps)
        stats = trainer.train(into, n_epochs=args.epochs, batch_size=args.batch_size, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, lr=3e-4,
                              normalize_advantage=True, seed=args.seed, first_epoch=epochs)
        steps += K
        epochs += args.epochs
        evaluated = (it + 1) % args.eval_every == 0
        if evaluated:
            callback.evaluate(steps * E)
        collector.check_errors()
        st = dict(zip(SB3_NAMES, stats.tolist()))
        n_updates += int(st["train/n_updates"])
        st["train/n_updates"] = n_updates
        print(json.dumps({"iteration": it, "time/total_timesteps": steps * E, **rollout_names(rollout), **st}), flush=True)
        if evaluated:  # (the host looks here; a loop that only wants the best agent at the end never has to)
            print(json.dumps(callback.results()), flush=True)
    callback.load_best_into(pol)  # the agent EvalCallback would have saved as best_model
    callback.check_errors()
    for h in (callback, collector, trainer, opt, grad, pol, buf, eval_env, env):
        h.close()


if __name__ == "__main__":
    main()
