#!/usr/bin/env python3
"""The loop of examples/td3_device_train.py with the env steps as ONE call too: an iteration is `DeviceTD3Collect.collect` for
`--train-freq` env steps, `DeviceTD3Train.train` for as many gradient steps, and the refresh of the acting policy from the stepped
parameters -- enqueue-only calls, and nothing else.

`collect` enqueues SB3's off-policy `collect_rollouts`: per env step the exploration launch (uniform actions before
`--learning-starts`, then the actor plus white noise, or plus `--noise pink` / `ou` from a device process restarted per env by the
done flags), the env's step, the normaliser's step, the replay buffer's add of the RAW transition and one launch that keeps the last 100
finished episodes (SB3's `ep_info_buffer`) on the device; one closing launch writes the statistics block printed under SB3's
`rollout/*` names.  The observations between calls are the collect handle's.  It shows that the pieces fit -- it is not a tuned
trainer.  Needs an MI355X; inputs are synthetic:

    python examples/td3_device_collect.py [--iterations 50] [--envs 256] [--evs 5] [--train-freq 4] [--learning-starts 20]
                                          [--batch-size 256] [--buffer-size 100000] [--noise white|pink|ou] [--log-interval 10]

Prints one JSON line per logging interval.  `--time` measures the collection alone instead: the step-by-step loop of
examples/td3_pink_noise.py (arm A) against the one call (arm B), alternated `--repeats` times, in microseconds per env step.
"""
import argparse
import json
import os
import sys
import time

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import (DeviceAdam, DeviceOUNoise, DevicePinkNoise, DevicePolicy, DeviceReplayBuffer, DeviceTD3Collect, DeviceTD3Grad,  # noqa: E402
                         DeviceTD3Target, DeviceTD3Train, FleetVecEnv, FleetVecNormalize)
from fleetrl_amd.collect import SB3_NAMES as ROLLOUT_NAMES, STATS as ROLLOUT_STATS  # noqa: E402
from fleetrl_amd.offpolicy import STATS  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


def mlp(inp, out, hidden=64, last=None):
    layers = [nn.Linear(inp, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, out)]
    return nn.Sequential(*layers, *([last] if last else []))


class Critics(nn.Module):
    """TD3's twin Q networks."""

    def __init__(self, obs_dim, act_dim):
        super().__init__()
        self.q1, self.q2 = mlp(obs_dim + act_dim, 1), mlp(obs_dim + act_dim, 1)


def linear_layers(net):
    """[(W, b), ...] of a Sequential's linear layers: the shapes DeviceTD3Target and DevicePolicy are made from."""
    return [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]


def rollout_names(stats):
    """The collect call's statistics under SB3's names (and `rollout/<name>` for those SB3 has no key for)."""
    return {sb3 or "rollout/" + name: v for name, sb3, v in zip(ROLLOUT_STATS, ROLLOUT_NAMES, stats.tolist())}


def step_by_step(env, pol, buf, noise, args, first, n_steps, obs, done, last_raw, act, reward, terminal):
    """The env steps of examples/td3_pink_noise.py: exploration, step, add and a copy per env step."""
    for s in range(first, first + n_steps):
        if s < args.learning_starts:
            pol.sample_uniform(args.envs, seed=args.seed, step=s, actions_out=act, env_actions_out=act)
        elif noise is not None:
            pol.explore(obs, args.noise_sd, action_noise=noise, done=done, actions_out=act, env_actions_out=act)
        else:
            pol.explore(obs, args.noise_sd, seed=args.seed, step=s, actions_out=act, env_actions_out=act)
        env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
        raw = env.original_torch()
        buf.add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
        last_raw.copy_(raw.obs)


def time_arms(args, env, pol, buf, noise, collector):
    """Arm A (the loop above) and arm B (the one call), alternated; a window is `--rollouts` calls of `--train-freq` steps behind a
    warm-up one and ends in a device synchronise.  Every timed step lies behind learning_starts: the actor runs."""
    E, K, dev = args.envs, args.train_freq, torch.device("cuda", 0)
    D, N = pol.obs_dim, pol.act_dim
    obs, done, last_raw = torch.empty((E, D), device=dev), torch.zeros(E, device=dev, dtype=torch.uint8), torch.empty((E, D), device=dev)
    act, reward, terminal = torch.empty((E, N), device=dev), torch.empty(E, device=dev, dtype=torch.float64), torch.empty((E, D), device=dev)
    stats = torch.empty(16, device=dev, dtype=torch.float64)
    steps = args.learning_starts

    def arm_a(n):
        nonlocal steps
        for _ in range(n):
            step_by_step(env, pol, buf, noise, args, steps, K, obs, done, last_raw, act, reward, terminal)
            steps += K

    def arm_b(n):
        nonlocal steps
        for _ in range(n):
            collector.collect(buf, K, learning_starts=args.learning_starts, sigma=args.noise_sd, noise=noise, seed=args.seed, first_step=steps,
                              stats_out=stats)
            steps += K

    per_step = {"A": [], "B": []}
    with torch.no_grad():
        for _ in range(args.repeats):
            for name, arm in (("A", arm_a), ("B", arm_b)):
                if name == "A":
                    env.reset_torch(obs_out=obs)
                    last_raw.copy_(env.original_torch().obs)
                    done.zero_()
                else:
                    collector.reset()
                    collector.carry_start.zero_()
                arm(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arm(args.rollouts)
                torch.cuda.synchronize()
                per_step[name].append((time.perf_counter() - t0) * 1e6 / (args.rollouts * K))
    out = {"what": "td3 collection, microseconds per env step", "envs": E, "evs": N, "steps": K, "noise": args.noise, "rollouts_per_window": args.rollouts}
    for name, xs in per_step.items():
        xs = sorted(xs)
        out[name] = {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": per_step[name]}
    out["B_over_A"] = out["B"]["median"] / out["A"]["median"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--train-freq", type=int, default=4, help="env steps per collect call, and gradient steps per train call")
    ap.add_argument("--buffer-size", type=int, default=100_000)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--learning-starts", type=int, default=20)
    ap.add_argument("--noise", choices=("white", "pink", "ou"), default="white")
    ap.add_argument("--noise-sd", type=float, default=0.1)
    ap.add_argument("--log-interval", type=int, default=10)
    ap.add_argument("--episode-hours", type=int, default=None, help="episode length in hours (default: the benchmark's 48)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time the collection: the step-by-step loop against the one call")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=20, help="collect calls per timed window")
    args = ap.parse_args()
    E, N, K = args.envs, args.evs, args.train_freq
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    cfg = bench_config(E, N, "ct")
    if args.episode_hours is not None:
        cfg = dict(cfg, episode_length=args.episode_hours)
    env = FleetVecNormalize(FleetVecEnv(cfg, E, tables=synth_tables("ct", N), seed=args.seed), clip_reward=10.0)
    D = env.norm.D
    actor, critics = mlp(D, N, last=nn.Tanh()).to(dev), Critics(D, N).to(dev)
    actor_params, critic_params = list(actor.parameters()), [*critics.q1.parameters(), *critics.q2.parameters()]
    pol = DevicePolicy(linear_layers(actor), activation="relu", output="tanh")  # the acting policy: refreshed after every update
    buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
    episode_steps = int(env.venv.core.params.episode_steps)
    noise = {"white": lambda: None, "pink": lambda: DevicePinkNoise(E, N, episode_steps, seed=args.seed),
             "ou": lambda: DeviceOUNoise(E, N, sigma=1.0, seed=args.seed)}[args.noise]()
    collector = DeviceTD3Collect(env, pol)  # stats_window = 100, SB3's
    if args.time:
        time_arms(args, env, pol, buf, noise, collector)
        for h in (collector, noise, pol, buf, env):
            if h is not None:
                h.close()
        return
    make = lambda: DeviceTD3Target(linear_layers(actor), [linear_layers(critics.q1), linear_layers(critics.q2)], activation="relu", output="tanh")  # noqa: E731
    targets, nets = make(), make()  # the targets start as copies of the online networks
    grad = DeviceTD3Grad(nets, args.batch_size)
    opt_a, opt_c = DeviceAdam(nets, actor_params, nets="actor", lr=1e-3), DeviceAdam(nets, critic_params, nets="critic", lr=1e-3)
    update = DeviceTD3Train(buf, targets, grad, opt_a, opt_c, max_steps=K)
    sigma = torch.full((N,), 0.2, device=dev)  # the target-policy smoothing noise's scale
    train_stats = torch.zeros(16, device=dev, dtype=torch.float64)
    actor_loss = torch.zeros((), device=dev, dtype=torch.float64)  # of the last call that took an actor step (others report NaN)
    steps = updates = 0

    collector.reset()
    collector.carry_start.zero_()  # (SB3's off-policy loop has no episode_start: the noise processes start with their handles)
    for it in range(1, args.iterations + 1):
        # the iteration: enqueue-only calls
        rollout = collector.collect(buf, K, learning_starts=args.learning_starts, sigma=args.noise_sd, noise=noise, seed=args.seed, first_step=steps)
        steps += K
        if steps >= args.learning_starts:
            update.train(actor_params, critic_params, gradient_steps=K, batch_size=args.batch_size, gamma=0.99, tau=0.005, policy_delay=2, sigma=sigma,
                         noise_clip=0.5, lr=1e-3, seed=args.seed + 0x7A46E7, first_update=updates, env=env, stats_out=train_stats)
            updates += K
            pol.load_torch(actor_params)  # the next rollout acts with the stepped actor
            actor_loss = torch.where(torch.isnan(train_stats[3]), actor_loss, train_stats[3])
        if it % args.log_interval == 0 or it == args.iterations:
            collector.check_errors()
            # the only transfers: the statistics blocks
            log = {"iteration": it, "time/total_timesteps": steps * E, "transitions": buf.size() * E, **rollout_names(rollout)}
            if updates:
                log.update({"train/critic_loss": train_stats[STATS.index("critic_loss")].item(), "train/actor_loss": actor_loss.item(),
                            "train/n_updates": int(train_stats[STATS.index("n_updates")].item())})
            print(json.dumps(log), flush=True)
    for h in (collector, update, opt_a, opt_c, grad, nets, targets, noise, pol, buf, env):
        if h is not None:
            h.close()


if __name__ == "__main__":
    main()
