#!/usr/bin/env python3
"""The loop of examples/ppo_device_train.py with the rollout as ONE call too: an iteration is `DevicePPOCollect.collect` and
`DevicePPOTrain.train`, two enqueue-only calls, and nothing else.

`collect` enqueues SB3's `collect_rollouts` -- per env step the exploration launch, the env's step, the normaliser's step, the buffer's
add and one launch that keeps the last 100 finished episodes (SB3's `ep_info_buffer`) on the device; then the bootstrap values, the GAE
and one closing launch -- and returns one block of statistics on the device, printed under SB3's `rollout/*` names beside `train/*`.
The observation a rollout ends on is the collect handle's: the next call starts from it.  It shows that the pieces fit -- it is not a
tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/ppo_device_collect.py [--iterations 3] [--envs 256] [--evs 5] [--steps 64] [--batch-size 128] [--epochs 4]

Prints one JSON line per iteration.  `--time` measures the rollout alone instead: the step-by-step loop of
examples/ppo_device_train.py (arm A) against the one call (arm B), alternated `--repeats` times, in microseconds per env step.
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
from fleetrl_amd import (DeviceAdam, DevicePolicy, DevicePPOCollect, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer, FleetVecEnv,  # noqa: E402
                         FleetVecNormalize)
from fleetrl_amd.collect import SB3_NAMES as ROLLOUT_NAMES, STATS as ROLLOUT_STATS  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402
from fleetrl_amd.train import SB3_NAMES  # noqa: E402


class ActorCritic(nn.Module):
    """SB3's MlpPolicy in small: separate tanh MLPs for the Gaussian mean and the value, a state-independent log std."""

    def __init__(self, obs_dim, act_dim, hidden=64):
        super().__init__()
        mlp = lambda out: nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(), nn.Linear(hidden, out))  # noqa: E731
        self.pi, self.vf = mlp(act_dim), mlp(1)
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    def linear_parameters(self):
        """W, b per layer, the actor's then the critic's: the order DevicePolicy.load_torch takes."""
        return [p for net in (self.pi, self.vf) for m in net if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]


def rollout_names(stats):
    """The collect call's statistics under SB3's names (and `rollout/<name>` for those SB3 has no key for)."""
    return {sb3 or "rollout/" + name: v for name, sb3, v in zip(ROLLOUT_STATS, ROLLOUT_NAMES, stats.tolist())}


def step_by_step(env, pol, buf, log_std, seed, steps, carry_obs, carry_start, env_act, last_value, reward):
    """The rollout of examples/ppo_device_train.py: four calls per env step, then the bootstrap value and the GAE."""
    K = buf.n_steps
    buf.reset()
    obs, start = carry_obs, carry_start
    for t in range(K):
        row = buf.slot(t)
        pol.sample(obs, log_std, seed=seed, step=steps + t, actions_out=row.actions, env_actions_out=env_act, log_prob_out=row.log_prob,
                   values_out=row.value)
        nxt = buf.slot(t + 1) if t + 1 < K else None
        nobs, ndone = (nxt.obs, nxt.episode_start) if nxt else (carry_obs, carry_start)
        if nobs is obs:  # (K = 1: the carry buffers are still being read)
            obs, start = obs.clone(), start.clone()
        env.step_torch(env_act, obs_out=nobs, reward_out=reward, done_out=ndone)
        buf.add(obs, row.actions, reward, start, row.value, row.log_prob)
        obs, start = nobs, ndone
    pol.act(obs, out=env_act, values_out=last_value)
    buf.compute_returns_and_advantage(last_value, start)


def time_arms(args, env, pol, buf, collector, log_std):
    """Arm A (the loop above) and arm B (the one call), alternated; a window is `--rollouts` rollouts behind a warm-up one and ends in
    a device synchronise.  Both arms step the same env on, so they see the same mix of episode ends."""
    E, K, dev = args.envs, args.steps, torch.device("cuda", 0)
    D, N = pol.obs_dim, pol.act_dim
    carry_obs, carry_start = torch.empty((E, D), device=dev), torch.ones(E, device=dev, dtype=torch.uint8)
    env_act, last_value, reward = torch.empty((E, N), device=dev), torch.empty((E, 1), device=dev), torch.empty(E, device=dev, dtype=torch.float64)
    stats = torch.empty(16, device=dev, dtype=torch.float64)
    steps = 0

    def arm_a(n):
        nonlocal steps
        for _ in range(n):
            step_by_step(env, pol, buf, log_std, args.seed, steps, carry_obs, carry_start, env_act, last_value, reward)
            steps += K

    def arm_b(n):
        nonlocal steps
        for _ in range(n):
            collector.collect(buf, log_std, seed=args.seed, first_step=steps, stats_out=stats)
            steps += K

    per_step = {"A": [], "B": []}
    with torch.no_grad():
        for _ in range(args.repeats):
            for name, arm in (("A", arm_a), ("B", arm_b)):
                # each arm continues from where the env stands: its own carry from a reset of its own
                if name == "A":
                    env.reset_torch(obs_out=carry_obs) if hasattr(env, "reset_torch") else env.core.batch.reset_dev(carry_obs.data_ptr())
                    carry_start.fill_(1)
                else:
                    collector.reset()
                arm(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                arm(args.rollouts)
                torch.cuda.synchronize()
                per_step[name].append((time.perf_counter() - t0) * 1e6 / (args.rollouts * K))
    out = {"what": "ppo rollout, microseconds per env step", "envs": E, "evs": N, "steps": K, "rollouts_per_window": args.rollouts}
    for name, xs in per_step.items():
        xs = sorted(xs)
        out[name] = {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "all": per_step[name]}
    out["B_over_A"] = out["B"]["median"] / out["A"]["median"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--episode-hours", type=int, default=None, help="episode length in hours (default: the benchmark's 48)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time", action="store_true", help="time the rollout: the step-by-step loop against the one call")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rollouts", type=int, default=20, help="rollouts per timed window")
    args = ap.parse_args()
    E, N, K = args.envs, args.evs, args.steps
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    cfg = bench_config(E, N, "ct")
    if args.episode_hours is not None:
        cfg = dict(cfg, episode_length=args.episode_hours)
    env = FleetVecNormalize(FleetVecEnv(cfg, E, tables=synth_tables("ct", N), seed=args.seed), clip_reward=10.0)
    D = env.norm.D
    net = ActorCritic(D, N).to(dev)
    buf = DeviceRolloutBuffer(E, K, D, N, gamma=0.99, gae_lambda=0.95)
    params = net.linear_parameters()
    layers = lambda ps: [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]  # noqa: E731
    pol = DevicePolicy(layers(params[:6]), critic_layers=layers(params[6:]), activation="tanh", output="clip")
    collector = DevicePPOCollect(env, pol)  # stats_window = 100, SB3's
    if args.time:
        time_arms(args, env, pol, buf, collector, net.log_std.detach())
        for h in (collector, pol, buf, env):
            h.close()
        return
    grad = DevicePPOGrad(pol, min(args.batch_size, E * K))
    into = params + [net.log_std]  # load_torch's order, then log_std
    opt = DeviceAdam(pol, into, lr=3e-4, eps=1e-5, max_grad_norm=0.5)  # SB3's PPO: Adam with eps 1e-5, gradients clipped at 0.5
    trainer = DevicePPOTrain(buf, grad, opt)
    steps = 0   # the noise's step counter: never repeats over the run
    epochs = 0  # the shuffle's epoch counter: never repeats over the run either
    n_updates = 0

    collector.reset()
    for it in range(args.iterations):
        # the iteration: two calls, both enqueue only
        rollout = collector.collect(buf, net.log_std, seed=args.seed, first_step=steps)
        stats = trainer.train(into, n_epochs=args.epochs, batch_size=args.batch_size, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, lr=3e-4,
                              normalize_advantage=True, seed=args.seed, first_epoch=epochs)
        steps += K
        epochs += args.epochs
        collector.check_errors()
        # the only transfers of the iteration: the two statistics blocks
        st = dict(zip(SB3_NAMES, stats.tolist()))
        n_updates += int(st["train/n_updates"])
        st["train/n_updates"] = n_updates
        print(json.dumps({"iteration": it, "time/total_timesteps": steps * E, **rollout_names(rollout), **st}), flush=True)
    for h in (collector, trainer, opt, grad, pol, buf, env):
        h.close()


if __name__ == "__main__":
    main()
