#!/usr/bin/env python3
"""A short SAC loop with the forward side of a gradient step in the library (`DeviceSACNetworks`): `act` draws
the squashed-Gaussian action in ONE launch, `target` computes the entropy-regularised bootstrap target of the minibatch in ONE launch
(the online actor on next_obs, its log-probability, both target critics, the min, r + (1 - d) * gamma * (q - alpha * log pi)), the
critics' gradients come from the existing `DeviceTD3Grad.critic_grad` launches, `DeviceAdam` steps them and `polyak` blends the
targets.  What torch still does in a gradient step: the actor loss and the entropy-coefficient loss with their backward passes and
optimiser steps, after which `load_torch` refreshes the online image.

SB3's SAC critic loss is 0.5 * sum_c mse(q_c, y); the TD3 launches compute sum_c mse(q_c, y).  `fleetrl_amd.sac.critic_update` halves
the gradients before the optimiser step and the loop reports half of the launches' loss, so the update is SB3's
(tests/test_update_ref_gpu.py holds it to SB3's loop under torch autograd).

Measured: with these 64-64 trunks at a batch of 256 the target launch takes 40 us against 361 us of the
eager-torch restatement below (`--time`).

Warm-up actions are uniform (`DevicePolicy.sample_uniform`, SB3's `action_space.sample()` before `learning_starts`).  It shows that
the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/sac_device_targets.py [--steps 200] [--envs 256] [--evs 5] [--batch 256] [--learning-starts 8] [--time]

Prints one JSON line per logging interval; `--time` then alternates the one-call target with an eager-torch float32 restatement and
prints the medians and ranges of both.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import (DeviceAdam, DevicePolicy, DeviceReplayBuffer, DeviceSACNetworks, DeviceTD3Grad, FleetVecEnv,  # noqa: E402
                         FleetVecNormalize)
from fleetrl_amd.sac import CRITIC_LOSS_SCALE, critic_update  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


def mlp(inp, out, hidden):
    return nn.Sequential(nn.Linear(inp, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, out))


def linear_layers(net):
    return [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]


def squashed(actor, obs, eps, A):
    """The actor in torch, for the losses that need its gradient: (action, log-probability), the header's expressions."""
    out = actor(obs)
    mean, log_std = out[:, :A], out[:, A:].clamp(-20.0, 2.0)
    a = torch.tanh(mean + log_std.exp() * eps)
    lp = (-0.5 * eps * eps - log_std - 0.9189385332).sum(1) - torch.log(1.0 - a * a + 1e-6).sum(1)
    return a, lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--buffer-size", type=int, default=100_000)
    ap.add_argument("--learning-starts", type=int, default=8)
    ap.add_argument("--log-interval", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    E, N, B = args.envs, args.evs, args.batch
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    env = FleetVecNormalize(FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=args.seed), clip_reward=10.0)
    D = env.norm.D
    # the actor's last layer is [2N, hidden]: the mu rows, then the log_std rows
    actor, q1, q2 = mlp(D, 2 * N, args.hidden).to(dev), mlp(D + N, 1, args.hidden).to(dev), mlp(D + N, 1, args.hidden).to(dev)
    shapes = (linear_layers(actor), [linear_layers(q1), linear_layers(q2)])
    nets, targets = DeviceSACNetworks(*shapes, activation="relu"), DeviceSACNetworks(*shapes, activation="relu")
    actor_params, critic_params = list(actor.parameters()), [*q1.parameters(), *q2.parameters()]
    online = actor_params + critic_params  # W, b per layer: the actor, q1, q2 -- what load_torch and polyak read
    grad = DeviceTD3Grad(nets, B)
    opt_c = DeviceAdam(nets, critic_params, nets="critic", lr=3e-4)
    opt_a = torch.optim.Adam(actor_params, lr=3e-4)
    log_alpha = torch.zeros(1, device=dev, requires_grad=True)
    opt_alpha = torch.optim.Adam([log_alpha], lr=3e-4)
    alpha = torch.ones(1, device=dev)  # exp(log_alpha), kept on the device: the target launch reads it when it runs
    target_entropy = -float(N)
    warmup = DevicePolicy([(torch.zeros((N, D)), torch.zeros(N))])  # sample_uniform runs no network
    buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
    gamma, tau = 0.99, 0.005
    act_seed, target_seed = args.seed + 0xAC7, args.seed + 0x7A26E7  # the target draws under a seed of its own

    obs, reward, done = torch.empty((E, D), device=dev), torch.empty(E, device=dev, dtype=torch.float64), torch.empty(E, device=dev, dtype=torch.uint8)
    terminal, last_raw, act = torch.empty((E, D), device=dev), torch.empty((E, D), device=dev), torch.empty((E, N), device=dev)
    env.reset_torch(obs_out=obs)
    last_raw.copy_(env.original_torch().obs)
    critic_stats = torch.zeros(8, device=dev)
    a_loss = torch.zeros((), device=dev)
    reward_sum = torch.zeros((), device=dev, dtype=torch.float64)
    updates = 0

    for step in range(1, args.steps + 1):
        with torch.no_grad():
            if step <= args.learning_starts:
                warmup.sample_uniform(E, seed=act_seed, step=step, actions_out=act, env_actions_out=act)
            else:
                nets.act(obs, seed=act_seed, step=step, actions_out=act)  # one launch; the same action for the env and the buffer
            env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
            raw = env.original_torch()
            buf.add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
            last_raw.copy_(raw.obs)
            reward_sum += raw.reward.mean()

        if step > args.learning_starts:
            b = buf.sample(B, env=env)
            # the entropy coefficient (SB3: before the critic update, on the actor's current log-probability)
            eps = torch.randn((B, N), device=dev)
            pi, log_pi = squashed(actor, b.observations, eps, N)
            alpha_loss = -(log_alpha * (log_pi.detach() + target_entropy)).mean()
            opt_alpha.zero_grad(set_to_none=True)
            alpha_loss.backward()
            opt_alpha.step()
            with torch.no_grad():
                alpha.copy_(log_alpha.exp())
            # the critics: target (one launch), gradients (two launches), Adam on the image and the parameters (one launch)
            # (SB3's 0.5 * (mse + mse) is the helper's loss_scale: see the module's docstring)
            critic_update(nets, targets, grad, opt_c, b, critic_params, gamma=gamma, ent_coef=alpha, seed=target_seed, step=updates,
                          stats_out=critic_stats)
            # the actor (torch): alpha * log pi - min_c Q_c(s, pi(s)); the critics' parameters are the ones the device just stepped
            x = torch.cat([b.observations, pi], dim=1)
            a_loss = (alpha.detach() * log_pi - torch.min(q1(x), q2(x)).view(-1)).mean()
            opt_a.zero_grad(set_to_none=True)
            a_loss.backward()
            opt_a.step()
            nets.load_torch(online)  # the actor's new weights into the online image (one launch)
            targets.polyak(online, tau)  # one launch; the targets' copy of the actor follows too, and nothing reads it
            updates += 1

        if step % args.log_interval == 0 or step == args.steps:
            buf.check_errors()
            print(json.dumps({"step": step, "transitions": buf.size() * E, "gradient_steps": updates,
                              "critic_loss": CRITIC_LOSS_SCALE * critic_stats[0].item(), "actor_loss": a_loss.item(), "ent_coef": alpha.item(),
                              "mean_raw_reward": (reward_sum / step).item()}), flush=True)

    if args.time:
        b = buf.sample(B, env=env)
        tq1, tq2 = copy.deepcopy(q1), copy.deepcopy(q2)
        y = torch.empty(B, device=dev)

        def one_call():
            nets.target(targets, b.next_observations, b.rewards, b.dones, gamma=gamma, ent_coef=alpha, seed=target_seed, step=0, out=y)

        def eager():
            with torch.no_grad():
                eps = torch.randn((B, N), device=dev)
                a, lp = squashed(actor, b.next_observations, eps, N)
                x = torch.cat([b.next_observations, a], dim=1)
                q = torch.min(tq1(x), tq2(x)).view(-1) - alpha * lp
                return b.rewards.view(-1) + (1.0 - b.dones.view(-1)) * gamma * q

        times = {"one_call": [], "eager_torch": []}
        for rep in range(22):  # arms alternated; the first two rounds warm up
            for name, fn in (("one_call", one_call), ("eager_torch", eager)):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(20):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[name].append(t0.elapsed_time(t1) / 20 * 1e3)
        print(json.dumps({"target_us": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
                          "batch": B, "hidden": args.hidden, "obs_dim": D, "act_dim": N}), flush=True)

    for h in (opt_c, grad, targets, nets, warmup, buf, env):
        h.close()


if __name__ == "__main__":
    main()
