#!/usr/bin/env python3
"""The TD3 loop of examples/td3_device_adam.py with its inner `for` replaced by ONE call: `DeviceTD3Train.train` enqueues the
`gradient_steps` gradient steps of an env step -- per step `sample`, `target`, `critic_grad`, the critic optimiser's step and, on
every `policy_delay`-th update, `actor_grad`, the actor optimiser's step and the Polyak update, which here reads the ONLINE weight
image instead of walking torch's tensors -- and one closing launch that writes what SB3 logs as `train/*`.  The `policy_delay`
bookkeeping is the library's: the loop passes the number of gradient steps taken so far.  The weights are bit-equal to the loop of
td3_device_adam.py from the same state.  Measured (profiles/td3_train_rate.json).

Per env step: the actor reads the normalised observations, Gaussian noise from torch.randn explores, the env and the normaliser
step on the device, and `add` stores the RAW transition in one launch.  No tensor crosses to the host inside the loop.  It shows that
the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/td3_device_train.py [--steps 200] [--envs 256] [--evs 5] [--buffer-size 100000] [--batch-size 256]
                                        [--learning-starts 20] [--gradient-steps 1] [--log-interval 50]

Prints one JSON line per logging interval.
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import DeviceAdam, DeviceReplayBuffer, DeviceTD3Grad, DeviceTD3Target, DeviceTD3Train, FleetVecEnv, FleetVecNormalize  # noqa: E402
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

    def forward(self, obs, act):
        x = torch.cat([obs, act], dim=1)
        return self.q1(x), self.q2(x)


def linear_layers(net):
    """[(W, b), ...] of a Sequential's linear layers: the shapes DeviceTD3Target is made from."""
    return [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--buffer-size", type=int, default=100_000)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--learning-starts", type=int, default=20)
    ap.add_argument("--gradient-steps", type=int, default=1)
    ap.add_argument("--log-interval", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    E, N = args.envs, args.evs
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    env = FleetVecNormalize(FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=args.seed), clip_reward=10.0)
    D = env.norm.D
    actor, critics = mlp(D, N, last=nn.Tanh()).to(dev), Critics(D, N).to(dev)
    # the targets start as copies of the online networks
    targets = DeviceTD3Target(linear_layers(actor), [linear_layers(critics.q1), linear_layers(critics.q2)], activation="relu", output="tanh")
    # the networks that are differentiated: a second image, which the optimisers keep equal to torch's parameters
    nets = DeviceTD3Target(linear_layers(actor), [linear_layers(critics.q1), linear_layers(critics.q2)], activation="relu", output="tanh")
    grad = DeviceTD3Grad(nets, args.batch_size)
    actor_params, critic_params = list(actor.parameters()), [*critics.q1.parameters(), *critics.q2.parameters()]
    sigma = torch.full((N,), 0.2, device=dev)  # the target-policy smoothing noise's scale
    # the optimisers on the ONLINE image: a step writes the new weights to torch's parameters and to `nets` (SB3's TD3 does not clip)
    opt_a, opt_c = DeviceAdam(nets, actor_params, nets="actor", lr=1e-3), DeviceAdam(nets, critic_params, nets="critic", lr=1e-3)
    buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
    # the whole update: borrows the five handles above
    update = DeviceTD3Train(buf, targets, grad, opt_a, opt_c, max_steps=max(args.gradient_steps, 1))
    stats = torch.zeros(16, device=dev, dtype=torch.float64)
    actor_loss = torch.zeros((), device=dev, dtype=torch.float64)  # of the last call that took an actor step (others report NaN)
    gamma, tau, policy_delay, noise_sd, noise_clip = 0.99, 0.005, 2, 0.1, 0.5

    # the step's outputs, written in place every step; the raw observations of the step before are kept for `add`
    obs, reward, done = torch.empty((E, D), device=dev), torch.empty(E, device=dev, dtype=torch.float64), torch.empty(E, device=dev, dtype=torch.uint8)
    terminal = torch.empty((E, D), device=dev)
    last_raw = torch.empty((E, D), device=dev)
    env.reset_torch(obs_out=obs)
    last_raw.copy_(env.original_torch().obs)
    updates = 0
    reward_sum = torch.zeros((), device=dev, dtype=torch.float64)

    for step in range(1, args.steps + 1):
        with torch.no_grad():
            act = (actor(obs) + noise_sd * torch.randn((E, N), device=dev)).clamp(-1, 1)
            env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
            raw = env.original_torch()  # the raw observations, float64 rewards and terminal rows, where the step left them
            buf.add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
            last_raw.copy_(raw.obs)
            reward_sum += raw.reward.mean()

        if step >= args.learning_starts:
            # every gradient step of this env step, enqueued by one call; normalised with the statistics as they are now; a seed of its
            # own (the exploration above draws from torch's generator); `updates` is SB3's _n_updates
            update.train(actor_params, critic_params, gradient_steps=args.gradient_steps, batch_size=args.batch_size, gamma=gamma, tau=tau,
                         policy_delay=policy_delay, sigma=sigma, noise_clip=noise_clip, lr=1e-3, seed=args.seed + 0x7A46E7,
                         first_update=updates, env=env, stats_out=stats)
            updates += args.gradient_steps
            actor_loss = torch.where(torch.isnan(stats[3]), actor_loss, stats[3])

        if step % args.log_interval == 0 or step == args.steps:
            buf.check_errors()
            # the only transfers: a few numbers for the log
            log = {"step": step, "transitions": buf.size() * E, "mean_raw_reward": (reward_sum / step).item()}
            if updates:
                log.update({"train/critic_loss": stats[STATS.index("critic_loss")].item(), "train/actor_loss": actor_loss.item(),
                            "train/n_updates": int(stats[STATS.index("n_updates")].item())})
            print(json.dumps(log), flush=True)
    update.close()
    opt_a.close()
    opt_c.close()
    grad.close()
    nets.close()
    targets.close()
    buf.close()
    env.close()


if __name__ == "__main__":
    main()
