#!/usr/bin/env python3
"""The TD3 loop of examples/td3_device_grad.py with the optimisers on the device as well: two `DeviceAdam` handles stand on the
ONLINE image (a second `DeviceTD3Target` beside the targets'), one over the actor and one over the critics.  Per gradient step:
`critic_grad` (two launches) writes the critics' gradients into the `.grad` of torch's own parameters and the critic optimiser's
`step` (one launch: SB3's TD3 does not clip, so no norm is formed) applies torch's Adam update, writing every new weight both to the
torch parameter and to the online image; on every `policy_delay`-th step the same for the actor.  No `load_torch` follows a step,
and torch does nothing in a gradient step any more.  Deterministic from the minibatch to the weights.  For the first critic step
torch's own Adam runs on a copy, and the largest difference between the stepped parameters is printed.  Measured (DESIGN.md section
7o, profiles/adam_rate.json).

Per env step: the actor reads the normalised observations, Gaussian noise from torch.randn explores, the env and the normaliser
step on the device, and `add` stores the RAW transition in one launch.  Per gradient step: `sample` draws and gathers the minibatch
in one launch, `target` computes the bootstrap target in one launch.  No tensor crosses to the host inside the loop.  It shows that the
pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/td3_device_adam.py [--steps 200] [--envs 256] [--evs 5] [--buffer-size 100000] [--batch-size 256]
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
from fleetrl_amd import DeviceAdam, DeviceReplayBuffer, DeviceTD3Grad, DeviceTD3Target, FleetVecEnv, FleetVecNormalize  # noqa: E402
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
    # the targets start as copies of the online networks; `online` is what polyak() reads: W, b per layer, actor, q1, q2
    targets = DeviceTD3Target(linear_layers(actor), [linear_layers(critics.q1), linear_layers(critics.q2)], activation="relu", output="tanh")
    online = [*actor.parameters(), *critics.q1.parameters(), *critics.q2.parameters()]
    # the networks that are differentiated: a second image, refreshed from `online` after every optimiser step
    nets = DeviceTD3Target(linear_layers(actor), [linear_layers(critics.q1), linear_layers(critics.q2)], activation="relu", output="tanh")
    grad = DeviceTD3Grad(nets, args.batch_size)
    actor_params, critic_params = list(actor.parameters()), [*critics.q1.parameters(), *critics.q2.parameters()]
    critic_stats, actor_stats = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    sigma = torch.full((N,), 0.2, device=dev)  # the target-policy smoothing noise's scale
    # the optimisers on the ONLINE image: a step writes the new weights to torch's parameters and to `nets` (SB3's TD3 does not clip)
    opt_a, opt_c = DeviceAdam(nets, actor_params, nets="actor", lr=1e-3), DeviceAdam(nets, critic_params, nets="critic", lr=1e-3)
    checked = False
    buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
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
            for _ in range(args.gradient_steps):
                b = buf.sample(args.batch_size, env=env)  # normalised with the statistics as they are now
                # one launch; a seed of its own (the exploration above draws from torch's generator), the update count as the step
                target_q = targets.target(b.next_observations, b.rewards, b.dones, gamma=gamma, sigma=sigma, noise_clip=noise_clip,
                                          seed=args.seed + 0x7A46E7, step=updates)
                # both MSE losses and their backward: two launches into the critics' .grad (overwritten: nothing to zero)
                grad.critic_grad(b, target_q, into=critic_params, stats_out=critic_stats)
                if not checked:  # once: torch's own Adam on a copy of the critics' parameters, from the same gradients
                    copy = [nn.Parameter(p.detach().clone()) for p in critic_params]
                    for c, p in zip(copy, critic_params):
                        c.grad = p.grad.clone()
                    torch.optim.Adam(copy, lr=1e-3).step()
                opt_c.step()  # one launch (two with clipping): Adam, and the image's new weights
                if not checked:
                    checked = True
                    print(json.dumps({"max_abs_param_diff_to_torch_adam": max(float((p.detach() - c.detach()).abs().max()) for p, c in zip(critic_params, copy))}),
                          flush=True)
                updates += 1
                if updates % policy_delay == 0:
                    # -mean(Q_0(obs, actor(obs))) and its backward into the actor: two launches
                    grad.actor_grad(b.observations, into=actor_params, stats_out=actor_stats)
                    opt_a.step()
                    targets.polyak(online, tau)  # one launch for the actor and both critics

        if step % args.log_interval == 0 or step == args.steps:
            buf.check_errors()
            # the only transfers: a few numbers for the log
            print(json.dumps({"step": step, "transitions": buf.size() * E, "updates": updates, "critic_loss": critic_stats[0].item(),
                              "actor_loss": actor_stats[0].item(), "mean_raw_reward": (reward_sum / step).item()}), flush=True)
    opt_a.close()
    opt_c.close()
    grad.close()
    nets.close()
    targets.close()
    buf.close()
    env.close()


if __name__ == "__main__":
    main()
