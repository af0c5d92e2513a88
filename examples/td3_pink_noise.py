#!/usr/bin/env python3
"""The loop of examples/td3_device_explore.py with the reference's TD3 recipe for the action noise: pink noise over sequences as long
as an episode (`PinkActionNoise(noise_scale, seq_len=episode steps, n_actions)` there, `DevicePinkNoise` here), generated on the
device per env and restarted by the env's own done flags.

Per env step: before `--learning-starts` the actions are uniform (`sample_uniform`, SB3's warm-up); afterwards `explore` runs the
actor on the normalised observations, takes the next row of the pink process (`action_noise=`; the done flags of the step before
give the envs whose episode ended a new sequence, as SB3's VectorizedActionNoise.reset does) and clips the sum to the action space:
two launches, nothing crosses to the host.  The step on which every env starts a new sequence is the slow one (DESIGN.md
"Correlated action noise on the device").  `load_torch` refreshes the device actor after every actor update.  The env and the
normaliser step on the device, and `add` stores the RAW transition (`FleetVecNormalize.original_torch()`: SB3's off-policy loop keeps the
original observations and rewards) in one launch.  Per gradient step: `sample` draws the minibatch's indices on the device, gathers
the rows and normalises them with the statistics of that moment -- one launch.  No tensor crosses to the host inside the loop.
It shows that the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/td3_pink_noise.py [--steps 200] [--envs 256] [--evs 5] [--buffer-size 100000] [--batch-size 256]
                                   [--learning-starts 20] [--gradient-steps 1] [--log-interval 50]

Prints one JSON line per logging interval.
"""
import argparse
import copy
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import DevicePinkNoise, DevicePolicy, DeviceReplayBuffer, FleetVecEnv, FleetVecNormalize  # noqa: E402
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


def polyak(net, target, tau):
    with torch.no_grad():
        for p, q in zip(net.parameters(), target.parameters()):
            q.lerp_(p, tau)


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
    episode_steps = int(env.venv.core.params.episode_steps)  # episode hours x steps per hour: 192
    D = env.norm.D
    actor, critics = mlp(D, N, last=nn.Tanh()).to(dev), Critics(D, N).to(dev)
    actor_t, critics_t = copy.deepcopy(actor).requires_grad_(False), copy.deepcopy(critics).requires_grad_(False)
    opt_a, opt_c = torch.optim.Adam(actor.parameters(), lr=1e-3), torch.optim.Adam(critics.parameters(), lr=1e-3)
    buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
    gamma, tau, policy_delay, noise_sd, target_noise, noise_clip = 0.99, 0.005, 2, 0.1, 0.2, 0.5
    actor_params = [p for m in actor if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
    pol = DevicePolicy([(actor_params[i], actor_params[i + 1]) for i in range(0, 6, 2)], activation="relu", output="tanh")
    pink = DevicePinkNoise(E, N, episode_steps, seed=args.seed)  # one sequence per env, column and episode
    act = torch.empty((E, N), device=dev)

    # the step's outputs, written in place every step; the raw observations of the step before are kept for `add`
    obs, reward, done = torch.empty((E, D), device=dev), torch.empty(E, device=dev, dtype=torch.float64), torch.empty(E, device=dev, dtype=torch.uint8)
    done.zero_()
    terminal = torch.empty((E, D), device=dev)
    last_raw = torch.empty((E, D), device=dev)
    env.reset_torch(obs_out=obs)
    last_raw.copy_(env.original_torch().obs)
    updates = 0
    q_loss = a_loss = torch.zeros((), device=dev)
    reward_sum = torch.zeros((), device=dev, dtype=torch.float64)

    for step in range(1, args.steps + 1):
        with torch.no_grad():
            if step < args.learning_starts:
                pol.sample_uniform(E, seed=args.seed, step=step, actions_out=act, env_actions_out=act)
            else:  # clip(actor(obs) + noise_sd * pink, -1, 1); `done` still holds the flags of the step before
                pol.explore(obs, noise_sd, action_noise=pink, done=done, actions_out=act, env_actions_out=act)
            env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
            raw = env.original_torch()  # the raw observations, float64 rewards and terminal rows, where the step left them
            buf.add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
            last_raw.copy_(raw.obs)
            reward_sum += raw.reward.mean()

        if step >= args.learning_starts:
            for _ in range(args.gradient_steps):
                b = buf.sample(args.batch_size, env=env)  # normalised with the statistics as they are now
                with torch.no_grad():
                    noise = (target_noise * torch.randn_like(b.actions)).clamp(-noise_clip, noise_clip)
                    next_act = (actor_t(b.next_observations) + noise).clamp(-1, 1)
                    target_q = b.rewards + (1 - b.dones) * gamma * torch.min(*critics_t(b.next_observations, next_act))
                q1, q2 = critics(b.observations, b.actions)
                q_loss = nn.functional.mse_loss(q1, target_q) + nn.functional.mse_loss(q2, target_q)
                opt_c.zero_grad(set_to_none=True)
                q_loss.backward()
                opt_c.step()
                updates += 1
                if updates % policy_delay == 0:
                    a_loss = -critics.q1(torch.cat([b.observations, actor(b.observations)], dim=1)).mean()
                    opt_a.zero_grad(set_to_none=True)
                    a_loss.backward()
                    opt_a.step()
                    pol.load_torch(actor_params)
                    polyak(actor, actor_t, tau)
                    polyak(critics, critics_t, tau)

        if step % args.log_interval == 0 or step == args.steps:
            buf.check_errors()
            # the only transfers: a few numbers for the log
            print(json.dumps({"step": step, "transitions": buf.size() * E, "updates": updates, "critic_loss": q_loss.item(),
                              "actor_loss": a_loss.item(), "mean_raw_reward": (reward_sum / step).item()}), flush=True)
    pink.close()
    pol.close()
    buf.close()
    env.close()


if __name__ == "__main__":
    main()
