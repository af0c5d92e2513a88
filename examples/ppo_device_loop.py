#!/usr/bin/env python3
"""A complete PPO iteration loop that never leaves the GPU: FleetVecEnv + FleetVecNormalize + a small torch actor-critic +
DeviceRolloutBuffer.

Per rollout step: the policy reads the observations where the last step wrote them -- row t of the buffer --, the env and the
normaliser write the next observations and dones into row t + 1, and `add` stores actions, reward, value and log-probability in one
launch.  No tensor crosses to the host inside the rollout; the advantages are one launch; the clipped-surrogate update runs over
`get(batch_size)`.  It shows that the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/ppo_device_loop.py [--iterations 3] [--envs 256] [--evs 5] [--steps 64] [--batch-size 1024] [--epochs 2]

Prints one JSON line per iteration.
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import DeviceRolloutBuffer, FleetVecEnv, FleetVecNormalize  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


class ActorCritic(nn.Module):
    """SB3's MlpPolicy in small: separate tanh MLPs for the Gaussian mean and the value, a state-independent log std."""

    def __init__(self, obs_dim, act_dim, hidden=64):
        super().__init__()
        mlp = lambda out: nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(), nn.Linear(hidden, out))  # noqa: E731
        self.pi, self.vf = mlp(act_dim), mlp(1)
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    def dist(self, obs):
        return torch.distributions.Normal(self.pi(obs), self.log_std.exp())

    def evaluate(self, obs, actions):
        d = self.dist(obs)
        return self.vf(obs).squeeze(-1), d.log_prob(actions).sum(-1), d.entropy().sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    E, N, K = args.envs, args.evs, args.steps
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    env = FleetVecNormalize(FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=args.seed), clip_reward=10.0)
    D = env.norm.D
    net = ActorCritic(D, N).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4)
    buf = DeviceRolloutBuffer(E, K, D, N, gamma=0.99, gae_lambda=0.95)
    clip_range, vf_coef, ent_coef = 0.2, 0.5, 0.0

    # what the rollout's last step leaves for the next rollout's row 0
    carry_obs, carry_start = torch.empty((E, D), device=dev), torch.ones(E, device=dev, dtype=torch.uint8)
    reward = torch.empty(E, device=dev, dtype=torch.float64)
    env.reset_torch(obs_out=carry_obs)

    for it in range(args.iterations):
        buf.reset()
        obs, start = carry_obs, carry_start
        with torch.no_grad():
            for t in range(K):
                d = net.dist(obs)
                act = d.sample()
                value, logp = net.vf(obs), d.log_prob(act).sum(-1)
                nxt = buf.slot(t + 1) if t + 1 < K else None
                nobs, ndone = (nxt.obs, nxt.episode_start) if nxt else (carry_obs, carry_start)
                clipped = act.clamp(-1, 1)  # the env sees the clipped action, the buffer keeps the sampled one (as SB3 does)
                if nobs is obs:  # (K = 1: the carry buffers are still being read)
                    obs, start = obs.clone(), start.clone()
                env.step_torch(clipped, obs_out=nobs, reward_out=reward, done_out=ndone)
                buf.add(obs, act, reward, start, value, logp)  # obs / start of rows >= 1 already are the row: not copied
                obs, start = nobs, ndone
            buf.compute_returns_and_advantage(net.vf(obs), start)

        pl = vl = torch.zeros((), device=dev)
        for _ in range(args.epochs):
            for b in buf.get(args.batch_size):
                values, logp, entropy = net.evaluate(b.observations, b.actions)
                adv = (b.advantages - b.advantages.mean()) / (b.advantages.std() + 1e-8)
                ratio = (logp - b.old_log_prob).exp()
                pl = -torch.min(adv * ratio, adv * ratio.clamp(1 - clip_range, 1 + clip_range)).mean()
                vl = nn.functional.mse_loss(values, b.returns)
                loss = pl + vf_coef * vl - ent_coef * entropy.mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                nn.utils.clip_grad_norm_(net.parameters(), 0.5)
                opt.step()
        buf.check_errors()
        # the only transfers of the iteration: three numbers for the log
        print(json.dumps({"iteration": it, "policy_loss": pl.item(), "value_loss": vl.item(), "mean_reward": buf.rewards.mean().item(),
                          "episode_starts": int(buf.episode_starts.sum().item())}), flush=True)
    buf.close()
    env.close()


if __name__ == "__main__":
    main()
