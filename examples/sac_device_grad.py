#!/usr/bin/env python3
"""A short SAC loop whose gradient step runs without autograd (`fleetrl_amd.sac.gradient_step`): the soft target,
the critics' gradients and Adam step (`critic_update`), the actor's and the entropy coefficient's gradients in two launches
(`DeviceSACGrad.actor_grad`) with their Adam steps (`actor_update`), and the Polyak update.  There is no `backward()` anywhere in the
loop; torch's share of a gradient step is the `exp` of the one-element `log_ent_coef`.

The actor is SB3's: `latent_pi`, then the two heads `mu` and `log_std`.  `fused_head_parameters` re-points the heads' tensors at the
halves of ONE `[2A, H]` pair, which is what the device differentiates and steps, so torch's own `actor.mu` / `actor.log_std` follow
every step without a copy.

Warm-up actions are uniform.  It shows that the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/sac_device_grad.py [--steps 40] [--envs 64] [--evs 5] [--batch 256] [--learning-starts 4] [--check]

Prints one JSON line per logging interval.  `--check` replays every gradient step on a copy of the networks under torch autograd and
`torch.optim.Adam` (float32, on the GPU, the device's own recorded draws) and prints the largest relative difference of the
parameters at the end.
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
from fleetrl_amd import (DeviceAdam, DevicePolicy, DeviceReplayBuffer, DeviceSACGrad, DeviceSACNetworks, FleetVecEnv,  # noqa: E402
                         FleetVecNormalize)
from fleetrl_amd.sac import CRITIC_LOSS_SCALE, fused_head_parameters, gradient_step  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


class Actor(nn.Module):
    """SB3's SAC actor: latent_pi, then mu and log_std over the same latent."""

    def __init__(self, D, A, hidden):
        super().__init__()
        self.latent_pi = nn.Sequential(nn.Linear(D, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())
        self.mu, self.log_std = nn.Linear(hidden, A), nn.Linear(hidden, A)

    def action_log_prob(self, obs, eps):
        h = self.latent_pi(obs)
        mean, log_std = self.mu(h), self.log_std(h).clamp(-20.0, 2.0)
        std = log_std.exp()
        u = mean + std * eps
        a = torch.tanh(u)
        return a, torch.distributions.Normal(mean, std).log_prob(u).sum(1) - torch.log(1.0 - a * a + 1e-6).sum(1)


def critic(D, A, hidden):
    return nn.Sequential(nn.Linear(D + A, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, 1))


def linear_layers(net):
    return [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]


class AutogradTwin:
    """The same gradient step as SB3 writes it, on copies of the networks: the `--check` arm."""

    def __init__(self, actor, q1, q2, log_alpha, lr):
        self.actor, self.q1, self.q2 = copy.deepcopy(actor), copy.deepcopy(q1), copy.deepcopy(q2)
        self.log_alpha = log_alpha.detach().clone().requires_grad_(True)
        self.opt_a = torch.optim.Adam(self.actor.parameters(), lr=lr)
        self.opt_c = torch.optim.Adam([*self.q1.parameters(), *self.q2.parameters()], lr=lr)
        self.opt_e = torch.optim.Adam([self.log_alpha], lr=lr)
        self.tq1, self.tq2 = copy.deepcopy(q1), copy.deepcopy(q2)

    def step(self, b, eps, target_eps, gamma, tau, target_entropy):
        pi, log_pi = self.actor.action_log_prob(b.observations, eps)
        alpha = self.log_alpha.detach().exp()
        ent_loss = -(self.log_alpha * (log_pi + target_entropy).detach()).mean()
        self.opt_e.zero_grad()
        ent_loss.backward()
        self.opt_e.step()
        with torch.no_grad():
            na, nlp = self.actor.action_log_prob(b.next_observations, target_eps)
            x = torch.cat([b.next_observations, na], 1)
            nq = torch.min(self.tq1(x), self.tq2(x)) - alpha * nlp.view(-1, 1)
            y = b.rewards.view(-1, 1) + (1.0 - b.dones.view(-1, 1)) * gamma * nq
        x = torch.cat([b.observations, b.actions], 1)
        c_loss = 0.5 * (nn.functional.mse_loss(self.q1(x), y) + nn.functional.mse_loss(self.q2(x), y))
        self.opt_c.zero_grad()
        c_loss.backward()
        self.opt_c.step()
        x = torch.cat([b.observations, pi], 1)
        a_loss = (alpha * log_pi.view(-1, 1) - torch.min(self.q1(x), self.q2(x))).mean()
        self.opt_a.zero_grad()
        a_loss.backward()
        self.opt_a.step()
        with torch.no_grad():
            for net, tgt in ((self.q1, self.tq1), (self.q2, self.tq2)):
                for p, t in zip(net.parameters(), tgt.parameters()):
                    t.mul_(1 - tau).add_(p, alpha=tau)

    def parameters(self):
        return [*self.actor.parameters(), *self.q1.parameters(), *self.q2.parameters(), self.log_alpha]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--buffer-size", type=int, default=20_000)
    ap.add_argument("--learning-starts", type=int, default=4)
    ap.add_argument("--log-interval", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    E, N, B = args.envs, args.evs, args.batch
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    env = FleetVecNormalize(FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=args.seed), clip_reward=10.0)
    D = env.norm.D
    actor, q1, q2 = Actor(D, N, args.hidden).to(dev), critic(D, N, args.hidden).to(dev), critic(D, N, args.hidden).to(dev)
    gamma, tau, lr, target_entropy = 0.99, 0.005, 3e-4, -float(N)
    log_alpha = torch.zeros(1, device=dev, requires_grad=True)
    twin = AutogradTwin(actor, q1, q2, log_alpha, lr) if args.check else None
    head_w, head_b = fused_head_parameters(actor)  # actor.mu / actor.log_std are views of this pair from here on
    actor_params = [*actor.latent_pi.parameters(), head_w, head_b]
    critic_params = [*q1.parameters(), *q2.parameters()]
    shapes = (linear_layers(actor.latent_pi) + [(head_w, head_b)], [linear_layers(q1), linear_layers(q2)])
    nets, targets = DeviceSACNetworks(*shapes, activation="relu"), DeviceSACNetworks(*shapes, activation="relu")
    grad = DeviceSACGrad(nets, B)
    opt_a = DeviceAdam(nets, actor_params, nets="actor", lr=lr)
    opt_c = DeviceAdam(nets, critic_params, nets="critic", lr=lr)
    opt_e = DeviceAdam(nets, [log_alpha], nets="none", lr=lr)
    alpha = torch.ones(1, device=dev)
    warmup = DevicePolicy([(torch.zeros((N, D)), torch.zeros(N))])  # sample_uniform runs no network
    buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
    act_seed, grad_seed, target_seed = args.seed + 0xAC7, args.seed + 0x6AD, args.seed + 0x7A26E7  # three draws, three seeds

    obs, reward, done = torch.empty((E, D), device=dev), torch.empty(E, device=dev, dtype=torch.float64), torch.empty(E, device=dev, dtype=torch.uint8)
    terminal, last_raw, act = torch.empty((E, D), device=dev), torch.empty((E, D), device=dev), torch.empty((E, N), device=dev)
    env.reset_torch(obs_out=obs)
    last_raw.copy_(env.original_torch().obs)
    critic_stats, actor_stats = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    eps, target_eps = torch.empty((B, N), device=dev), torch.empty((B, N), device=dev)
    updates = 0

    for step in range(1, args.steps + 1):
        with torch.no_grad():
            if step <= args.learning_starts:
                warmup.sample_uniform(E, seed=act_seed, step=step, actions_out=act, env_actions_out=act)
            else:
                nets.act(obs, seed=act_seed, step=step, actions_out=act)
            env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
            raw = env.original_torch()
            buf.add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
            last_raw.copy_(raw.obs)

        if step > args.learning_starts:
            b = buf.sample(B, env=env)
            if twin is not None:  # the draws of this step, recorded under the same keys, and SB3's step on the copies
                nets.act(b.observations, seed=grad_seed, step=updates, noise=eps)
                nets.act(b.next_observations, seed=target_seed, step=updates, noise=target_eps)
                twin.step(b, eps, target_eps, gamma, tau, target_entropy)
            gradient_step(nets, targets, grad, opt_a, opt_c, b, actor_params, critic_params, gamma=gamma, tau=tau, seed=grad_seed,
                          target_seed=target_seed, step=updates, log_ent_coef=log_alpha, ent_adam=opt_e, target_entropy=target_entropy,
                          alpha_out=alpha, critic_stats_out=critic_stats, actor_stats_out=actor_stats)
            updates += 1

        if step % args.log_interval == 0 or step == args.steps:
            buf.check_errors()
            line = {"step": step, "gradient_steps": updates, "backward_calls": 0, "critic_loss": CRITIC_LOSS_SCALE * critic_stats[0].item(),
                    "actor_loss": actor_stats[0].item(), "ent_coef_loss": actor_stats[1].item(), "ent_coef": alpha.item()}
            if twin is not None and step == args.steps:
                mine = [*actor.parameters(), *q1.parameters(), *q2.parameters(), log_alpha]
                rel = max(((p.detach() - q.detach()).abs().max() / q.detach().abs().max().clamp_min(1e-12)).item()
                          for p, q in zip(mine, twin.parameters()))
                line["check"] = {"max_relative_difference": rel, "tensors": len(mine)}
            print(json.dumps(line), flush=True)

    for h in (opt_e, opt_c, opt_a, grad, targets, nets, warmup, buf, env):
        h.close()


if __name__ == "__main__":
    main()
