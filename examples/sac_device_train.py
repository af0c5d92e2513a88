#!/usr/bin/env python3
"""The SAC loop of examples/sac_device_grad.py with its gradient steps replaced by ONE call per update: `DeviceSACTrain.train` enqueues
`gradient_steps` gradient steps -- per step `sample`, alpha = exp(log_ent_coef) read before its optimiser steps, the soft target, the
critics' gradients times 0.5 and their Adam step, the actor's and the entropy coefficient's gradients with their Adam steps and, on
the steps g of the call with g % target_update_interval == 0, the Polyak update from the ONLINE weight image -- and one closing launch
that writes what SB3 logs as `train/*`.  The loop passes the number of gradient steps taken so far; no tensor
crosses to the host inside it.

A ring is filled with `DeviceSACNetworks.act` (uniform actions while it warms up), then collecting and calls of `train` alternate.  It
shows that the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/sac_device_train.py [--updates 10] [--gradient-steps 8] [--collect 4] [--envs 64] [--evs 5] [--batch 256]
                                        [--target-update-interval 1] [--check]

Prints one JSON line per update.  `--check` keeps a second, identically loaded set of handles and replays every update on it step by
step from the public pieces (`DeviceSACTrain.alpha`, `critic_update`, `actor_update`, `targets.polyak`), then compares every parameter,
the targets and `log_ent_coef` bit for bit.
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
from fleetrl_amd import (DeviceAdam, DevicePolicy, DeviceReplayBuffer, DeviceSACGrad, DeviceSACNetworks, DeviceSACTrain, FleetVecEnv,  # noqa: E402
                         FleetVecNormalize)
from fleetrl_amd.sac import actor_update, critic_update, fused_head_parameters  # noqa: E402
from fleetrl_amd.sac_train import SAC_TRAIN_SB3_NAMES  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


class Actor(nn.Module):
    """SB3's SAC actor: latent_pi, then mu and log_std over the same latent."""

    def __init__(self, D, A, hidden):
        super().__init__()
        self.latent_pi = nn.Sequential(nn.Linear(D, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())
        self.mu, self.log_std = nn.Linear(hidden, A), nn.Linear(hidden, A)


def critic(D, A, hidden):
    return nn.Sequential(nn.Linear(D + A, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, 1))


def linear_layers(net):
    return [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]


class Agent:
    """Every handle of one SAC agent on copies of the given torch networks."""

    def __init__(self, actor, q1, q2, args, E, D, N, lr, dev):
        self.actor, self.q1, self.q2 = copy.deepcopy(actor), copy.deepcopy(q1), copy.deepcopy(q2)
        self.log_alpha = torch.zeros(1, device=dev, requires_grad=True)
        head_w, head_b = fused_head_parameters(self.actor)  # actor.mu / actor.log_std are views of this pair from here on
        self.actor_params = [*self.actor.latent_pi.parameters(), head_w, head_b]
        self.critic_params = [*self.q1.parameters(), *self.q2.parameters()]
        shapes = (linear_layers(self.actor.latent_pi) + [(head_w, head_b)], [linear_layers(self.q1), linear_layers(self.q2)])
        self.nets, self.targets = DeviceSACNetworks(*shapes, activation="relu"), DeviceSACNetworks(*shapes, activation="relu")
        self.grad = DeviceSACGrad(self.nets, args.batch)
        self.opt_a = DeviceAdam(self.nets, self.actor_params, nets="actor", lr=lr)
        self.opt_c = DeviceAdam(self.nets, self.critic_params, nets="critic", lr=lr)
        self.opt_e = DeviceAdam(self.nets, [self.log_alpha], nets="none", lr=lr)
        self.buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
        self.train = DeviceSACTrain(self.buf, self.targets, self.grad, self.opt_a, self.opt_c, self.opt_e, max_steps=args.gradient_steps)
        self.alpha, self.stats8 = torch.ones(1, device=dev), torch.zeros(8, device=dev)

    def step_by_step(self, env, *, G, B, gamma, tau, seed, target_seed, first_update, interval):
        """The same update from the public pieces, one gradient step after the other."""
        for g in range(G):
            u = first_update + g
            b = self.buf.sample(B, env=env)
            alpha = self.train.alpha(self.log_alpha, out=self.alpha)
            critic_update(self.nets, self.targets, self.grad, self.opt_c, b, self.critic_params, gamma=gamma, ent_coef=alpha, seed=target_seed,
                          step=u, stats_out=self.stats8)
            actor_update(self.grad, self.opt_a, b.observations, self.actor_params, ent_coef=alpha, seed=seed, step=u,
                         log_ent_coef=self.log_alpha, ent_adam=self.opt_e, stats_out=self.stats8)
            if g % interval == 0:
                self.targets.polyak([*self.actor_params, *self.critic_params], tau)

    def tensors(self):
        return [*self.actor_params, *self.critic_params, self.log_alpha, *self.targets.export_torch()]

    def close(self):
        for h in (self.train, self.opt_e, self.opt_c, self.opt_a, self.grad, self.targets, self.nets, self.buf):
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--gradient-steps", type=int, default=8)
    ap.add_argument("--collect", type=int, default=4, help="env steps between two updates (and before the first)")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--buffer-size", type=int, default=20_000)
    ap.add_argument("--target-update-interval", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    E, N, B, G = args.envs, args.evs, args.batch, args.gradient_steps
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    env = FleetVecNormalize(FleetVecEnv(bench_config(E, N, "ct"), E, tables=synth_tables("ct", N), seed=args.seed), clip_reward=10.0)
    D = env.norm.D
    actor, q1, q2 = Actor(D, N, args.hidden).to(dev), critic(D, N, args.hidden).to(dev), critic(D, N, args.hidden).to(dev)
    gamma, tau, lr = 0.99, 0.005, 3e-4
    agent = Agent(actor, q1, q2, args, E, D, N, lr, dev)
    twin = Agent(actor, q1, q2, args, E, D, N, lr, dev) if args.check else None
    warmup = DevicePolicy([(torch.zeros((N, D)), torch.zeros(N))])  # sample_uniform runs no network
    act_seed, grad_seed, target_seed = args.seed + 0xAC7, args.seed + 0x6AD, args.seed + 0x7A26E7  # three draws, three seeds

    obs, reward, done = torch.empty((E, D), device=dev), torch.empty(E, device=dev, dtype=torch.float64), torch.empty(E, device=dev, dtype=torch.uint8)
    terminal, last_raw, act = torch.empty((E, D), device=dev), torch.empty((E, D), device=dev), torch.empty((E, N), device=dev)
    env.reset_torch(obs_out=obs)
    last_raw.copy_(env.original_torch().obs)
    stats = torch.zeros(16, device=dev, dtype=torch.float64)
    updates = step = 0

    for update in range(1, args.updates + 1):
        with torch.no_grad():
            for _ in range(args.collect):
                step += 1
                if update == 1:
                    warmup.sample_uniform(E, seed=act_seed, step=step, actions_out=act, env_actions_out=act)
                else:
                    agent.nets.act(obs, seed=act_seed, step=step, actions_out=act)
                env.step_torch(act, obs_out=obs, reward_out=reward, done_out=done, terminal_out=terminal)
                raw = env.original_torch()
                for a in (agent, twin):
                    if a is not None:
                        a.buf.add(last_raw, raw.obs, act, raw.reward, done, terminal=raw.terminal)
                last_raw.copy_(raw.obs)
        kw = dict(gamma=gamma, tau=tau, seed=grad_seed, target_seed=target_seed, first_update=updates)
        # every gradient step of this update, enqueued by one call; normalised with the statistics as they are now
        agent.train.train(agent.actor_params, agent.critic_params, gradient_steps=G, batch_size=B, lr=lr,
                          target_update_interval=args.target_update_interval, log_ent_coef=agent.log_alpha, env=env, stats_out=stats, **kw)
        if twin is not None:
            twin.step_by_step(env, G=G, B=B, interval=args.target_update_interval, **kw)
        updates += G
        agent.buf.check_errors()
        host = stats.tolist()  # the only transfer: sixteen numbers for the log
        line = {"update": update, "env_steps": step, **{name: host[k] for k, name in enumerate(SAC_TRAIN_SB3_NAMES) if name}}
        line["train/n_updates"] = int(line["train/n_updates"])
        if twin is not None and update == args.updates:
            mine, theirs = agent.tensors(), twin.tensors()
            equal = all(torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)) for p, q in zip(mine, theirs))
            line["check"] = {"bit_equal": bool(equal), "tensors": len(mine), "calls": [agent.buf.calls, twin.buf.calls]}
        print(json.dumps(line), flush=True)

    for h in (agent, twin, warmup, env):
        if h is not None:
            h.close()


if __name__ == "__main__":
    main()
