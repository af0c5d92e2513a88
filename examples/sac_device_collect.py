#!/usr/bin/env python3
"""An SB3-style SAC iteration as three enqueue-only calls: `DeviceSACCollect.collect` (`OffPolicyAlgorithm.collect_rollouts`: uniform
actions while the ring warms up, then the squashed-Gaussian sample, the env's step, the normaliser's step and the buffer's add per env
step, and `rollout/*` at the end), `DeviceSACTrain.train` (`SAC.train`: every gradient step of the update) and, every k-th iteration,
`DeviceEvalCallback.evaluate` on the SAC networks (`EvalCallback`: deterministic episodes on an evaluation env, the best weights -- the
actor and the critics -- kept on the device).  Nothing in between waits for the device: the host reads sixteen numbers per call for the
log.  It shows that the pieces fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/sac_device_collect.py [--iterations 4] [--steps 4] [--gradient-steps 2] [--eval-every 2] [--envs 8] [--evs 2]
                                          [--learning-starts 6] [--check]

Prints one JSON line per iteration: `rollout/*`, `train/*` and, when it evaluated, `eval/*`.  `--check` keeps a second, identically
built env and agent, replays every collect on them step by step from the public pieces (`DeviceSACNetworks.sample_uniform` / `act`,
`step_torch`, `DeviceReplayBuffer.add`) and compares the replay buffers, the carried observations and every weight bit for bit.
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
from fleetrl_amd import (DeviceAdam, DeviceEvalCallback, DeviceReplayBuffer, DeviceSACCollect, DeviceSACGrad, DeviceSACNetworks,  # noqa: E402
                         DeviceSACTrain, FleetVecEnv, FleetVecNormalize)
from fleetrl_amd.collect import SB3_NAMES  # noqa: E402
from fleetrl_amd.sac import fused_head_parameters  # noqa: E402
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


def make_env(args, E, seed):
    cfg = dict(bench_config(E, args.evs, "ct"), episode_length=args.episode_hours)
    return FleetVecNormalize(FleetVecEnv(cfg, E, tables=synth_tables("ct", args.evs), seed=seed), clip_reward=10.0)


class Agent:
    """One SAC agent on copies of the given torch networks, with an env of its own."""

    def __init__(self, actor, q1, q2, args, lr, dev):
        E, N = args.envs, args.evs
        self.env = make_env(args, E, args.seed)
        self.D = D = self.env.norm.D
        self.actor, self.q1, self.q2 = copy.deepcopy(actor), copy.deepcopy(q1), copy.deepcopy(q2)
        self.log_alpha = torch.zeros(1, device=dev, requires_grad=True)
        head_w, head_b = fused_head_parameters(self.actor)  # actor.mu / actor.log_std are views of this pair from here on
        self.actor_params = [*self.actor.latent_pi.parameters(), head_w, head_b]
        self.critic_params = [*self.q1.parameters(), *self.q2.parameters()]
        shapes = (linear_layers(self.actor.latent_pi) + [(head_w, head_b)], [linear_layers(self.q1), linear_layers(self.q2)])
        self.nets, self.targets = DeviceSACNetworks(*shapes, activation="relu"), DeviceSACNetworks(*shapes, activation="relu")
        self.grad = DeviceSACGrad(self.nets, args.batch_size)
        self.opt_a = DeviceAdam(self.nets, self.actor_params, nets="actor", lr=lr)
        self.opt_c = DeviceAdam(self.nets, self.critic_params, nets="critic", lr=lr)
        self.opt_e = DeviceAdam(self.nets, [self.log_alpha], nets="none", lr=lr)
        self.buf = DeviceReplayBuffer(args.buffer_size, E, D, N, seed=args.seed)
        self.train = DeviceSACTrain(self.buf, self.targets, self.grad, self.opt_a, self.opt_c, self.opt_e, max_steps=args.gradient_steps)

    def tensors(self):
        b = self.buf
        return [*self.actor_params, *self.critic_params, self.log_alpha, *self.targets.export_torch(), b.observations, b.next_observations, b.actions,
                b.rewards, b.dones]

    def close(self):
        for h in (self.train, self.opt_e, self.opt_c, self.opt_a, self.grad, self.targets, self.nets, self.buf, self.env):
            h.close()


class StepByStep:
    """The collect call replayed from the public pieces on a twin agent: the Python loop a SAC agent ran before."""

    def __init__(self, agent, args, dev):
        E, D, N = args.envs, agent.D, args.evs
        self.agent = agent
        self.obs, self.last_raw, self.terminal = (torch.empty((E, D), device=dev) for _ in range(3))
        self.act = torch.empty((E, N), device=dev)
        self.reward, self.done = torch.empty(E, device=dev, dtype=torch.float64), torch.empty(E, device=dev, dtype=torch.uint8)
        agent.env.reset_torch(obs_out=self.obs)
        self.last_raw.copy_(agent.env.original_torch().obs)

    def collect(self, n_steps, *, learning_starts, seed, first_step):
        a, env = self.agent, self.agent.env
        for t in range(n_steps):
            s = first_step + t
            if s < learning_starts:
                a.nets.sample_uniform(self.act.shape[0], seed=seed, step=s, actions_out=self.act)
            else:
                a.nets.act(self.obs, seed=seed, step=s, actions_out=self.act)
            env.step_torch(self.act, obs_out=self.obs, reward_out=self.reward, done_out=self.done, terminal_out=self.terminal)
            raw = env.original_torch()
            a.buf.add(self.last_raw, raw.obs, self.act, raw.reward, self.done, terminal=raw.terminal)
            self.last_raw.copy_(raw.obs)


def bits_equal(xs, ys):
    return all(torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)) for p, q in zip(xs, ys))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4, help="env steps per collect (SB3's train_freq)")
    ap.add_argument("--gradient-steps", type=int, default=2)
    ap.add_argument("--learning-starts", type=int, default=6, help="env steps (per env) of uniform actions")
    ap.add_argument("--eval-every", type=int, default=2, help="evaluate every k-th iteration")
    ap.add_argument("--eval-envs", type=int, default=3)
    ap.add_argument("--eval-episodes", type=int, default=3)
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--evs", type=int, default=2)
    ap.add_argument("--episode-hours", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--buffer-size", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    E, N = args.envs, args.evs
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)

    probe = make_env(args, 1, args.seed)  # (the observation width, before the networks exist)
    D = probe.norm.D
    probe.close()
    actor, q1, q2 = Actor(D, N, args.hidden).to(dev), critic(D, N, args.hidden).to(dev), critic(D, N, args.hidden).to(dev)
    gamma, tau, lr = 0.99, 0.005, 3e-4
    agent = Agent(actor, q1, q2, args, lr, dev)
    collector = DeviceSACCollect(agent.env, agent.nets, stats_window=100)
    eval_env = make_env(args, args.eval_envs, args.seed + 1)
    evaluator = DeviceEvalCallback(agent.nets, eval_env, n_eval_episodes=args.eval_episodes, train_normalizer=agent.env)
    twin = Agent(actor, q1, q2, args, lr, dev) if args.check else None
    replay = StepByStep(twin, args, dev) if twin is not None else None
    act_seed, grad_seed, target_seed = args.seed + 0xAC7, args.seed + 0x6AD, args.seed + 0x7A26E7  # three draws, three seeds

    collector.reset()
    rollout, trained = (torch.zeros(16, device=dev, dtype=torch.float64) for _ in range(2))
    steps = updates = 0
    for it in range(1, args.iterations + 1):
        ckw = dict(learning_starts=args.learning_starts, seed=act_seed, first_step=steps)
        collector.collect(agent.buf, args.steps, stats_out=rollout, **ckw)
        steps += args.steps
        tkw = dict(gradient_steps=args.gradient_steps, batch_size=args.batch_size, lr=lr, gamma=gamma, tau=tau, seed=grad_seed,
                   target_seed=target_seed, first_update=updates)
        agent.train.train(agent.actor_params, agent.critic_params, log_ent_coef=agent.log_alpha, env=agent.env, stats_out=trained, **tkw)
        updates += args.gradient_steps
        evaluated = it % args.eval_every == 0
        if evaluated:
            evaluator.evaluate(steps * E)
        r, t = rollout.tolist(), trained.tolist()  # the transfers: sixteen numbers per call for the log
        line = {"iteration": it, "time/total_timesteps": steps * E, **{name: r[k] for k, name in enumerate(SB3_NAMES) if name},
                "rollout/total_episodes": int(r[3]), **{name: t[k] for k, name in enumerate(SAC_TRAIN_SB3_NAMES) if name}}
        line["train/n_updates"] = int(line["train/n_updates"])
        if evaluated:
            line.update(evaluator.results())
        if twin is not None:
            replay.collect(args.steps, **ckw)
            twin.train.train(twin.actor_params, twin.critic_params, log_ent_coef=twin.log_alpha, env=twin.env, **tkw)
            same = bits_equal(agent.tensors(), twin.tensors()) and bits_equal([collector.carry_obs, collector.raw_obs], [replay.obs, replay.last_raw])
            same = same and (agent.buf.pos, agent.buf.full) == (twin.buf.pos, twin.buf.full)
            line["check"] = "bit-equal" if same else "DIFFERENT"
        print(json.dumps(line), flush=True)
        if line.get("check") == "DIFFERENT":
            sys.exit("the one call and the pieces called step by step disagree")
    agent.buf.check_errors()
    collector.check_errors()

    for h in (evaluator, collector, eval_env, agent, twin):
        if h is not None:
            h.close()


if __name__ == "__main__":
    main()
