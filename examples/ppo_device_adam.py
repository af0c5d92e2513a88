#!/usr/bin/env python3
"""The loop of examples/ppo_device_grad.py with the optimiser on the device as well: FleetVecEnv + FleetVecNormalize +
DevicePolicy.sample + DeviceRolloutBuffer + DevicePPOGrad + DeviceAdam; torch keeps the advantage normalisation.

Per minibatch: `DevicePPOGrad.grad` -- two launches -- writes the gradients into the `.grad` of torch's own parameters, and
`DeviceAdam.step` -- two launches -- replaces `clip_grad_norm_`, `opt.step()` and `load_torch`: the global norm in a stated order,
SB3's clip at 0.5, torch's Adam update, every new weight written both to the torch parameter and to the device policy's weight
image.  A gradient step is four launches, deterministic from the minibatch to the weights.  For the first minibatch torch's own
clip + Adam runs on a copy of the parameters, and the largest difference between the two sets of stepped parameters is printed.

Per rollout step: `DevicePolicy.sample` reads the observations where the last step wrote them -- row t of the buffer --, runs the
actor and the critic, draws the Gaussian noise on the device (Philox, keyed by the seed, the env and the global step count) and
writes the sampled action, the value and the log-probability straight into row t; the env steps on the clipped action; `add` stores
the reward and leaves the rest of the row alone.  The optimiser step itself refreshes the device policy's weights, no
host synchronisation; `log_std` is read from the torch parameter when a launch runs.  It shows that the pieces fit -- it is not a
tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/ppo_device_adam.py [--iterations 3] [--envs 256] [--evs 5] [--steps 64] [--batch-size 1024] [--epochs 2]

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
from fleetrl_amd import DeviceAdam, DevicePolicy, DevicePPOGrad, DeviceRolloutBuffer, FleetVecEnv, FleetVecNormalize  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


class ActorCritic(nn.Module):
    """SB3's MlpPolicy in small: separate tanh MLPs for the Gaussian mean and the value, a state-independent log std."""

    def __init__(self, obs_dim, act_dim, hidden=64):
        super().__init__()
        mlp = lambda out: nn.Sequential(nn.Linear(obs_dim, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(), nn.Linear(hidden, out))  # noqa: E731
        self.pi, self.vf = mlp(act_dim), mlp(1)
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    def evaluate(self, obs, actions):
        d = torch.distributions.Normal(self.pi(obs), self.log_std.exp())
        return self.vf(obs).squeeze(-1), d.log_prob(actions).sum(-1), d.entropy().sum(-1)

    def linear_parameters(self):
        """W, b per layer, the actor's then the critic's: the order DevicePolicy.load_torch takes."""
        return [p for net in (self.pi, self.vf) for m in net if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]


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
    buf = DeviceRolloutBuffer(E, K, D, N, gamma=0.99, gae_lambda=0.95)
    params = net.linear_parameters()
    layers = lambda ps: [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]  # noqa: E731
    pol = DevicePolicy(layers(params[:6]), critic_layers=layers(params[6:]), activation="tanh", output="clip")
    grad = DevicePPOGrad(pol, min(args.batch_size, E * K))
    into = params + [net.log_std]  # load_torch's order, then log_std
    opt = DeviceAdam(pol, into, lr=3e-4, eps=1e-5, max_grad_norm=0.5)  # SB3's PPO: Adam with eps 1e-5, gradients clipped at 0.5
    grad_norm = torch.zeros(1, device=dev)
    checked = False
    env_act, last_value = torch.empty((E, N), device=dev), torch.empty((E, 1), device=dev)
    steps = 0  # the noise's step counter: never repeats over the run
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
                row = buf.slot(t)
                # one launch: actor, critic, noise; the sampled action, the value and the log-probability land in row t, the
                # clipped action the env sees (the buffer keeps the sampled one, as SB3 does) in env_act
                pol.sample(obs, net.log_std, seed=args.seed, step=steps, actions_out=row.actions, env_actions_out=env_act,
                           log_prob_out=row.log_prob, values_out=row.value)
                steps += 1
                nxt = buf.slot(t + 1) if t + 1 < K else None
                nobs, ndone = (nxt.obs, nxt.episode_start) if nxt else (carry_obs, carry_start)
                if nobs is obs:  # (K = 1: the carry buffers are still being read)
                    obs, start = obs.clone(), start.clone()
                env.step_torch(env_act, obs_out=nobs, reward_out=reward, done_out=ndone)
                buf.add(obs, row.actions, reward, start, row.value, row.log_prob)  # what already is the row is not copied
                obs, start = nobs, ndone
            pol.act(obs, out=env_act, values_out=last_value)  # the bootstrap value (the action is not used)
            buf.compute_returns_and_advantage(last_value, start)

        stats = torch.zeros(8, device=dev)
        for _ in range(args.epochs):
            for b in buf.get(args.batch_size):
                adv = (b.advantages - b.advantages.mean()) / (b.advantages.std() + 1e-8)
                stats = grad.grad(b, net.log_std, clip_range, vf_coef, ent_coef, into=into, advantages=adv)
                if not checked:  # once: torch's own clip + Adam on a copy of the parameters, from the same gradients
                    copy = [nn.Parameter(p.detach().clone()) for p in into]
                    for c, p in zip(copy, into):
                        c.grad = p.grad.clone()
                    ref = torch.optim.Adam(copy, lr=3e-4, eps=1e-5)
                    ref_norm = nn.utils.clip_grad_norm_(copy, 0.5)
                    ref.step()
                opt.step(norm_out=grad_norm)  # two launches: the norm; clip, Adam and the image's new weights
                if not checked:
                    checked = True
                    print(json.dumps({"max_abs_param_diff_to_torch_adam": max(float((p.detach() - c.detach()).abs().max()) for p, c in zip(into, copy)),
                                      "grad_norm": grad_norm.item(), "torch_grad_norm": float(ref_norm)}), flush=True)
        buf.check_errors()
        # the only transfers of the iteration: the last minibatch's statistics and two numbers for the log
        st = stats.tolist()
        print(json.dumps({"iteration": it, "policy_loss": st[0], "value_loss": st[1], "approx_kl": st[4], "clip_fraction": st[5],
                          "mean_reward": buf.rewards.mean().item(), "episode_starts": int(buf.episode_starts.sum().item())}), flush=True)
    opt.close()
    grad.close()
    pol.close()
    buf.close()
    env.close()


if __name__ == "__main__":
    main()
