#!/usr/bin/env python3
"""The loop of examples/ppo_device_adam.py with the whole update as ONE call: FleetVecEnv + FleetVecNormalize + DevicePolicy.sample +
DeviceRolloutBuffer + DevicePPOGrad + DeviceAdam + DevicePPOTrain.

Per iteration `DevicePPOTrain.train` enqueues SB3's `PPO.train()` -- `--epochs` passes over the rollout in freshly shuffled minibatches
of `--batch-size` rows, the advantages normalised per minibatch, five launches per minibatch and one closing launch -- and returns one
block of statistics on the device: the means of the loss terms over all minibatches, the buffer's explained variance and the mean
standard deviation, printed under SB3's `train/*` names.  No `torch.randperm`, no Python loop over minibatches, no torch reduction: the
shuffle is a keyed bijection evaluated on the device under (seed, the number of epochs trained so far), so a run is reproducible from
its seed and a checkpoint needs that count only.  The rollout is the one of examples/ppo_device_adam.py.  It shows that the pieces
fit -- it is not a tuned trainer.  Needs an MI355X; inputs are synthetic:

    python examples/ppo_device_train.py [--iterations 3] [--envs 256] [--evs 5] [--steps 64] [--batch-size 128] [--epochs 4]
                                        [--clip-range-vf 0.2] [--no-normalize-advantage] [--target-kl 0.01] [--time]

`--clip-range-vf` is SB3's `clip_range_vf` (off by default, as in SB3): the value loss on the prediction clipped around the rollout's
values, inside the same launches.  `--no-normalize-advantage` is `normalize_advantage=False`.  `--target-kl` is SB3's `target_kl` (off
by default): the device stops the update at the first minibatch whose approx_kl exceeds 1.5 times it, and the line also carries the
optimiser steps taken, the epochs entered, whether the update stopped, the approx_kl compared last and its mean over the last epoch
(what SB3 logs as train/approx_kl); `train/n_updates` then counts epochs entered, as SB3 does.  Prints one JSON line per iteration;
with `--time` one more line: the host wall time of further updates on the last rollout, the final synchronisation included.
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
from fleetrl_amd import DeviceAdam, DevicePolicy, DevicePPOGrad, DevicePPOTrain, DeviceRolloutBuffer, FleetVecEnv, FleetVecNormalize  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402
from fleetrl_amd.train import KL_SB3_NAMES, SB3_NAMES  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--evs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--clip-range-vf", type=float, default=None, help="SB3's clip_range_vf; default: no value clipping")
    ap.add_argument("--no-normalize-advantage", action="store_true", help="SB3's normalize_advantage=False")
    ap.add_argument("--target-kl", type=float, default=None, help="SB3's target_kl; default: no early stopping")
    ap.add_argument("--time", action="store_true", help="after the last iteration, time the update alone on its rollout")
    ap.add_argument("--reps", type=int, default=7, help="updates timed by --time")
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
    trainer = DevicePPOTrain(buf, grad, opt)
    env_act, last_value = torch.empty((E, N), device=dev), torch.empty((E, 1), device=dev)
    steps = 0   # the noise's step counter: never repeats over the run
    epochs = 0  # the shuffle's epoch counter: never repeats over the run either
    n_updates = 0
    clip_range, vf_coef, ent_coef = 0.2, 0.5, 0.0
    # (None is the default of train(): the argument is passed only when it is set)
    extra = {} if args.clip_range_vf is None else {"clip_range_vf": args.clip_range_vf}
    if args.target_kl is not None:
        extra["target_kl"] = args.target_kl
    names = SB3_NAMES if args.target_kl is None else SB3_NAMES + KL_SB3_NAMES
    normalize = not args.no_normalize_advantage

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

        # the whole update: one call, enqueued behind the rollout on the same stream
        stats = trainer.train(into, n_epochs=args.epochs, batch_size=args.batch_size, clip_range=clip_range, vf_coef=vf_coef,
                              ent_coef=ent_coef, lr=3e-4, normalize_advantage=normalize, seed=args.seed, first_epoch=epochs, **extra)
        epochs += args.epochs
        buf.check_errors()
        # the only transfers of the iteration: the statistics block and two numbers for the log
        st = dict(zip(names, stats.tolist()))
        n_updates += int(st["train/n_updates"] if args.target_kl is None else st["train/epochs"])
        st["train/n_updates"] = n_updates
        print(json.dumps({"iteration": it, **st, "mean_reward": buf.rewards.mean().item(),
                          "episode_starts": int(buf.episode_starts.sum().item())}), flush=True)
    if args.time:
        runs = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.train(into, n_epochs=args.epochs, batch_size=args.batch_size, clip_range=clip_range, vf_coef=vf_coef, ent_coef=ent_coef,
                          lr=3e-4, normalize_advantage=normalize, seed=args.seed, first_epoch=epochs, stats_out=stats, **extra)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) * 1e3)
            epochs += args.epochs
        print(json.dumps({"time": "one update, host wall time, ms", "rows": E * K, "batch_size": args.batch_size, "epochs": args.epochs,
                          "clip_range_vf": args.clip_range_vf, "target_kl": args.target_kl, "normalize_advantage": normalize, "median_ms": sorted(runs)[len(runs) // 2],
                          "runs_ms": [round(x, 3) for x in runs]}), flush=True)
    for h in (trainer, opt, grad, pol, buf, env):
        h.close()


if __name__ == "__main__":
    main()
