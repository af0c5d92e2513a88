#!/usr/bin/env python3
"""Evaluate a trained stable-baselines3 agent without stable-baselines3, on the GPU: the policy's forward pass is one launch
(DevicePolicy), the env and the frozen normaliser step on the device, and `evaluate_policy` keeps SB3's books.  Next to it the
reference's "uncontrolled charging" benchmark on a twin env built from the same seed, i.e. over the same start rows.

    python examples/evaluate_agent_device.py [MODEL.zip] [--envs 64] [--episodes 64] [--normalize STATS.npz]

Without MODEL.zip the weights of the reference's example agent are used (tests/golden/ppo_lmd_arbitrage_policy.npz: an MlpPolicy
45 -> 64 -> 64 -> 1, trained on one last-mile-delivery vehicle with building load and PV in the observation).  STATS.npz is a
normaliser state written by `FleetVecNormalize.save`; without it the statistics are the initial ones (mean 0, variance 1), which
is not what the agent was trained with: the printed reward then shows that the pieces fit, not how good the agent is.  Inputs are
synthetic.  Needs an MI355X.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import bench_config  # noqa: E402  (the reference's config dict with the benchmark's values)
from fleetrl_amd import DevicePolicy, FleetVecEnv, FleetVecNormalize, evaluate_policy  # noqa: E402
from fleetrl_amd.policies import run_policy  # noqa: E402
from fleetrl_amd.synth import synth_tables  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model", nargs="?", help="an SB3 archive (model.save); default: the shipped agent's weights")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--normalize", help="normaliser state written by FleetVecNormalize.save")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    E, N = args.envs, 1
    if args.model:
        policy = DevicePolicy.from_sb3_zip(args.model)
    else:
        with np.load(os.path.join(ROOT, "tests", "golden", "ppo_lmd_arbitrage_policy.npz")) as z:
            policy = DevicePolicy.from_state_dict({k: z[k] for k in z.files})
    cfg, tables = bench_config(E, N, "lmd"), synth_tables("lmd", N)

    def make():
        return FleetVecEnv(cfg, E, tables=tables, seed=args.seed)

    agent_env = make()
    if agent_env.observation_space.shape[0] != policy.obs_dim or agent_env.action_space.shape[0] != policy.act_dim:
        sys.exit(f"the policy maps {policy.obs_dim} observations to {policy.act_dim} actions, the env has "
                 f"{agent_env.observation_space.shape[0]} and {agent_env.action_space.shape[0]}")
    if args.normalize:
        venv = FleetVecNormalize.load(args.normalize, agent_env)
        venv.training = False
    else:
        venv = FleetVecNormalize(agent_env, training=False)
    venv.norm_reward = False  # raw rewards: comparable with the benchmark's
    rewards, lengths = evaluate_policy(policy, venv, n_eval_episodes=args.episodes, return_episode_rewards=True)

    twin = make()  # the same seed: the same start rows, episode by episode
    twin.core.batch.reset()
    steps = int(twin.core.params.episode_steps)
    rounds = -(-args.episodes // E)
    _, reward_sum, done_count = run_policy(twin.core.batch, "uncontrolled", steps * rounds)
    print(f"policy {policy.describe()['heads'][0]['widths']} on {E} envs: {len(rewards)} episodes of {lengths[0]} steps")
    print(f"agent         mean episode reward {np.mean(rewards):12.4f}  (std {np.std(rewards):.4f})")
    print(f"uncontrolled  mean episode reward {reward_sum.sum() / max(int(done_count.sum()), 1):12.4f}  ({int(done_count.sum())} episodes)")
    policy.close()
    venv.close()
    twin.close()


if __name__ == "__main__":
    main()
