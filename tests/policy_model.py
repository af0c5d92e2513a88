"""The policy forward of fleetrl_amd/csrc/fleet_policy.hip in NumPy float64 from the float32 weights, the same chain in torch-CPU
float32 (the arithmetic stable-baselines3 itself would run), the networks and inputs the GPU tests use, state dicts of the three
SB3 families, and SB3 2.3.2's evaluate_policy loop restated line by line.  Shared by tests/test_policy_cpu.py and
tests/test_policy_gpu.py; nothing here needs a GPU."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_lmd_arbitrage_policy.npz")


# ---- the forward -------------------------------------------------------------------------------------------------------------------
def forward64(layers, x, activation, output, low=-1.0, high=1.0) -> np.ndarray:
    """float64 arithmetic on the float32 weights and inputs, nothing rounded on the way."""
    y = np.asarray(x, dtype=np.float64)
    for i, (w, b) in enumerate(layers):
        y = y @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
        if i < len(layers) - 1:
            y = np.tanh(y) if activation == "tanh" else np.maximum(y, 0.0)
    if output == "clip":
        y = np.clip(y, low, high)
    elif output == "tanh":
        y = np.tanh(y)
    return y


def forward_torch32(layers, x, activation, output, low=-1.0, high=1.0) -> np.ndarray:
    """The same chain as torch-CPU float32 `nn.Linear` modules."""
    import torch
    from torch import nn

    mods = []
    for i, (w, b) in enumerate(layers):
        lin = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.asarray(w, dtype=np.float32)))
            lin.bias.copy_(torch.from_numpy(np.asarray(b, dtype=np.float32)))
        mods.append(lin)
        if i < len(layers) - 1:
            mods.append(nn.Tanh() if activation == "tanh" else nn.ReLU())
    with torch.no_grad():
        y = nn.Sequential(*mods)(torch.from_numpy(np.array(x, dtype=np.float32)))
        if output == "clip":
            y = y.clamp(low, high)
        elif output == "tanh":
            y = torch.tanh(y)
    return y.numpy()


def norm_obs32(x, mean, var, clip_obs, epsilon) -> np.ndarray:
    """fleet_norm_obs1: (float)clip(((double)x - mean) / sqrt(var + epsilon), +-clip_obs)."""
    z = (np.asarray(x, dtype=np.float64) - mean) / np.sqrt(np.asarray(var, dtype=np.float64) + epsilon)
    return np.clip(z, -clip_obs, clip_obs).astype(np.float32)


# ---- the networks and inputs of the GPU tests ---------------------------------------------------------------------------------------
def random_layers(rng, sizes) -> list:
    """torch's default nn.Linear initialisation: U(-1/sqrt(in), 1/sqrt(in)) for weights and biases."""
    out = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        k = 1.0 / np.sqrt(i)
        out.append((rng.uniform(-k, k, (o, i)).astype(np.float32), rng.uniform(-k, k, o).astype(np.float32)))
    return out


def fixture_arrays() -> dict:
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def fixture_layers():
    z = fixture_arrays()
    actor = [(z[f"mlp_extractor.policy_net.{n}.weight"], z[f"mlp_extractor.policy_net.{n}.bias"]) for n in (0, 2)]
    critic = [(z[f"mlp_extractor.value_net.{n}.weight"], z[f"mlp_extractor.value_net.{n}.bias"]) for n in (0, 2)]
    return actor + [(z["action_net.weight"], z["action_net.bias"])], critic + [(z["value_net.weight"], z["value_net.bias"])]


# name -> (sizes, activation, output); "fixture" is the shipped agent with its critic
NETWORKS = {
    "fixture": ((45, 64, 64, 1), "tanh", "clip"),
    "388-64-64-50": ((388, 64, 64, 50), "tanh", "clip"),
    "388-400-300-50": ((388, 400, 300, 50), "relu", "tanh"),
    "1-1": ((1, 1), "tanh", "clip"),
    "3-1-2": ((3, 1, 2), "relu", "none"),
    "45-63-65-1": ((45, 63, 65, 1), "tanh", "clip"),
    "389-512-512-3": ((389, 512, 512, 3), "relu", "clip"),
    "one-layer-17-5": ((17, 5), "tanh", "tanh"),
    "four-layers-20-33-130-70-4": ((20, 33, 130, 70, 4), "tanh", "none"),
}


@functools.lru_cache(maxsize=None)
def network(name):
    """(actor layers, critic layers or None, activation, output)."""
    sizes, activation, output = NETWORKS[name]
    if name == "fixture":
        actor, critic = fixture_layers()
        return actor, critic, activation, output
    return random_layers(np.random.default_rng(sorted(NETWORKS).index(name) + 100), sizes), None, activation, output


def batch_sizes(tile_rows: int) -> list:
    """Around the tile height T: 1, 2, T-1, T, T+1, 4T-1, 4T, 4T+1, 16T+1 (1, 2, 15, 16, 17, 63, 64, 65, 257 for T = 16)."""
    T = tile_rows
    return sorted({1, 2, T - 1, T, T + 1, 4 * T - 1, 4 * T, 4 * T + 1, 16 * T + 1})


@functools.lru_cache(maxsize=None)
def inputs(name, E) -> np.ndarray:
    """Standard normal x 3 clipped to +-10; from 7 rows on, row 5 is all zero and row 6 all +-10."""
    D = NETWORKS[name][0][0]
    rng = np.random.default_rng(1000 * sorted(NETWORKS).index(name) + E)
    x = np.clip(rng.standard_normal((E, D)) * 3, -10, 10).astype(np.float32)
    if E >= 7:
        x[5] = 0.0
        x[6] = np.where(rng.random(D) < 0.5, -10.0, 10.0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(name, E):
    """[(float64 model, eps_ref)] per head: eps_ref = max |torch-CPU float32 - float64 model|."""
    actor, critic, activation, output = network(name)
    x = inputs(name, E)
    out = []
    for layers, o in ((actor, output),) + (((critic, "none"),) if critic else ()):
        y64 = forward64(layers, x, activation, o)
        y32 = forward_torch32(layers, x, activation, o)
        out.append((y64, float(np.max(np.abs(y32.astype(np.float64) - y64)))))
    return out


# ---- state dicts of the three SB3 families ------------------------------------------------------------------------------------------
def ppo_state_dict(actor, critic) -> dict:
    sd = {"log_std": np.zeros(actor[-1][0].shape[0], np.float32)}
    for net, head, layers in (("policy_net", "action_net", actor), ("value_net", "value_net", critic)):
        for i, (w, b) in enumerate(layers[:-1]):
            sd[f"mlp_extractor.{net}.{2 * i}.weight"], sd[f"mlp_extractor.{net}.{2 * i}.bias"] = w, b
        sd[f"{head}.weight"], sd[f"{head}.bias"] = layers[-1]
    return sd


def td3_state_dict(actor, qf) -> dict:
    sd = {}
    for prefix in ("actor.mu", "actor_target.mu"):
        for i, (w, b) in enumerate(actor):
            sd[f"{prefix}.{2 * i}.weight"], sd[f"{prefix}.{2 * i}.bias"] = w, b
    for prefix in ("critic.qf0", "critic.qf1", "critic_target.qf0", "critic_target.qf1"):
        for i, (w, b) in enumerate(qf):
            sd[f"{prefix}.{2 * i}.weight"], sd[f"{prefix}.{2 * i}.bias"] = w, b
    return sd


def sac_state_dict(actor, qf) -> dict:
    sd = {}
    for i, (w, b) in enumerate(actor[:-1]):
        sd[f"actor.latent_pi.{2 * i}.weight"], sd[f"actor.latent_pi.{2 * i}.bias"] = w, b
    sd["actor.mu.weight"], sd["actor.mu.bias"] = actor[-1]
    sd["actor.log_std.weight"], sd["actor.log_std.bias"] = actor[-1][0] * 0, actor[-1][1] * 0
    for prefix in ("critic.qf0", "critic_target.qf0"):
        for i, (w, b) in enumerate(qf):
            sd[f"{prefix}.{2 * i}.weight"], sd[f"{prefix}.{2 * i}.bias"] = w, b
    return sd


# ---- stable-baselines3 2.3.2 common/evaluation.py::evaluate_policy, an env without Monitor, no callback, no threshold -----------------
def sb3_evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False):
    n_envs = env.num_envs
    episode_rewards = []
    episode_lengths = []
    episode_counts = np.zeros(n_envs, dtype="int")
    # Divides episodes among different sub environments in the vector as evenly as possible
    episode_count_targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")
    current_rewards = np.zeros(n_envs)
    current_lengths = np.zeros(n_envs, dtype="int")
    observations = env.reset()
    states = None
    episode_starts = np.ones((env.num_envs,), dtype=bool)
    while (episode_counts < episode_count_targets).any():
        actions, states = model.predict(observations, state=states, episode_start=episode_starts, deterministic=deterministic)
        new_observations, rewards, dones, infos = env.step(actions)
        current_rewards += rewards
        current_lengths += 1
        for i in range(n_envs):
            if episode_counts[i] < episode_count_targets[i]:
                done = dones[i]
                episode_starts[i] = done
                if dones[i]:
                    episode_rewards.append(current_rewards[i])
                    episode_lengths.append(current_lengths[i])
                    episode_counts[i] += 1
                    current_rewards[i] = 0
                    current_lengths[i] = 0
        observations = new_observations
    mean_reward = np.mean(episode_rewards)
    std_reward = np.std(episode_rewards)
    if return_episode_rewards:
        return episode_rewards, episode_lengths
    return mean_reward, std_reward
