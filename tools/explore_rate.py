"""Cost of sampling exploration actions on the device (fleet_explore_act_dev, fleet_policy.hip) at E = 4096 for 388-64-64-50 tanh
with its critic (bench.py's c3 widths) and 45-64-64-1 tanh with its critic (the reference's shipped agent); prints one JSON line
and writes it to profiles/explore_rate_c3.json with --write.  The method of tools/policy_rate.py: HIP events on torch's stream around
back-to-back calls, medians of --reps, the arms interleaved in one process.  Arms:
  sample          fleet_explore_act_dev, GAUSSIAN, with log-prob and values
  forward         the deterministic fleet_policy_forward_dev with values: the yardstick for what the epilogue adds
  torch_eager     what examples/ppo_device_loop.py runs per rollout step: dist, sample, the critic, log_prob, clamp
  torch_graph     the same sequence replayed from a `torch.cuda.graph` capture
Both torch arms write the distribution's arithmetic out in tensor ops (randn_like, mean + std * eps, Normal.log_prob's expression):
`torch.distributions.Normal` validates its arguments and `torch.normal` checks std >= 0 by reading a device flag on the host,
which a capture refuses and which would put host round trips into the eager arm's back-to-back loop.  Without them the torch arms
time torch's launches alone, which favours torch.  No number is gated.

    python tools/explore_rate.py [--reps 9] [--write]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from policy_rate import event_us, random_layers  # noqa: E402

E = 4096
NETWORKS = {"388-64-64-50-tanh": (388, 64, 64, 50), "45-64-64-1-tanh": (45, 64, 64, 1)}


def torch_mlp(torch, layers, dev):
    from torch import nn

    mods = []
    for i, (w, b) in enumerate(layers):
        lin = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w)), lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if i < len(layers) - 1:
            mods.append(nn.Tanh())
    return nn.Sequential(*mods).to(dev).requires_grad_(False)


def measure(torch, name, reps):
    from fleetrl_amd import DevicePolicy, _capi

    sizes = NETWORKS[name]
    D, A = sizes[0], sizes[-1]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    actor, critic = random_layers(rng, sizes), random_layers(rng, sizes[:-1] + (1,))
    pol = DevicePolicy(actor, critic_layers=critic, activation="tanh", output="clip")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    obs = torch.randn((E, D), device=dev, generator=gen)
    log_std = torch.full((A,), -0.5, device=dev)
    act, env_act, det = (torch.empty((E, A), device=dev) for _ in range(3))
    logp, val = torch.empty(E, device=dev), torch.empty((E, 1), device=dev)
    pi, vf = torch_mlp(torch, actor, dev), torch_mlp(torch, critic, dev)

    def eager():  # examples/ppo_device_loop.py, the rollout's policy step
        mean, std = pi(obs), log_std.exp()
        a = mean + std * torch.randn_like(mean)  # Normal(mean, std).sample()
        logp = (-((a - mean) ** 2) / (2 * std ** 2) - log_std - 0.9189385332046727).sum(-1)  # .log_prob(a).sum(-1)
        return a, vf(obs), logp, a.clamp(-1, 1)

    with torch.no_grad():
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                eager()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eager()
        pol.use_torch_stream()
        args = _capi.FleetExploreArgs()
        args.mode, args.noise_mode, args.seed, args.scale = _capi.EXPLORE_GAUSSIAN, _capi.EXPLORE_NOISE_DRAW, 7, log_std.data_ptr()
        args.actions, args.env_actions, args.log_prob, args.values = act.data_ptr(), env_act.data_ptr(), logp.data_ptr(), val.data_ptr()
        optr, dptr, vptr = obs.data_ptr(), det.data_ptr(), val.data_ptr()
        step = [0]

        def sample():
            args.step = step[0]
            step[0] += 1
            pol.explore_dev(optr, E, None, args)

        arms = {"sample": sample, "forward": lambda: pol.forward_dev(optr, E, None, dptr, vptr), "torch_eager": eager,
                "torch_graph": graph.replay}
        for fn in arms.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        res = {}
        runs = {k: [] for k in arms}
        for _ in range(reps):  # interleaved rounds
            for k, fn in arms.items():
                runs[k].extend(event_us(torch, fn, 1, inner=50))
    for k, v in runs.items():
        res[k + "_us"] = float(np.median(v))
        res[k + "_runs_us"] = [round(x, 2) for x in v]
    res["sample_minus_forward_us"] = res["sample_us"] - res["forward_us"]
    res["sample_over_torch_eager"] = res["sample_us"] / res["torch_eager_us"]
    res["sample_over_torch_graph"] = res["sample_us"] / res["torch_graph_us"]
    pol.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"E": E, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "networks": {name: measure(torch, name, args.reps) for name in NETWORKS}}
    line = json.dumps(out)
    print(line)
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "explore_rate_c3.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
