"""Cost of the correlated noise processes (fleet_noise_next_dev, fleet_noise.hip) at E = 4096, A = 50, n = 192 -- the reference's
TD3 recipe at the benchmark's batch -- beside the exploration step they feed; prints one JSON line and writes it to
profiles/noise_rate.json with --write.  The method of tools/explore_rate.py: HIP events on torch's stream, medians of --reps, the arms
interleaved in one process.  Arms, microseconds per call:
  pink_ordinary    `next` when no env takes a new sequence (back-to-back calls inside one sequence)
  pink_all         `next` when every env does (done = 1 everywhere: the phase-locked episode boundary); one call per event pair
  pink_staggered   `next` when 1 / n of the envs do (done flags staggered over the batch, a different 1 / n every call)
  ou               `next` of the Ornstein-Uhlenbeck process
  explore_uniform  fleet_explore_act_dev UNIFORM at the same shape: the yardstick for one small launch
  explore_white    fleet_explore_act_dev ACTION_NOISE drawing white noise (388-64-64-50 actor)
  explore_given    the same with the noise given: what runs behind `next` with action_noise=
pink_amortised_us = pink_ordinary + (pink_all - pink_ordinary) / n: the per-step cost over a phase-locked episode.  No number is gated.

    python tools/noise_rate.py [--reps 9] [--write]
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

E, A, N, D = 4096, 50, 192, 388


def measure(torch, reps):
    from fleetrl_amd import DeviceOUNoise, DevicePinkNoise, DevicePolicy, _capi

    dev = torch.device("cuda", 0)
    pol = DevicePolicy(random_layers(np.random.default_rng(0), (D, 64, 64, A)), activation="relu", output="tanh")
    pink, ou = DevicePinkNoise(E, A, N, seed=7), DeviceOUNoise(E, A, sigma=0.5, seed=7)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    obs = torch.randn((E, D), device=dev, generator=gen)
    sigma = torch.full((A,), 0.1, device=dev)
    eps, act = torch.empty((E, A), device=dev), torch.empty((E, A), device=dev)
    ones = torch.ones(E, device=dev, dtype=torch.uint8)
    stagger = torch.zeros((N, E), device=dev, dtype=torch.uint8)
    stagger[torch.arange(E, device=dev) % N, torch.arange(E, device=dev)] = 1  # call c: the envs with e % n == c
    for h in (pol, pink, ou):
        h.use_torch_stream()
    args = _capi.FleetExploreArgs()
    args.seed, args.scale, args.noise_lo, args.noise_hi = 7, sigma.data_ptr(), -1.0, 1.0
    args.actions, args.env_actions = act.data_ptr(), act.data_ptr()
    step = [0]

    def explore(mode, noise_mode, noise=None):
        def fn():
            args.mode, args.noise_mode, args.noise, args.step = mode, noise_mode, noise, step[0]
            step[0] += 1
            pol.explore_dev(obs.data_ptr(), E, None, args)
        return fn

    eptr, optr = eps.data_ptr(), ones.data_ptr()
    calls = [0]

    def staggered():
        pink.next_dev(stagger[calls[0] % N].data_ptr(), eptr)
        calls[0] += 1

    def ordinary():  # 50 calls from position 0: no env reaches the end of its sequence inside the timed loop
        pink.next_dev(None, eptr)

    arms = {"pink_ordinary": (ordinary, 50), "pink_all": (lambda: pink.next_dev(optr, eptr), 1), "pink_staggered": (staggered, 48),
            "ou": (lambda: ou.next_dev(None, eptr), 50),
            "explore_uniform": (explore(_capi.EXPLORE_UNIFORM, _capi.EXPLORE_NOISE_DRAW), 50),
            "explore_white": (explore(_capi.EXPLORE_ACTION_NOISE, _capi.EXPLORE_NOISE_DRAW), 50),
            "explore_given": (explore(_capi.EXPLORE_ACTION_NOISE, _capi.EXPLORE_NOISE_GIVEN, eptr), 50)}
    for fn, _ in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in arms}
    for _ in range(reps):  # interleaved rounds
        for k, (fn, inner) in arms.items():
            if k == "pink_ordinary":
                pink.reset()  # position 0 everywhere (outside the timed window)
                torch.cuda.synchronize()
            runs[k].extend(event_us(torch, fn, 1, inner=inner))
    res = {}
    for k, v in runs.items():
        res[k + "_us"] = float(np.median(v))
        res[k + "_runs_us"] = [round(x, 2) for x in v]
    res["pink_amortised_us"] = res["pink_ordinary_us"] + (res["pink_all_us"] - res["pink_ordinary_us"]) / N
    res["pink_ordinary_over_explore_uniform"] = res["pink_ordinary_us"] / res["explore_uniform_us"]
    res["cache_bytes"] = pink.describe()["cache_bytes"]
    for h in (pol, pink, ou):
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"E": E, "A": A, "n": N, "reps": args.reps, "device": torch.cuda.get_device_name(0), **measure(torch, args.reps)}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "noise_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
