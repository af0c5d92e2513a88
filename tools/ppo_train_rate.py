"""Wall time of one PPO update (fleet_train.hip) for 64-64 tanh trunks, D = 388, A = 50 on a rollout of 64 envs x 256 steps (n = 16384
rows), 2 epochs, batch_size 64 and 128; prints one JSON line and writes it to profiles/ppo_train_rate.json with --write.

Two arms, each with a policy, parameters, a gradient handle and an optimiser of its own on ONE shared rollout buffer, alternating
--reps times in one process; host wall time from the first enqueue to the end of the final synchronisation, medians reported:
  one_call     `DevicePPOTrain.train`: the shuffle, the gather and the normalisation on the device, five launches per minibatch
  python_loop  the loop of examples/ppo_device_adam.py: per minibatch a slice of `torch.randperm`, `DeviceRolloutBuffer.gather`, torch's
               mean / std normalisation, `DevicePPOGrad.grad` and `DeviceAdam.step`
and, for the breakdown of a minibatch of the one call, HIP events around 50 back-to-back `grad` and `step` calls on their own: what is
left of the one call's time per minibatch is the minibatch launch AND the gaps between the five dependent launches (a kernel trace
of this tool gives the kernels' own durations: DESIGN.md section 7p).

    python tools/ppo_train_rate.py [--reps 7] [--write]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, A, HIDDEN, E, K, EPOCHS = 388, 50, (64, 64), 64, 256, 2
BATCH_SIZES = (64, 128)
CLIP, VF, ENT, LR, EPS, MAXN = 0.2, 0.5, 0.0, 3e-4, 1e-5, 0.5


def mlp(torch, sizes):
    from torch import nn

    mods = []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(a, b))
        if i < len(sizes) - 2:
            mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def make_arm(torch, buf, batch_size, dev):
    from torch import nn

    from fleetrl_amd import DeviceAdam, DevicePolicy, DevicePPOGrad

    torch.manual_seed(0)
    pi, vf = mlp(torch, (D,) + HIDDEN + (A,)).to(dev), mlp(torch, (D,) + HIDDEN + (1,)).to(dev)
    linear = lambda net: [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]  # noqa: E731
    log_std = nn.Parameter(torch.zeros(A, device=dev))
    pol = DevicePolicy(linear(pi), critic_layers=linear(vf), activation="tanh", output="clip")
    into = [p for net in (pi, vf) for pair in linear(net) for p in pair] + [log_std]
    grad = DevicePPOGrad(pol, batch_size)
    opt = DeviceAdam(pol, into, lr=LR, eps=EPS, max_grad_norm=MAXN)
    return pol, into, grad, opt


def wall_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_us(torch, fn, inner=50):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def measure(torch, buf, batch_size, reps, dev):
    from fleetrl_amd import DevicePPOTrain

    n = E * K
    pol_a, into_a, grad_a, opt_a = make_arm(torch, buf, batch_size, dev)
    pol_b, into_b, grad_b, opt_b = make_arm(torch, buf, batch_size, dev)
    trainer = DevicePPOTrain(buf, grad_a, opt_a)
    stats = torch.empty(16, device=dev, dtype=torch.float64)
    epochs = [0]

    def one_call():
        trainer.train(into_a, n_epochs=EPOCHS, batch_size=batch_size, clip_range=CLIP, vf_coef=VF, ent_coef=ENT, lr=LR, seed=1,
                      first_epoch=epochs[0], stats_out=stats)
        epochs[0] += EPOCHS

    def python_loop():
        for _ in range(EPOCHS):
            for b in buf.get(batch_size):
                adv = (b.advantages - b.advantages.mean()) / (b.advantages.std() + 1e-8)
                grad_b.grad(b, into_b[-1], CLIP, VF, ENT, into=into_b, advantages=adv)
                opt_b.step()

    arms = {"one_call": one_call, "python_loop": python_loop}
    for fn in arms.values():  # warm-up: allocations, the first launches
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            runs[k].append(wall_ms(torch, fn))
    minibatches = -(-n // batch_size) * EPOCHS
    res = {"batch_size": batch_size, "minibatches": minibatches, "launches_one_call": 5 * minibatches + 1}
    for k, v in runs.items():
        res[k + "_ms"] = float(np.median(v))
        res[k + "_runs_ms"] = [round(x, 3) for x in v]
    res["python_loop_over_one_call"] = res["python_loop_ms"] / res["one_call_ms"]
    spread = max(runs["python_loop"]) - min(runs["python_loop"])
    res["python_loop_spread_ms"] = spread
    res["verdict"] = "WIN" if res["python_loop_ms"] - res["one_call_ms"] > spread else "LOSS"
    # the breakdown of one minibatch of the one call
    batch = next(iter(buf.get(batch_size)))
    grad_us = event_us(torch, lambda: grad_b.grad(batch, into_b[-1], CLIP, VF, ENT, into=into_b))
    step_us = event_us(torch, opt_b.step)
    per = res["one_call_ms"] * 1e3 / minibatches
    res["breakdown_us"] = {"per_minibatch": per, "grad_two_launches": grad_us, "step_two_launches": step_us,
                           "rest_minibatch_launch_and_gaps": per - grad_us - step_us}
    res["statistics"] = dict(zip(("policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "loss", "n_updates",
                                  "explained_variance", "std"), stats.tolist()))
    torch.cuda.synchronize()
    for h in (trainer, opt_a, grad_a, pol_a, opt_b, grad_b, pol_b):
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("the arms alternate at least five times")
    import torch

    from fleetrl_amd import DeviceRolloutBuffer

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    buf = DeviceRolloutBuffer(E, K, D, A)
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=gen)  # noqa: E731
    buf.observations.copy_(rnd(K, E, D))
    buf.actions.copy_(rnd(K, E, A))
    buf.values.copy_(rnd(K, E))
    buf.advantages.copy_(rnd(K, E))
    buf.returns.copy_(buf.values + buf.advantages)
    # log-probabilities near those of a unit Gaussian at these actions: ratios near 1, as after a rollout
    buf.log_probs.copy_((-0.5 * buf.actions ** 2 - 0.9189385332).sum(-1) + 0.05 * rnd(K, E))
    buf.pos, buf.full = K, True
    out = {"D": D, "A": A, "hidden": list(HIDDEN), "num_envs": E, "n_steps": K, "rows": E * K, "n_epochs": EPOCHS, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "timing": "host wall time of one update, the final synchronisation included; medians",
           "batch_sizes": {str(bs): measure(torch, buf, bs, args.reps, dev) for bs in BATCH_SIZES}}
    buf.close()
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ppo_train_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
