"""Wall time of one SAC update of 64 gradient steps (fleet_sactrain.hip) and the time of its Polyak launch, for ReLU trunks 64-64 and
256-256, D = 388, A = 50, B = 256, twin critics, a learned entropy coefficient, on a replay ring of 64 envs x 256 rows; prints one JSON
line and writes it to profiles/sac_train_rate.json with --write.

(a) Two arms, each with networks, images, a gradient handle, three optimisers and a replay buffer of its own (the same contents),
alternating --reps times in one process after a warm-up update; host wall time from the first enqueue to the end of the final
synchronisation, medians reported:
  one_call     `DeviceSACTrain.train(gradient_steps=64)`
  python_loop  64 times `DeviceReplayBuffer.sample` and `fleetrl_amd.sac.gradient_step`: the path without the one call
(b) The Polyak launch on its own, HIP events around 50 back-to-back calls, the arms alternating --reps times, medians:
  image        `DeviceSACTrain.polyak`: the targets' image from the online image, one contiguous stream
  tensor_walk  `DeviceSACNetworks.polyak(online parameters)`: fleet_qtarget_polyak_dev, torch's tensors re-laid through a pointer array
A kernel trace of this tool (rocprofv3 --kernel-trace --stats, in a run of its own) gives the kernels' own durations: DESIGN.md 7x.

    python tools/sac_train_rate.py [--reps 7] [--trunks 64-64,256-256] [--write]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, A, E, R, B, G = 388, 50, 64, 256, 256, 64
TRUNKS = ((64, 64), (256, 256))
GAMMA, TAU, LR, SEED, TARGET_SEED = 0.99, 0.005, 3e-4, 0x5AC7A1, 0x7A26E7


def mlp(torch, sizes):
    from torch import nn

    mods = []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(a, b))
        if i < len(sizes) - 2:
            mods.append(nn.ReLU())
    return nn.Sequential(*mods)


class Arm:
    """Everything one SAC agent needs, from seed 0: two arms start from the same bits."""

    def __init__(self, torch, hidden, dev):
        from torch import nn

        from fleetrl_amd import DeviceAdam, DeviceReplayBuffer, DeviceSACGrad, DeviceSACNetworks, DeviceSACTrain

        torch.manual_seed(0)
        actor = mlp(torch, (D, *hidden, 2 * A)).to(dev)  # the last layer: the ONE [2A, H] pair (mu rows, then log_std rows)
        with torch.no_grad():
            actor[-1].bias[A:] -= 1.0
        q = [mlp(torch, (D + A, *hidden, 1)).to(dev) for _ in range(2)]
        linear = lambda net: [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]  # noqa: E731
        make = lambda: DeviceSACNetworks(linear(actor), [linear(q[0]), linear(q[1])], activation="relu")  # noqa: E731
        self.targets, self.nets = make(), make()
        self.actor_params, self.critic_params = list(actor.parameters()), [*q[0].parameters(), *q[1].parameters()]
        self.online = [*self.actor_params, *self.critic_params]
        self.log_alpha = torch.zeros(1, device=dev, requires_grad=True)
        self.grad = DeviceSACGrad(self.nets, B)
        self.opt_a = DeviceAdam(self.nets, self.actor_params, nets="actor", lr=LR)
        self.opt_c = DeviceAdam(self.nets, self.critic_params, nets="critic", lr=LR)
        self.opt_e = DeviceAdam(self.nets, [self.log_alpha], nets="none", lr=LR)
        self.buf = DeviceReplayBuffer(R * E, E, D, A, seed=1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(2)
        rnd = lambda *shape: torch.randn(shape, device=dev, generator=gen)  # noqa: E731
        self.buf.observations.copy_(rnd(R, E, D))
        self.buf.next_observations.copy_(rnd(R, E, D))
        self.buf.actions.copy_(rnd(R, E, A).clamp(-1, 1))
        self.buf.rewards.copy_(rnd(R, E))
        self.buf.dones.copy_((torch.rand((R, E), device=dev, generator=gen) < 0.01).to(torch.uint8))
        self.buf.set_position(0, True, 0)
        self.update = DeviceSACTrain(self.buf, self.targets, self.grad, self.opt_a, self.opt_c, self.opt_e, max_steps=G)
        self.stats = torch.empty(16, device=dev, dtype=torch.float64)
        self.critic_stats, self.actor_stats, self.alpha = torch.zeros(8, device=dev), torch.zeros(8, device=dev), torch.ones(1, device=dev)
        self.updates = 0

    def one_call(self):
        self.update.train(self.actor_params, self.critic_params, gradient_steps=G, batch_size=B, gamma=GAMMA, tau=TAU, lr=LR, seed=SEED,
                          target_seed=TARGET_SEED, first_update=self.updates, log_ent_coef=self.log_alpha, stats_out=self.stats)
        self.updates += G

    def python_loop(self):
        from fleetrl_amd.sac import gradient_step

        for _ in range(G):
            b = self.buf.sample(B)
            gradient_step(self.nets, self.targets, self.grad, self.opt_a, self.opt_c, b, self.actor_params, self.critic_params, gamma=GAMMA,
                          tau=TAU, seed=SEED, target_seed=TARGET_SEED, step=self.updates, log_ent_coef=self.log_alpha, ent_adam=self.opt_e,
                          alpha_out=self.alpha, critic_stats_out=self.critic_stats, actor_stats_out=self.actor_stats)
            self.updates += 1

    def close(self):
        for h in (self.update, self.opt_e, self.opt_a, self.opt_c, self.grad, self.nets, self.targets, self.buf):
            h.close()


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


def alternate(arms: dict, reps: int, timer) -> dict:
    runs = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            runs[k].append(timer(fn))
    return runs


def verdict(runs: dict, new: str, old: str) -> dict:
    """Medians; `new` WINS when it is faster than `old` by more than the larger of the two arms' spreads; inside it: a TIE."""
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = max(max(runs[k]) - min(runs[k]) for k in (new, old))
    return {"spread": spread, "verdict": "WIN" if med[old] - med[new] > spread else ("LOSS" if med[new] - med[old] > spread else "TIE")}


def measure(torch, hidden, reps, dev):
    a, b = Arm(torch, hidden, dev), Arm(torch, hidden, dev)
    arms = {"one_call": a.one_call, "python_loop": b.python_loop}
    for fn in arms.values():  # the warm-up update: allocations, the first launches
        fn()
    torch.cuda.synchronize()
    # (the python loop's alpha is torch.exp's, the one call's the double exponential rounded once: within one ulp, so not bit-equal)
    close = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a.online, b.online))
    runs = alternate(arms, reps, lambda fn: wall_ms(torch, fn))
    scale_chunks = a.update.describe()["scale_chunks"]
    res = {"hidden": list(hidden), "image_floats": int(sum(p.numel() for p in a.online)), "gradient_steps": G,
           "scale_chunks": scale_chunks, "max_relative_weight_difference_after_warm_up": close}
    for k, v in runs.items():
        res[k + "_ms"] = float(np.median(v))
        res[k + "_runs_ms"] = [round(x, 3) for x in v]
    res["python_loop_over_one_call"] = res["python_loop_ms"] / res["one_call_ms"]
    v = verdict(runs, "one_call", "python_loop")
    res["update_spread_ms"], res["update_verdict"] = v["spread"], v["verdict"]
    from fleetrl_amd.sac_train import SAC_TRAIN_STATS

    res["statistics"] = dict(zip(SAC_TRAIN_STATS, a.stats.tolist()))
    # (b) the Polyak launch on its own
    polyak = {"image": lambda: a.update.polyak(TAU), "tensor_walk": lambda: a.targets.polyak(a.online, TAU)}
    pruns = alternate(polyak, reps, lambda fn: event_us(torch, fn))
    res["polyak_us"] = {k: float(np.median(v)) for k, v in pruns.items()}
    res["polyak_runs_us"] = {k: [round(x, 2) for x in v] for k, v in pruns.items()}
    v = verdict(pruns, "image", "tensor_walk")
    res["polyak_image_vs_tensor_walk"] = {"spread_us": v["spread"], "verdict": v["verdict"]}
    torch.cuda.synchronize()
    a.close()
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trunks", default=",".join("-".join(map(str, h)) for h in TRUNKS))
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    if args.reps < 1 or (args.write and args.reps < 7):
        ap.error("the arms alternate at least seven times for a result that is written")
    import torch

    dev = torch.device("cuda", 0)
    trunks = [tuple(int(w) for w in t.split("-")) for t in args.trunks.split(",")]
    out = {"D": D, "A": A, "batch_size": B, "gradient_steps": G, "target_update_interval": 1, "num_envs": E, "rows": R, "reps": args.reps,
           "device": torch.cuda.get_device_name(0),
           "timing": "(a) host wall time of one update, the final synchronisation included; (b) HIP events around 50 back-to-back calls; medians",
           "kernel_trace": "not measured",
           "trunks": {"-".join(map(str, h)): measure(torch, h, args.reps, dev) for h in trunks}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sac_train_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
