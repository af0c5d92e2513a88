"""Wall time of one TD3 update of 64 gradient steps (fleet_offpolicy.hip) and the time of its Polyak launch, for ReLU trunks 64-64 and
400-300, D = 388, A = 50, B = 256, on a replay ring of 64 envs x 256 rows; prints one JSON line and writes it to
profiles/td3_train_rate.json with --write.

(a) Two arms, each with networks, images, a gradient handle, optimisers and a replay buffer of its own (the same contents), alternating
--reps times in one process; host wall time from the first enqueue to the end of the final synchronisation, medians reported:
  one_call     `DeviceTD3Train.train(gradient_steps=64)`
  python_loop  the inner loop of examples/td3_device_adam.py, 64 times: `sample`, `target`, `critic_grad`, `step` and on every second
               update `actor_grad`, `step`, `DeviceTD3Target.polyak(online parameters)`
(b) The Polyak launch on its own, HIP events around 50 back-to-back calls, the arms alternating --reps times, medians:
  image        `DeviceTD3Train.polyak`: the targets' image from the online image, one contiguous stream
  tensor_walk  `DeviceTD3Target.polyak(online parameters)`: fleet_qtarget_polyak_dev, torch's tensors re-laid through a pointer array
  foreach_lerp `torch._foreach_lerp_` on plain copies of the parameters: what SB3's polyak_update amounts to
A kernel trace of this tool (rocprofv3 --kernel-trace --stats, in a run of its own) gives the kernels' own durations: DESIGN.md 7q.

    python tools/td3_train_rate.py [--reps 7] [--write]
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
TRUNKS = ((64, 64), (400, 300))
GAMMA, TAU, DELAY, NOISE_CLIP, LR, SEED = 0.99, 0.005, 2, 0.5, 1e-3, 0x7A46E7


def mlp(torch, sizes, last=None):
    from torch import nn

    mods = []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(a, b))
        if i < len(sizes) - 2:
            mods.append(nn.ReLU())
    return nn.Sequential(*mods, *([last] if last else []))


class Arm:
    """Everything one TD3 agent needs, from seed 0: two arms start from the same bits."""

    def __init__(self, torch, hidden, dev):
        from torch import nn

        from fleetrl_amd import DeviceAdam, DeviceReplayBuffer, DeviceTD3Grad, DeviceTD3Target, DeviceTD3Train

        torch.manual_seed(0)
        actor = mlp(torch, (D, *hidden, A), nn.Tanh()).to(dev)
        q = [mlp(torch, (D + A, *hidden, 1)).to(dev) for _ in range(2)]
        linear = lambda net: [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]  # noqa: E731
        make = lambda: DeviceTD3Target(linear(actor), [linear(q[0]), linear(q[1])], activation="relu", output="tanh")  # noqa: E731
        self.targets, self.nets = make(), make()
        self.actor_params, self.critic_params = list(actor.parameters()), [*q[0].parameters(), *q[1].parameters()]
        self.online = [*self.actor_params, *self.critic_params]
        self.grad = DeviceTD3Grad(self.nets, B)
        self.opt_a = DeviceAdam(self.nets, self.actor_params, nets="actor", lr=LR)
        self.opt_c = DeviceAdam(self.nets, self.critic_params, nets="critic", lr=LR)
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
        self.update = DeviceTD3Train(self.buf, self.targets, self.grad, self.opt_a, self.opt_c, max_steps=G)
        self.sigma = torch.full((A,), 0.2, device=dev)
        self.stats = torch.empty(16, device=dev, dtype=torch.float64)
        self.critic_stats, self.actor_stats = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
        self.updates = 0

    def one_call(self):
        self.update.train(self.actor_params, self.critic_params, gradient_steps=G, batch_size=B, gamma=GAMMA, tau=TAU, policy_delay=DELAY,
                          sigma=self.sigma, noise_clip=NOISE_CLIP, lr=LR, seed=SEED, first_update=self.updates, stats_out=self.stats)
        self.updates += G

    def python_loop(self):
        for _ in range(G):
            b = self.buf.sample(B)
            y = self.targets.target(b.next_observations, b.rewards, b.dones, gamma=GAMMA, sigma=self.sigma, noise_clip=NOISE_CLIP, seed=SEED,
                                    step=self.updates)
            self.grad.critic_grad(b, y, into=self.critic_params, stats_out=self.critic_stats)
            self.opt_c.step()
            self.updates += 1
            if self.updates % DELAY == 0:
                self.grad.actor_grad(b.observations, into=self.actor_params, stats_out=self.actor_stats)
                self.opt_a.step()
                self.targets.polyak(self.online, TAU)

    def close(self):
        for h in (self.update, self.opt_a, self.opt_c, self.grad, self.nets, self.targets, self.buf):
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
    """Medians; `new` WINS when it is faster than `old` by more than the larger of the two arms' spreads."""
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = max(max(runs[k]) - min(runs[k]) for k in (new, old))
    return {"spread": spread, "verdict": "WIN" if med[old] - med[new] > spread else ("LOSS" if med[new] - med[old] > spread else "TIE")}


def measure(torch, hidden, reps, dev):
    a, b = Arm(torch, hidden, dev), Arm(torch, hidden, dev)
    arms = {"one_call": a.one_call, "python_loop": b.python_loop}
    for fn in arms.values():  # warm-up: allocations, the first launches
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a.online, b.online))  # one update each from the same bits
    runs = alternate(arms, reps, lambda fn: wall_ms(torch, fn))
    delayed = G // DELAY
    res = {"hidden": list(hidden), "image_floats": int(sum(p.numel() for p in a.online)), "gradient_steps": G, "actor_steps": delayed,
           "launches_one_call": 5 * (G - delayed) + 9 * delayed + 1, "weights_bit_equal_after_warm_up": bool(same)}
    for k, v in runs.items():
        res[k + "_ms"] = float(np.median(v))
        res[k + "_runs_ms"] = [round(x, 3) for x in v]
    res["python_loop_over_one_call"] = res["python_loop_ms"] / res["one_call_ms"]
    v = verdict(runs, "one_call", "python_loop")
    res["update_spread_ms"], res["update_verdict"] = v["spread"], v["verdict"]
    res["statistics"] = dict(zip(("critic_loss", "critic_0_loss", "critic_1_loss", "actor_loss", "last_critic_loss", "last_actor_loss",
                                  "n_updates", "actor_steps"), a.stats.tolist()))
    # (b) the Polyak launch on its own
    plain_t, plain_p = [p.detach().clone() for p in a.online], [p.detach() for p in a.online]
    polyak = {"image": lambda: a.update.polyak(TAU), "tensor_walk": lambda: a.targets.polyak(a.online, TAU),
              "foreach_lerp": lambda: torch._foreach_lerp_(plain_t, plain_p, TAU)}
    pruns = alternate(polyak, reps, lambda fn: event_us(torch, fn))
    res["polyak_us"] = {k: float(np.median(v)) for k, v in pruns.items()}
    res["polyak_runs_us"] = {k: [round(x, 2) for x in v] for k, v in pruns.items()}
    for old in ("tensor_walk", "foreach_lerp"):
        v = verdict(pruns, "image", old)
        res["polyak_image_vs_" + old] = {"spread_us": v["spread"], "verdict": v["verdict"]}
    torch.cuda.synchronize()
    a.close()
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    if args.reps < 1 or (args.write and args.reps < 7):
        ap.error("the arms alternate at least seven times for a result that is written")
    import torch

    dev = torch.device("cuda", 0)
    out = {"D": D, "A": A, "batch_size": B, "gradient_steps": G, "policy_delay": DELAY, "num_envs": E, "rows": R, "reps": args.reps,
           "device": torch.cuda.get_device_name(0),
           "timing": "(a) host wall time of one update, the final synchronisation included; (b) HIP events around 50 back-to-back calls; medians",
           "trunks": {"-".join(map(str, h)): measure(torch, h, args.reps, dev) for h in TRUNKS}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "td3_train_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
