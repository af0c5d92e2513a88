"""Cost of the TD3 learning target and of the Polyak update on the device (fleet_qtarget.hip) for D = 388, A = 50 with 64-64 and
400-300 trunks (ReLU, tanh output, twin critics), at B = 256 and B = 4096; prints one JSON line and writes it to
profiles/qtarget_rate.json with --write.  HIP events on torch's stream around 50 back-to-back calls, medians of --reps rounds, the
arms interleaved in one process (the method of tools/policy_rate.py).

Target arms: (a) the fused launch; (b) the torch sequence of examples/td3_device_loop.py -- the smoothing noise and its clamp, the
target actor, the clamp, the cat, both critics, the min, r + (1 - d) * gamma * q -- in tensor ops, eager and replayed from a
`torch.cuda.graph` capture.  (torch draws its noise with randn_like, the launch with Philox: both pay for their generator.)
Polyak arms: the launch; the per-parameter `lerp_` loop; `torch._foreach_lerp_`.  No number is gated.

    python tools/qtarget_rate.py [--reps 9] [--write]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, A = 388, 50
TRUNKS = {"64-64": (64, 64), "400-300": (400, 300)}
BATCHES = (256, 4096)
GAMMA, SIGMA, NOISE_CLIP, TAU = 0.99, 0.2, 0.5, 0.005


def event_us(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def random_layers(rng, sizes):
    out = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        k = 1.0 / np.sqrt(i)
        out.append((rng.uniform(-k, k, (o, i)).astype(np.float32), rng.uniform(-k, k, o).astype(np.float32)))
    return out


def torch_net(torch, layers, dev, last=None):
    from torch import nn

    mods = []
    for i, (w, b) in enumerate(layers):
        lin = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w)), lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if i < len(layers) - 1:
            mods.append(nn.ReLU())
    return nn.Sequential(*mods, *([last] if last else [])).to(dev).requires_grad_(False)


def interleaved(torch, arms, reps):
    for fn in arms.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            runs[k].append(event_us(torch, fn, 50))
    out = {}
    for k, v in runs.items():
        out[k + "_us"] = float(np.median(v))
        out[k + "_runs_us"] = [round(x, 2) for x in v]
    return out


def measure(torch, trunk, reps):
    from torch import nn

    from fleetrl_amd import DeviceTD3Target

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    hidden = TRUNKS[trunk]
    actor = random_layers(rng, (D,) + hidden + (A,))
    critics = [random_layers(rng, (D + A,) + hidden + (1,)) for _ in range(2)]
    tgt = DeviceTD3Target(actor, critics, activation="relu", output="tanh")
    actor_t, q1_t, q2_t = torch_net(torch, actor, dev, nn.Tanh()), torch_net(torch, critics[0], dev), torch_net(torch, critics[1], dev)
    res = {"parameters": int(sum(w.size + b.size for net in [actor] + critics for w, b in net)), "batches": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    with torch.no_grad():
        for B in BATCHES:
            next_obs = torch.randn((B, D), device=dev, generator=gen)
            rewards, dones = torch.randn(B, device=dev, generator=gen), (torch.rand(B, device=dev, generator=gen) < 0.1).float()
            like = torch.empty((B, A), device=dev)
            y = torch.empty(B, device=dev)
            sigma = torch.full((A,), SIGMA, device=dev)

            def sequence():
                noise = (SIGMA * torch.randn_like(like)).clamp(-NOISE_CLIP, NOISE_CLIP)
                next_act = (actor_t(next_obs) + noise).clamp(-1, 1)
                x = torch.cat([next_obs, next_act], dim=1)
                return rewards + (1 - dones) * GAMMA * torch.min(q1_t(x), q2_t(x))[:, 0]

            # the launch against the sequence on the noise the launch recorded (clamp order and tanhf differ in the last bits)
            rec = torch.empty((B, A), device=dev)
            got = tgt.target(next_obs, rewards, dones, gamma=GAMMA, sigma=sigma, noise_clip=NOISE_CLIP, seed=7, step=0, noise=rec)
            na = (actor_t(next_obs) + (SIGMA * rec).clamp(-NOISE_CLIP, NOISE_CLIP)).clamp(-1, 1)
            xa = torch.cat([next_obs, na], dim=1)
            want = rewards + (1 - dones) * GAMMA * torch.min(q1_t(xa), q2_t(xa))[:, 0]
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                for _ in range(3):
                    sequence()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                sequence()
            tgt.use_torch_stream()
            step = [0]

            def launch():
                step[0] += 1
                tgt.target(next_obs, rewards, dones, gamma=GAMMA, sigma=sigma, noise_clip=NOISE_CLIP, seed=7, step=step[0], out=y)

            r = {"max_abs_diff_to_torch": float((got - want).abs().max()), "workgroups": -(-B // tgt.tile_rows)}
            r.update(interleaved(torch, {"kernel": launch, "torch_eager": sequence, "torch_graph": g.replay}, reps))
            r["torch_eager_over_kernel"] = r["torch_eager_us"] / r["kernel_us"]
            r["torch_graph_over_kernel"] = r["torch_graph_us"] / r["kernel_us"]
            res["batches"][str(B)] = r
        # Polyak: the online parameters against the targets
        online = [torch.from_numpy(a).to(dev) for net in [actor] + critics for w, b in net for a in (w, b)]
        target = [t.clone() for t in online]

        def loop():
            for p, q in zip(online, target):
                q.lerp_(p, TAU)

        arms = {"kernel": lambda: tgt.polyak(online, TAU), "torch_lerp_loop": loop,
                "torch_foreach_lerp": lambda: torch._foreach_lerp_(target, online, TAU)}
        r = {"tensors": len(online)}
        r.update(interleaved(torch, arms, reps))
        r["lerp_loop_over_kernel"] = r["torch_lerp_loop_us"] / r["kernel_us"]
        r["foreach_lerp_over_kernel"] = r["torch_foreach_lerp_us"] / r["kernel_us"]
        res["polyak"] = r
    tgt.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"D": D, "A": A, "n_critics": 2, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "trunks": {name: measure(torch, name, args.reps) for name in TRUNKS}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "qtarget_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
