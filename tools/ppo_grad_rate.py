"""Cost of PPO's minibatch loss and gradients on the device (fleet_ppo.hip) for D = 388, A = 50 with 64-64 and 400-300 tanh trunks,
at B = 256 and B = 4096; prints one JSON line and writes it to profiles/ppo_grad_rate.json with --write.  HIP events on torch's
stream around 50 back-to-back calls, medians of --reps rounds, the arms interleaved in one process (the method of
tools/qtarget_rate.py).

Arms: (a) the two launches of `DevicePPOGrad.grad`; (b) torch's evaluate + clipped loss + backward on the same networks
(examples/ppo_device_rollout.py's update without the optimiser), eager and replayed from a `torch.cuda.graph` capture (null, with the
reason, where the capture of a backward pass is refused).  No number is gated.

    python tools/ppo_grad_rate.py [--reps 9] [--write]
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
CLIP_RANGE, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01


def event_us(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


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


def mlp(torch, sizes):
    from torch import nn

    mods = []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(a, b))
        if i < len(sizes) - 2:
            mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def measure(torch, trunk, reps):
    from torch import nn

    from fleetrl_amd import DevicePolicy, DevicePPOGrad

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    hidden = TRUNKS[trunk]
    pi, vf = mlp(torch, (D,) + hidden + (A,)).to(dev), mlp(torch, (D,) + hidden + (1,)).to(dev)
    log_std = nn.Parameter(torch.full((A,), -0.3, device=dev))
    linear = [p for net in (pi, vf) for m in net if isinstance(m, nn.Linear) for p in (m.weight, m.bias)]
    params = linear + [log_std]
    layers = lambda ps: [(ps[i], ps[i + 1]) for i in range(0, len(ps), 2)]  # noqa: E731
    n = 2 * (len(hidden) + 1)
    pol = DevicePolicy(layers(linear[:n]), critic_layers=layers(linear[n:]), activation="tanh", output="clip")
    g = DevicePPOGrad(pol, max(BATCHES))
    res = {"parameters": int(sum(p.numel() for p in params)), "scratch_bytes": g.describe()["scratch_bytes"], "batches": {}}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    for B in BATCHES:
        from collections import namedtuple

        Batch = namedtuple("Batch", ["observations", "actions", "old_log_prob", "advantages", "returns"])
        obs = torch.randn((B, D), device=dev, generator=gen)
        with torch.no_grad():
            actions = pi(obs) + log_std.exp() * torch.randn((B, A), device=dev, generator=gen)
            old = torch.distributions.Normal(pi(obs), log_std.exp()).log_prob(actions).sum(-1) + 0.9 * (torch.rand(B, device=dev, generator=gen) - 0.5)
        b = Batch(obs, actions, old, torch.randn(B, device=dev, generator=gen), torch.randn(B, device=dev, generator=gen))

        def sequence():
            for p in params:
                p.grad = None
            d = torch.distributions.Normal(pi(b.observations), log_std.exp(), validate_args=False)  # (validation reads back: no capture)
            logp, entropy = d.log_prob(b.actions).sum(-1), d.entropy().sum(-1)
            ratio = (logp - b.old_log_prob).exp()
            pl = -torch.min(b.advantages * ratio, b.advantages * ratio.clamp(1 - CLIP_RANGE, 1 + CLIP_RANGE)).mean()
            vl = nn.functional.mse_loss(b.returns, vf(b.observations).squeeze(-1))
            loss = pl + ENT_COEF * -entropy.mean() + VF_COEF * vl
            loss.backward()
            return loss

        sequence()
        want = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        stats = g.grad(b, log_std, CLIP_RANGE, VF_COEF, ENT_COEF, into=params)
        diff = max(float((p.grad - w).abs().max()) for p, w in zip(params, want))
        kernel_grads = [p.grad for p in params]
        stats_out = torch.empty_like(stats)

        def launch():
            for p, k in zip(params, kernel_grads):
                p.grad = k
            g.grad(b, log_std, CLIP_RANGE, VF_COEF, ENT_COEF, into=params, stats_out=stats_out)

        arms = {"kernel": launch, "torch_eager": sequence}
        graph_error = None
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    sequence()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                sequence()
            arms["torch_graph"] = graph.replay
        except Exception as exc:  # the comparison arm only: recorded, not hidden
            graph_error = f"{type(exc).__name__}: {exc}"[:300]
            torch.cuda.synchronize()
        g.use_torch_stream()
        r = {"max_abs_grad_diff_to_autograd": diff, "rows_workgroups": 2 * -(-B // g.tile_rows), "torch_graph_error": graph_error}
        r.update(interleaved(torch, arms, reps))
        r["torch_eager_over_kernel"] = r["torch_eager_us"] / r["kernel_us"]
        r["torch_graph_over_kernel"] = r["torch_graph_us"] / r["kernel_us"] if "torch_graph_us" in r else None
        res["batches"][str(B)] = r
    g.close()
    pol.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"D": D, "A": A, "activation": "tanh", "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "trunks": {name: measure(torch, name, args.reps) for name in TRUNKS}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ppo_grad_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
