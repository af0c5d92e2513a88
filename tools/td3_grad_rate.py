"""Cost of TD3's critic and actor minibatch gradients on the device (fleet_td3.hip) for D = 388, A = 50 with 64-64 and 400-300 ReLU
trunks, at B = 256 and B = 4096; prints one JSON line and writes it to profiles/td3_grad_rate.json with --write.  HIP events on
torch's stream around 50 back-to-back calls, medians of --reps rounds, the arms interleaved in one process (the method of
tools/ppo_grad_rate.py).

Per entry, the arms: (a) the two launches of `DeviceTD3Grad.critic_grad` / `.actor_grad`; (b) torch's sequence on the same networks
(examples/td3_device_targets.py's losses and backward passes without the optimisers), eager and replayed from a `torch.cuda.graph`
capture (null, with the reason, where the capture of a backward pass is refused).  `load_torch`, the launch that refreshes the image
after an optimiser step, is timed on its own.  No number is gated.

    python tools/td3_grad_rate.py [--reps 9] [--write]
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


def mlp(torch, sizes, last=None):
    from torch import nn

    mods = []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(a, b))
        if i < len(sizes) - 2:
            mods.append(nn.ReLU())
    return nn.Sequential(*mods, *([last] if last else []))


def captured(torch, sequence):
    """`sequence` as a torch.cuda.graph replay, or (None, the reason)."""
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
        return graph.replay, None
    except Exception as exc:  # the comparison arm only: recorded, not hidden
        torch.cuda.synchronize()
        return None, f"{type(exc).__name__}: {exc}"[:300]


def timed(torch, g, launch, sequence, reps):
    arms = {"kernel": launch, "torch_eager": sequence}
    replay, graph_error = captured(torch, sequence)
    if replay:
        arms["torch_graph"] = replay
    g.use_torch_stream()
    r = {"torch_graph_error": graph_error}
    r.update(interleaved(torch, arms, reps))
    r["torch_eager_over_kernel"] = r["torch_eager_us"] / r["kernel_us"]
    r["torch_graph_over_kernel"] = r["torch_graph_us"] / r["kernel_us"] if "torch_graph_us" in r else None
    return r


def measure(torch, trunk, reps):
    from torch import nn

    from fleetrl_amd import DeviceTD3Grad, DeviceTD3Target

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    hidden = TRUNKS[trunk]
    actor = mlp(torch, (D,) + hidden + (A,), last=nn.Tanh()).to(dev)
    q1, q2 = mlp(torch, (D + A,) + hidden + (1,)).to(dev), mlp(torch, (D + A,) + hidden + (1,)).to(dev)
    linear = lambda net: [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]  # noqa: E731
    pa = [p for pair in linear(actor) for p in pair]
    pc = [p for net in (q1, q2) for pair in linear(net) for p in pair]
    nets = DeviceTD3Target(linear(actor), [linear(q1), linear(q2)], activation="relu", output="tanh")
    g = DeviceTD3Grad(nets, max(BATCHES))
    res = {"actor_parameters": int(sum(p.numel() for p in pa)), "critic_parameters": int(sum(p.numel() for p in pc)),
           "scratch_bytes": g.describe()["scratch_bytes"], "batches": {}}
    res["load_torch"] = interleaved(torch, {"load_torch": lambda: nets.load_torch(pa + pc)}, reps)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    for B in BATCHES:
        obs = torch.randn((B, D), device=dev, generator=gen)
        actions = torch.rand((B, A), device=dev, generator=gen) * 2 - 1
        target_q = torch.randn((B, 1), device=dev, generator=gen)

        def critic_sequence():
            for p in pc:
                p.grad = None
            x = torch.cat([obs, actions], dim=1)
            loss = nn.functional.mse_loss(q1(x), target_q) + nn.functional.mse_loss(q2(x), target_q)
            loss.backward()
            return loss

        def actor_sequence():
            for p in pa + pc:  # (SB3 zeroes the actor's only; the critics' gradients of this pass are discarded either way)
                p.grad = None
            loss = -q1(torch.cat([obs, actor(obs)], dim=1)).mean()
            loss.backward()
            return loss

        r = {"rows_workgroups": {"critic": 2 * -(-B // g.tile_rows), "actor": -(-B // g.tile_rows)}}
        for entry, params, sequence in (("critic", pc, critic_sequence), ("actor", pa, actor_sequence)):
            sequence()
            want = [p.grad.clone() for p in params]
            for p in pa + pc:
                p.grad = None
            stats_out = torch.empty(8, device=dev)
            if entry == "critic":
                call = lambda params=params, stats_out=stats_out: g.critic_grad((obs, actions), target_q, into=params, stats_out=stats_out)  # noqa: E731
            else:
                call = lambda params=params, stats_out=stats_out: g.actor_grad(obs, into=params, stats_out=stats_out)  # noqa: E731
            call()
            diff = max(float((p.grad - w).abs().max()) for p, w in zip(params, want))
            kernel_grads = [p.grad for p in params]

            def launch(params=params, kernel_grads=kernel_grads, call=call):
                for p, k in zip(params, kernel_grads):
                    p.grad = k
                call()

            e = {"max_abs_grad_diff_to_autograd": diff}
            e.update(timed(torch, g, launch, sequence, reps))
            r[entry] = e
        res["batches"][str(B)] = r
    g.close()
    nets.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"D": D, "A": A, "activation": "relu", "n_critics": 2, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "trunks": {name: measure(torch, name, args.reps) for name in TRUNKS}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "td3_grad_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
