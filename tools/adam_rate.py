"""Cost of the optimiser step on the device (fleet_adam.hip) for D = 388, A = 50 with 64-64 and 400-300 trunks; prints one JSON line and
writes it to profiles/adam_rate.json with --write.  HIP events on torch's stream around 50 back-to-back calls, medians of --reps
rounds, the arms interleaved in one process (the method of tools/td3_grad_rate.py).

Two spans: "ppo" -- both heads of a DevicePolicy and log_std, clipped at 0.5 (SB3's PPO) -- and "td3_critic" -- the two critics of a
DeviceTD3Target, not clipped (SB3's TD3 does not clip).  Per span, the arms: (a) `DeviceAdam.step`; (b) the sequence it replaces,
`clip_grad_norm_` (ppo) + `torch.optim.Adam.step()` + the image's `load_torch`, eager with torch's default Adam; (c) that sequence
with `fused=True`; (d) that sequence replayed from a `torch.cuda.graph` capture with `capturable=True` (null, with the reason, where
the capture is refused).  Every arm has parameters, gradients and an image of its own; the gradients stay what they were drawn as
(clip_grad_norm_ scales its arm's in place, once, below the threshold).  The bar: (a) must beat (b) by more than (b)'s own spread
between rounds, else the verdict says LOSS.  (c) and (d) are reported with no bar.

    python tools/adam_rate.py [--reps 9] [--write]
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
MAX_GRAD_NORM = 0.5


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


def mlp(torch, sizes, act):
    from torch import nn

    mods = []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        mods.append(nn.Linear(a, b))
        if i < len(sizes) - 2:
            mods.append(act())
    return nn.Sequential(*mods)


def captured(torch, image, sequence):
    """`sequence` as a torch.cuda.graph replay, or (None, the reason).  The image launches on the stream the capture runs on from
    before the capture begins: changing streams waits for the old one, which a capture does not allow."""
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                sequence()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        image.set_stream(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            sequence()
        torch.cuda.synchronize()
        return graph.replay, None
    except Exception as exc:  # the comparison arm only: recorded, not hidden
        torch.cuda.synchronize()
        return None, f"{type(exc).__name__}: {exc}"[:300]


def make_span(torch, span, hidden, dev):
    """(image, the span's parameters in DeviceAdam's order, all of the image's parameters in load_torch's order, nets argument)."""
    from torch import nn

    from fleetrl_amd import DevicePolicy, DeviceTD3Target

    linear = lambda net: [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]  # noqa: E731
    flat = lambda nets: [p for net in nets for pair in linear(net) for p in pair]  # noqa: E731
    if span == "ppo":
        pi, vf = mlp(torch, (D,) + hidden + (A,), nn.Tanh).to(dev), mlp(torch, (D,) + hidden + (1,), nn.Tanh).to(dev)
        log_std = nn.Parameter(torch.zeros(A, device=dev))
        image = DevicePolicy(linear(pi), critic_layers=linear(vf), activation="tanh", output="clip")
        return image, flat((pi, vf)) + [log_std], flat((pi, vf)), None
    actor = mlp(torch, (D,) + hidden + (A,), nn.ReLU).to(dev)
    q1, q2 = mlp(torch, (D + A,) + hidden + (1,), nn.ReLU).to(dev), mlp(torch, (D + A,) + hidden + (1,), nn.ReLU).to(dev)
    image = DeviceTD3Target(linear(actor), [linear(q1), linear(q2)], activation="relu", output="tanh")
    return image, flat((q1, q2)), flat((actor, q1, q2)), "critic"


def measure(torch, span, trunk, reps):
    from torch import nn

    from fleetrl_amd import DeviceAdam

    dev = torch.device("cuda", 0)
    clip = MAX_GRAD_NORM if span == "ppo" else None
    lr, eps = 3e-4, (1e-5 if span == "ppo" else 1e-8)
    arms, keep, graph_error = {}, [], None
    res = {}
    for arm in ("kernel", "torch_eager", "torch_fused", "torch_graph"):
        torch.manual_seed(0)
        image, params, image_params, nets = make_span(torch, span, TRUNKS[trunk], dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        total = sum(p.numel() for p in params)
        for p in params:  # a norm of about 2: above the threshold
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * (2.0 / total ** 0.5)
        keep.append((image, params))
        if arm == "kernel":
            opt = DeviceAdam(image, params, nets=nets, lr=lr, eps=eps, max_grad_norm=clip)
            keep.append(opt)
            d = opt.describe()
            res.update({"parameters": d["n_elements"], "tensors": d["n_tensors"], "state_bytes": d["state_bytes"],
                        "norm_workgroups": -(-d["n_elements"] // d["norm_chunk"]) if clip else 0, "launches": 2 if clip else 1})
            arms[arm] = opt.step
            if not clip:  # the norm launch as well, for its own sake (norm_out): the two launches of a clipped step
                norm_out = torch.empty(1, device=dev)
                arms["kernel_with_norm"] = lambda opt=opt, norm_out=norm_out: opt.step(norm_out=norm_out)
            continue
        kw = {"torch_eager": {}, "torch_fused": {"fused": True}, "torch_graph": {"capturable": True}}[arm]
        topt = torch.optim.Adam(params, lr=lr, eps=eps, **kw)

        def sequence(params=params, topt=topt, image=image, image_params=image_params):
            if clip:
                nn.utils.clip_grad_norm_(params, clip)
            topt.step()
            image.load_torch(image_params)

        if arm == "torch_graph":
            replay, graph_error = captured(torch, image, sequence)
            if replay:
                arms[arm] = replay
        else:
            arms[arm] = sequence
    res["torch_graph_error"] = graph_error
    res.update(interleaved(torch, arms, reps))
    eager = res["torch_eager_runs_us"]
    res["torch_eager_spread_us"] = max(eager) - min(eager)
    res["torch_eager_over_kernel"] = res["torch_eager_us"] / res["kernel_us"]
    res["torch_fused_over_kernel"] = res["torch_fused_us"] / res["kernel_us"]
    res["torch_graph_over_kernel"] = res["torch_graph_us"] / res["kernel_us"] if "torch_graph_us" in res else None
    res["verdict_against_eager"] = "WIN" if res["torch_eager_us"] - res["kernel_us"] > res["torch_eager_spread_us"] else "LOSS"
    torch.cuda.synchronize()
    for k in keep[::-1]:
        (k[0] if isinstance(k, tuple) else k).close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"D": D, "A": A, "reps": args.reps, "device": torch.cuda.get_device_name(0), "max_grad_norm": {"ppo": MAX_GRAD_NORM, "td3_critic": None},
           "spans": {span: {trunk: measure(torch, span, trunk, args.reps) for trunk in TRUNKS} for span in ("ppo", "td3_critic")}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "adam_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
