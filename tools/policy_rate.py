"""Cost of the policy forward on the device (fleet_policy.hip) at E = 4096 for three networks -- 388-64-64-50 tanh (bench.py's c3
observation and action widths), 388-400-300-50 ReLU (TD3's default actor) and 45-64-64-1 tanh (the reference's shipped agent) --
each with and without the fused normalisation; prints one JSON line and writes it to profiles/policy_rate_c3.json with --write.
HIP events on torch's stream, medians of --reps, the arms interleaved in one process.

Yardsticks: the same network in torch ops on the same device (nn.Linear chain plus the clip / tanh; with normalisation, the
float64 expression in front of it), eager and replayed from a `torch.cuda.graph` capture, and ONE device-to-device copy of the
bytes the forward reads and writes (observations in, actions out, the weights once).  The torch result is compared with the
kernel's first (max abs difference, reported).  For the two 388-column networks one more arm, `load_torch`: the re-lay launch that
copies torch's parameter tensors into the policy's image (what a training loop pays after every optimiser step).  No number is gated.

    python tools/policy_rate.py [--reps 9] [--write]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
E = 4096
NETWORKS = {"388-64-64-50-tanh": ((388, 64, 64, 50), "tanh", "clip"), "388-400-300-50-relu": ((388, 400, 300, 50), "relu", "tanh"),
            "45-64-64-1-tanh": ((45, 64, 64, 1), "tanh", "clip")}
LOAD_TORCH = ("388-64-64-50-tanh", "388-400-300-50-relu")


def event_us(torch, fn, reps, inner):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return out


def random_layers(rng, sizes):
    out = []
    for i, o in zip(sizes[:-1], sizes[1:]):
        k = 1.0 / np.sqrt(i)
        out.append((rng.uniform(-k, k, (o, i)).astype(np.float32), rng.uniform(-k, k, o).astype(np.float32)))
    return out


def torch_net(torch, layers, activation, output, dev):
    from torch import nn

    mods = []
    for i, (w, b) in enumerate(layers):
        lin = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w)), lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if i < len(layers) - 1:
            mods.append(nn.Tanh() if activation == "tanh" else nn.ReLU())
    net = nn.Sequential(*mods).to(dev).requires_grad_(False)
    return (lambda x: net(x).clamp(-1, 1)) if output == "clip" else (lambda x: torch.tanh(net(x)))


def measure(torch, name, reps):
    from fleetrl_amd import DeviceNormalizer, DevicePolicy

    sizes, activation, output = NETWORKS[name]
    D, A = sizes[0], sizes[-1]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    layers = random_layers(rng, sizes)
    pol = DevicePolicy(layers, activation=activation, output=output)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    norm = DeviceNormalizer(E, D)
    rew, done = torch.zeros(E, device=dev, dtype=torch.float64), torch.zeros(E, device=dev, dtype=torch.uint8)
    for _ in range(3):
        norm.step_torch(torch.randn((E, D), device=dev, generator=gen) * 3 + 1, rew, done)
    norm.configure(training=False)
    st, s = norm.get_state(), norm.settings
    mean = torch.from_numpy(st.obs_rms.mean).to(dev)
    sd = torch.from_numpy(np.sqrt(st.obs_rms.var + s.epsilon)).to(dev)
    raw = torch.randn((E, D), device=dev, generator=gen) * 3 + 1
    obs = ((raw.double() - mean) / sd).clamp(-s.clip_obs, s.clip_obs).float()
    out = torch.empty((E, A), device=dev)
    net = torch_net(torch, layers, activation, output, dev)
    with torch.no_grad():
        eager = lambda: net(obs)  # noqa: E731
        eager_norm = lambda: net(((raw.double() - mean) / sd).clamp(-s.clip_obs, s.clip_obs).float())  # noqa: E731
        res = {"max_abs_diff_to_torch": float((pol.act(obs) - eager()).abs().max()),
               "max_abs_diff_to_torch_fused_norm": float((pol.act(raw, normalizer=norm) - eager_norm()).abs().max())}
        graphs = {}
        side = torch.cuda.Stream()
        for key, fn in (("graph", eager), ("graph_norm", eager_norm)):
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs[key] = g
        nbytes = (E * (D + A) + sum(w.size + b.size for w, b in layers)) * 4
        src, dst = torch.empty(nbytes, device=dev, dtype=torch.uint8), torch.empty(nbytes, device=dev, dtype=torch.uint8)
        pol.use_torch_stream()
        optr, rptr, aptr = obs.data_ptr(), raw.data_ptr(), out.data_ptr()
        arms = {"kernel": lambda: pol.forward_dev(optr, E, None, aptr), "kernel_fused_norm": lambda: pol.forward_dev(rptr, E, norm, aptr),
                "torch_eager": eager, "torch_eager_norm": eager_norm, "torch_graph": graphs["graph"].replay,
                "torch_graph_norm": graphs["graph_norm"].replay, "copy": lambda: dst.copy_(src)}
        if name in LOAD_TORCH:
            params = [torch.from_numpy(a).to(dev) for w, b in layers for a in (w, b)]
            arms["load_torch"] = lambda: pol.load_torch(params)
        for fn in arms.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in arms}
        for _ in range(reps):  # interleaved rounds
            for k, fn in arms.items():
                runs[k].extend(event_us(torch, fn, 1, inner=50))
    res["bytes_read_and_written"] = nbytes
    res["fma_per_forward"] = int(E * sum(w.size for w, _ in layers))
    for k, v in runs.items():
        res[k + "_us"] = float(np.median(v))
        res[k + "_runs_us"] = [round(x, 2) for x in v]
    res["torch_eager_over_kernel"] = res["torch_eager_us"] / res["kernel_us"]
    res["torch_graph_over_kernel"] = res["torch_graph_us"] / res["kernel_us"]
    res["kernel_over_copy"] = res["kernel_us"] / res["copy_us"]
    norm.close()
    pol.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    from fleetrl_amd import DevicePolicy

    probe = DevicePolicy(random_layers(np.random.default_rng(0), (4, 2)))
    out = {"E": E, "reps": args.reps, "device": torch.cuda.get_device_name(0), "tile_rows": probe.tile_rows,
           "networks": {name: measure(torch, name, args.reps) for name in NETWORKS}}
    probe.close()
    line = json.dumps(out)
    print(line)
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "policy_rate_c3.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
