"""Cost of SAC's actor and entropy-coefficient gradients on the device (fleet_td3.hip: sac_actor_rows, sac_weights) for D = 388, A = 50,
twin critics, ReLU, with 256-256 and 64-64 trunks at B = 256; prints one JSON line and writes it to profiles/sac_grad_rate.json with
--write.  The method is tools/td3_grad_rate.py's (its helpers are imported): HIP events on torch's stream around 50 back-to-back calls,
the median of --reps alternated rounds, every round reported.

The arms: (a) the two launches of `DeviceSACGrad.actor_grad` with a learned entropy coefficient; (b) torch's sequence on the same
networks -- SB3's `actor.action_log_prob`, the entropy-coefficient loss, min over both critics, the actor loss and the two backward
passes, without the optimisers -- eager and replayed from a `torch.cuda.graph` capture (null, with the reason, where the capture of a
backward pass is refused).  Both arms use the same given noise.  No number is gated: the kernels are untuned.

    python tools/sac_grad_rate.py [--reps 9] [--write]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from td3_grad_rate import mlp, timed  # noqa: E402

D, A, B = 388, 50, 256
TRUNKS = {"64-64": (64, 64), "256-256": (256, 256)}


def measure(torch, trunk, reps):
    from torch import nn

    from fleetrl_amd import DeviceSACGrad, DeviceSACNetworks

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    hidden = TRUNKS[trunk]
    actor = mlp(torch, (D,) + hidden + (2 * A,)).to(dev)  # the last layer: the mu rows, then the log_std rows
    q1, q2 = mlp(torch, (D + A,) + hidden + (1,)).to(dev), mlp(torch, (D + A,) + hidden + (1,)).to(dev)
    linear = lambda net: [(m.weight, m.bias) for m in net if isinstance(m, nn.Linear)]  # noqa: E731
    pa = [p for pair in linear(actor) for p in pair]
    pc = [p for net in (q1, q2) for pair in linear(net) for p in pair]
    nets = DeviceSACNetworks(linear(actor), [linear(q1), linear(q2)], activation="relu")
    g = DeviceSACGrad(nets, B)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    obs = torch.randn((B, D), device=dev, generator=gen)
    eps = torch.randn((B, A), device=dev, generator=gen)
    log_alpha = torch.full((1,), -1.0, device=dev, requires_grad=True)
    alpha = log_alpha.detach().exp()
    target_entropy = -float(A)

    def sequence():
        for p in pa + pc + [log_alpha]:
            p.grad = None
        out = actor(obs)
        mean, log_std = out[:, :A], out[:, A:].clamp(-20.0, 2.0)
        std = log_std.exp()
        u = mean + std * eps
        a = torch.tanh(u)
        log_prob = (torch.distributions.Normal(mean, std, validate_args=False).log_prob(u).sum(1) - torch.log(1 - a ** 2 + 1e-6).sum(1)).reshape(-1, 1)
        ent_loss = -(log_alpha * (log_prob + target_entropy).detach()).mean()
        ent_loss.backward()
        x = torch.cat([obs, a], dim=1)
        loss = (alpha * log_prob - torch.min(q1(x), q2(x))).mean()
        loss.backward()
        return loss

    sequence()
    want = [p.grad.clone() for p in pa] + [log_alpha.grad.clone()]
    for p in pa + pc + [log_alpha]:
        p.grad = None
    stats_out = torch.empty(8, device=dev)
    call = lambda: g.actor_grad(obs, ent_coef=alpha, seed=1, step=0, into=pa, log_ent_coef=log_alpha, target_entropy=target_entropy,  # noqa: E731
                                noise=eps, noise_given=True, stats_out=stats_out)
    call()
    diff = max(float((p.grad - w).abs().max()) for p, w in zip(pa + [log_alpha], want))
    kernel_grads = [p.grad for p in pa + [log_alpha]]

    def launch():
        for p, k in zip(pa + [log_alpha], kernel_grads):
            p.grad = k
        call()

    res = {"actor_parameters": int(sum(p.numel() for p in pa)), "critic_parameters": int(sum(p.numel() for p in pc)),
           "scratch_bytes": g.describe()["scratch_bytes"], "rows_workgroups": -(-B // g.tile_rows), "max_abs_grad_diff_to_autograd": diff}
    res.update(timed(torch, g, launch, sequence, reps))
    g.close()
    nets.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    import torch

    out = {"D": D, "A": A, "B": B, "activation": "relu", "n_critics": 2, "learned_ent_coef": True, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "trunks": {name: measure(torch, name, args.reps) for name in TRUNKS}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "sac_grad_rate.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
