"""Cost of SAC's action and of its soft target on the device (fleet_sac.hip) for D = 388, A = 50, ReLU, twin critics: `act` at E = 4096
with 256-256 trunks (SB3's SAC default), `target` at B = 256 with 256-256 and with 64-64 trunks; prints one JSON line and writes it to
profiles/sac_rate.json (or --out) with --write.  HIP events on torch's stream around 50 back-to-back calls, medians of --reps rounds with
every round listed, the arms interleaved in one process (the method of tools/qtarget_rate.py).

Arms: (a) the one launch; (b) the same expressions in eager torch float32 tensor ops -- the trunk, the two heads as one Linear, the
clamp, exp, randn, tanh, the two log-probability sums; for the target also the cat, both critics, the min and the four closing
operations.  (torch draws its noise with randn, the launch with Philox: both pay for their generator.)  No number is gated.

    python tools/sac_rate.py [--reps 9] [--write] [--out profiles/sac_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from qtarget_rate import interleaved, random_layers, torch_net  # noqa: E402  (the same timing loop and networks)

D, A = 388, 50
TRUNKS = {"256-256": (256, 256), "64-64": (64, 64)}
ACT_E, TARGET_B = 4096, 256
GAMMA = 0.99


def squashed(torch, actor_t, obs, eps):
    out = actor_t(obs)
    mean, log_std = out[:, :A], out[:, A:].clamp(-20.0, 2.0)
    a = torch.tanh(mean + log_std.exp() * eps)
    return a, (-0.5 * eps * eps - log_std - 0.9189385332).sum(1) - torch.log(1.0 - a * a + 1e-6).sum(1)


def measure(torch, trunk, reps, with_act):
    from fleetrl_amd import DeviceSACNetworks

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    hidden = TRUNKS[trunk]
    actor = random_layers(rng, (D,) + hidden + (2 * A,))
    critics = [random_layers(rng, (D + A,) + hidden + (1,)) for _ in range(2)]
    nets, targets = DeviceSACNetworks(actor, critics), DeviceSACNetworks(actor, critics)
    actor_t, q1_t, q2_t = torch_net(torch, actor, dev), torch_net(torch, critics[0], dev), torch_net(torch, critics[1], dev)
    res = {"parameters": int(sum(w.size + b.size for net in [actor] + critics for w, b in net))}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    step = [0]
    with torch.no_grad():
        if with_act:
            E = ACT_E
            obs = torch.randn((E, D), device=dev, generator=gen)
            acts, lp, rec = torch.empty((E, A), device=dev), torch.empty(E, device=dev), torch.empty((E, A), device=dev)
            nets.act(obs, seed=7, step=0, actions_out=acts, log_prob_out=lp, noise=rec)
            want_a, want_lp = squashed(torch, actor_t, obs, rec)

            def launch():
                step[0] += 1
                nets.act(obs, seed=7, step=step[0], actions_out=acts, log_prob_out=lp)

            r = {"E": E, "workgroups": -(-E // nets.tile_rows), "max_abs_diff_actions_to_torch": float((acts - want_a).abs().max()),
                 "max_abs_diff_log_prob_to_torch": float((lp - want_lp).abs().max())}
            r.update(interleaved(torch, {"kernel": launch, "torch_eager": lambda: squashed(torch, actor_t, obs, torch.randn_like(acts))}, reps))
            r["torch_eager_over_kernel"] = r["torch_eager_us"] / r["kernel_us"]
            res["act"] = r
        B = TARGET_B
        next_obs = torch.randn((B, D), device=dev, generator=gen)
        rewards, dones = torch.randn(B, device=dev, generator=gen), (torch.rand(B, device=dev, generator=gen) < 0.1).float()
        alpha = torch.full((1,), 0.2, device=dev)
        y, rec, like = torch.empty(B, device=dev), torch.empty((B, A), device=dev), torch.empty((B, A), device=dev)

        def sequence(eps=None):
            a, lp = squashed(torch, actor_t, next_obs, torch.randn_like(like) if eps is None else eps)
            x = torch.cat([next_obs, a], dim=1)
            return rewards + (1 - dones) * GAMMA * (torch.min(q1_t(x), q2_t(x))[:, 0] - alpha * lp)

        got = nets.target(targets, next_obs, rewards, dones, gamma=GAMMA, ent_coef=alpha, seed=9, step=0, noise=rec)
        want = sequence(rec)

        def target_launch():
            step[0] += 1
            nets.target(targets, next_obs, rewards, dones, gamma=GAMMA, ent_coef=alpha, seed=9, step=step[0], out=y)

        r = {"B": B, "workgroups": -(-B // nets.tile_rows), "max_abs_diff_to_torch": float((got - want).abs().max())}
        r.update(interleaved(torch, {"kernel": target_launch, "torch_eager": sequence}, reps))
        r["torch_eager_over_kernel"] = r["torch_eager_us"] / r["kernel_us"]
        res["target"] = r
    nets.close(), targets.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac_rate.json"))
    args = ap.parse_args()
    import torch

    out = {"D": D, "A": A, "n_critics": 2, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "trunks": {name: measure(torch, name, args.reps, with_act=name == "256-256") for name in TRUNKS}}
    print(json.dumps(out))
    if args.write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
