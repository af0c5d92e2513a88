"""Cost of the replay buffer on the device (fleet_replay.hip) at the headline shape E = 4096, D = 388, A = 50 (bench.py's c3) with
R = 244 rows (a buffer of 1e6 transitions); prints one JSON line and writes it to profiles/replay_rate_c3.json with --write.  HIP
events on torch's stream, medians of --reps.

  sample    fleet_replay_sample_dev at B = 256, 4096 and 65 536 (five outputs, normalised, one launch) against ONE device-to-device
            copy of the bytes the sample writes, and against the same result in torch ops (advanced indexing of the five arrays at
            the drawn indices plus the normalisation expressions in float64); the two results are compared bit for bit first
  add       fleet_replay_add_dev back to back against ONE device-to-device copy of the bytes it moves, and inside 192 steps of
            fleet_step_dev + fleet_norm_step_dev against the same steps without storage
    python tools/replay_rate.py [--reps 9] [--write]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
E, R, D, A, K = 4096, 244, 388, 50, 192


def event_us(torch, fn, reps, inner=1):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / inner)
    return float(np.median(out)), [round(v, 2) for v in out]


def fill(torch, buf, norm, seed=0):
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(seed)
    for name in ("observations", "next_observations", "actions", "rewards"):
        t = getattr(buf, name)
        t.copy_(torch.randn(t.shape, device="cuda:0", generator=gen) * 3)
    buf.dones.copy_((torch.rand((R, E), device="cuda:0", generator=gen) < 1 / 192).to(torch.uint8))
    buf.set_position(0, True, 0)
    for _ in range(3):  # statistics that are not the initial ones
        norm.step_torch(torch.randn((E, D), device="cuda:0", generator=gen) * 3, torch.randn(E, device="cuda:0", generator=gen, dtype=torch.float64),
                        torch.zeros(E, device="cuda:0", dtype=torch.uint8))


def torch_sample(torch, buf, rows, envs, mean, sd, ret_sd, clip_obs, clip_reward):
    """SB3's _get_samples as a user would write it in torch ops on the device."""
    def nobs(x):
        return ((x.double() - mean) / sd).clamp(-clip_obs, clip_obs).float()

    r, e = rows.long(), envs.long()
    return (nobs(buf.observations[r, e]), buf.actions[r, e], nobs(buf.next_observations[r, e]),
            (buf.dones[r, e].float() * (1 - buf.timeouts[r, e].float())).reshape(-1, 1),
            (buf.rewards[r, e].double() / ret_sd).clamp(-clip_reward, clip_reward).float().reshape(-1, 1))


def measure_sample(torch, buf, norm, reps):
    st, s = norm.get_state(), norm.settings
    dev = torch.device("cuda", 0)
    mean = torch.from_numpy(st.obs_rms.mean).to(dev)
    sd = torch.from_numpy(np.sqrt(st.obs_rms.var + s.epsilon)).to(dev)
    ret_sd = float(np.sqrt(float(st.ret_rms.var) + s.epsilon))
    res = {}
    for B in (256, 4096, 65536):
        rows, envs = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
        buf.set_position(0, True, 0)
        got = buf.sample(B, env=norm, indices_out=(rows, envs))
        want = torch_sample(torch, buf, rows, envs, mean, sd, ret_sd, s.clip_obs, s.clip_reward)
        torch.cuda.synchronize()
        r = {"torch_ops_bit_identical": bool(all(torch.equal(g.view(torch.int32), w.contiguous().view(torch.int32)) for g, w in zip(got, want)))}
        ptrs = [t.data_ptr() for t in got]
        fn = lambda: buf.sample_dev(B, norm, *ptrs)  # noqa: E731
        raw = lambda: buf.sample_dev(B, None, *ptrs)  # noqa: E731
        for _ in range(5):
            fn(), raw()
        nbytes = B * (2 * D + A + 2) * 4
        src, dst = torch.empty(nbytes, device=dev, dtype=torch.uint8), torch.empty(nbytes, device=dev, dtype=torch.uint8)
        copy = lambda: dst.copy_(src)  # noqa: E731
        r["bytes_written"] = nbytes
        r["kernel_us"], r["kernel_runs"] = event_us(torch, fn, reps, inner=20)
        r["kernel_raw_us"], r["kernel_raw_runs"] = event_us(torch, raw, reps, inner=20)
        r["copy_us"], r["copy_runs"] = event_us(torch, copy, reps, inner=20)
        r["torch_ops_us"], r["torch_ops_runs"] = event_us(torch, lambda: torch_sample(torch, buf, rows, envs, mean, sd, ret_sd, s.clip_obs, s.clip_reward), reps, inner=5)
        r["kernel_again_us"], _ = event_us(torch, fn, reps, inner=20)
        r["kernel_over_copy"] = r["kernel_us"] / r["copy_us"]
        r["torch_ops_over_kernel"] = r["torch_ops_us"] / r["kernel_us"]
        res[f"B{B}"] = r
    buf.check_errors()
    return res


def measure_add(torch, buf, reps):
    from bench import CONFIGS, Group
    from fleetrl_amd import _capi
    from fleetrl_amd.vec_normalize import DeviceNormalizer

    spec = CONFIGS["c3"]
    dev = torch.device("cuda", 0)
    g = Group(torch, dev, spec["groups"][0], E, spec["evs"], spec, 0, 0, 16, 1)
    assert g.batch.obs_dim == D and spec["evs"] == A
    g.batch.use_torch_stream(dev)
    norm = DeviceNormalizer(E, D)
    norm.use_torch_stream(dev)
    buf.use_torch_stream()
    nobs, nrew = torch.empty((E, D), device=dev), torch.empty_like(g.reward)
    prev, term = torch.empty((E, D), device=dev), torch.zeros((E, D), device=dev)
    done = torch.zeros(E, device=dev, dtype=torch.uint8)
    g.batch.reset_dev(g.obs.data_ptr())

    def steps(store):
        for t in range(K):
            g.batch.step_dev(g.tape[t % g.L].data_ptr(), g.obs.data_ptr(), g.reward.data_ptr(), done.data_ptr())
            norm.step_dev(g.obs.data_ptr(), g.reward.data_ptr(), done.data_ptr(), None, nobs.data_ptr(), nrew.data_ptr(), None)
            if store:  # the raw step outputs, as SB3's off-policy loop stores them
                buf.add_dev(prev.data_ptr(), g.obs.data_ptr(), g.tape[t % g.L].data_ptr(), g.reward.data_ptr(), _capi.ACT_F64,
                            done.data_ptr(), term.data_ptr(), None)

    res = {}
    for _ in range(2):
        steps(True), steps(False)
    for key, store in (("without_storage", False), ("with_buffer", True), ("without_storage", False), ("with_buffer", True)):
        _, runs = event_us(torch, lambda: steps(store), reps)
        res.setdefault(key + "_runs_us_per_step", []).extend(round(v / K, 2) for v in runs)
    for key in ("without_storage", "with_buffer"):
        res[key + "_us_per_step"] = float(np.median(res[key + "_runs_us_per_step"]))
    res["add_us_per_step"] = res["with_buffer_us_per_step"] - res["without_storage_us_per_step"]
    tape0 = g.tape[0].data_ptr()
    add_only = lambda: buf.add_dev(prev.data_ptr(), g.obs.data_ptr(), tape0, g.reward.data_ptr(), _capi.ACT_F64, done.data_ptr(),  # noqa: E731
                                   term.data_ptr(), None)
    res["add_alone_us"], res["add_alone_runs"] = event_us(torch, add_only, reps, inner=50)
    nbytes = E * (2 * D + A + 1) * 4 + 2 * E  # what one add writes (and reads as many)
    src, dst = torch.empty(nbytes, device=dev, dtype=torch.uint8), torch.empty(nbytes, device=dev, dtype=torch.uint8)
    res["bytes_written"] = nbytes
    res["copy_us"], res["copy_runs"] = event_us(torch, lambda: dst.copy_(src), reps, inner=50)
    res["add_over_copy"] = res["add_alone_us"] / res["copy_us"]
    norm.close()
    g.batch.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--skip-add", action="store_true")
    args = ap.parse_args()
    import torch

    from fleetrl_amd import DeviceNormalizer, DeviceReplayBuffer

    buf = DeviceReplayBuffer(R * E, E, D, A, seed=1)
    norm = DeviceNormalizer(E, D)
    fill(torch, buf, norm)
    out = {"shape": {"E": E, "R": R, "D": D, "A": A}, "reps": args.reps, "device": torch.cuda.get_device_name(0),
           "sample": measure_sample(torch, buf, norm, args.reps)}
    if not args.skip_add:
        out["add"] = measure_add(torch, buf, args.reps)
    norm.close()
    buf.close()
    line = json.dumps(out)
    print(line)
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "replay_rate_c3.json"), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
