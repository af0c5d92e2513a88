"""Cost of the rollout buffer on the device (fleet_rollout.hip) at the headline shape E = 4096, K = 192, D = 388, A = 50 (bench.py's
c3); prints one JSON line and writes it to profiles/rollout_rate_c3.json with --write.  HIP events on the stream, medians of --reps.

  gae       fleet_rollout_finish_dev against the same recurrence in torch ops on the same tensors in the same process, eager and
            replayed from a torch.cuda.graph; the results are compared bit for bit before anything is timed
  gather    fleet_rollout_gather_dev of 65 536 rows (six outputs, one launch) against ONE device-to-device copy of the same byte
            count, and against torch advanced indexing of the six arrays
  rollout   192 steps of fleet_step_dev + fleet_norm_step_dev with the buffer in the loop (observations and dones land in the rows,
            fleet_rollout_add_dev stores the rest) against the same steps without storage: the per-step cost of `add`
  --variants T:R,...   fleet_rollout.hip alone compiled with FLEET_GAE_THREADS=T, FLEET_GAE_ROWS=R into ab_variants/ (--build-variants,
            needs only hipcc) and each one's `gae` timed beside the product's in one process, alternating
  --trace-loop N       nothing timed: N rollouts of 192 steps through DeviceRolloutBuffer under a torch policy, for a
            `rocprofv3 --kernel-trace --memory-copy-trace` run around this tool; --trace-summary DIR then writes what the trace
            shows between the first and the last step kernel (profiles/rollout_trace_c3.json)
    python tools/rollout_rate.py [--reps 9] [--write]
"""
import argparse
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
E, K, D, A = 4096, 192, 388, 50


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


def torch_gae(torch, rewards, values, starts, last_values, dones, adv, ret, g, gl):
    """compute_returns_and_advantage as a user would write it in torch ops: K dependent iterations."""
    last = torch.zeros_like(last_values)
    n = rewards.shape[0]
    for t in reversed(range(n)):
        nnt = 1.0 - (dones if t == n - 1 else starts[t + 1]).float()
        nv = last_values if t == n - 1 else values[t + 1]
        delta = rewards[t] + g * nv * nnt - values[t]
        last = delta + gl * nnt * last
        adv[t] = last
    torch.add(adv, values, out=ret)


def variant_path(t, r):
    return os.path.join(ROOT, "ab_variants", f"rollout_gae_{t}x{r}.so")


def build_variants(spec):
    from fleetrl_amd import build

    os.makedirs(os.path.join(ROOT, "ab_variants"), exist_ok=True)
    for t, r in spec:
        cmd = [build.hipcc(), *build.FLAGS, f"-DFLEET_GAE_THREADS={t}", f"-DFLEET_GAE_ROWS={r}",
               os.path.join(ROOT, "fleetrl_amd", "csrc", "fleet_rollout.hip"), "-o", variant_path(t, r)]
        subprocess.run(cmd, check=True)
        print("built", variant_path(t, r))


def fill(torch, buf, seed=0):
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(seed)
    for name in ("observations", "actions", "rewards", "values", "log_probs"):
        t = getattr(buf, name)
        t.copy_(torch.randn(t.shape, device="cuda:0", generator=gen))
    buf.episode_starts.copy_((torch.rand((K, E), device="cuda:0", generator=gen) < 1 / 192).to(torch.uint8))
    lv = torch.randn(E, device="cuda:0", generator=gen)
    dn = (torch.rand(E, device="cuda:0", generator=gen) < 0.5).to(torch.uint8)
    return lv, dn


def measure_gae(torch, buf, reps, variants):
    lv, dn = fill(torch, buf)
    g, gl = float(np.float32(buf.gamma)), float(np.float32(buf.gamma * buf.gae_lambda))
    adv, ret = torch.empty_like(buf.advantages), torch.empty_like(buf.returns)
    args = (torch, buf.rewards, buf.values, buf.episode_starts, lv, dn, adv, ret, g, gl)
    buf.compute_returns_and_advantage(lv, dn)
    torch_gae(*args)
    torch.cuda.synchronize()
    res = {"torch_eager_bit_identical": bool(torch.equal(adv, buf.advantages) and torch.equal(ret, buf.returns))}
    fn = lambda: buf.finish_dev(lv.data_ptr(), dn.data_ptr())  # noqa: E731
    for _ in range(5):
        fn()
    res["kernel_us"], res["kernel_runs"] = event_us(torch, fn, reps, inner=20)
    res["torch_eager_us"], res["torch_eager_runs"] = event_us(torch, lambda: torch_gae(*args), reps)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch_gae(*args)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        torch_gae(*args)
    adv.zero_()
    graph.replay()
    torch.cuda.synchronize()
    res["torch_graph_bit_identical"] = bool(torch.equal(adv, buf.advantages))
    res["torch_graph_us"], res["torch_graph_runs"] = event_us(torch, graph.replay, reps)
    res["kernel_again_us"], res["kernel_again_runs"] = event_us(torch, fn, reps, inner=20)
    res["speedup_vs_torch_eager"] = res["torch_eager_us"] / res["kernel_us"]
    res["speedup_vs_torch_graph"] = res["torch_graph_us"] / res["kernel_us"]
    res["bytes"] = K * E * (4 + 4 + 1 + 4 + 4) + E * 5
    if variants:
        from fleetrl_amd import _capi

        want = buf.advantages.clone()
        stream = torch.cuda.current_stream().cuda_stream
        p = _capi.FleetRolloutParams(C.sizeof(_capi.FleetRolloutParams), E, K, 1, 1, 0, buf.gamma, buf.gae_lambda)
        runs = {}
        handles = []
        for t, r in variants:
            lib = C.CDLL(variant_path(t, r))
            vp = C.c_void_p
            lib.fleet_rollout_create.argtypes = [C.c_int, C.POINTER(_capi.FleetRolloutParams), C.POINTER(vp)]
            lib.fleet_rollout_set_stream.argtypes = [vp, vp]
            lib.fleet_rollout_arrays.argtypes = [vp, C.POINTER(_capi.FleetRolloutArrays)]
            lib.fleet_rollout_finish_dev.argtypes = [vp, vp, vp]
            lib.fleet_rollout_destroy.argtypes = [vp]
            h = vp()
            assert lib.fleet_rollout_create(0, C.byref(p), C.byref(h)) == 0
            assert lib.fleet_rollout_set_stream(h, stream) == 0
            arr = _capi.FleetRolloutArrays()
            lib.fleet_rollout_arrays(h, C.byref(arr))
            from fleetrl_amd._handle import _DeviceArray

            view = lambda ptr, ts: torch.as_tensor(_DeviceArray(ptr, (K, E), ts, None), device=torch.device("cuda", 0))  # noqa: E731
            view(arr.rewards, "<f4").copy_(buf.rewards)
            view(arr.values, "<f4").copy_(buf.values)
            view(arr.episode_starts, "|u1").copy_(buf.episode_starts)
            run = lambda lib=lib, h=h: lib.fleet_rollout_finish_dev(h, lv.data_ptr(), dn.data_ptr())  # noqa: E731
            run()
            torch.cuda.synchronize()
            got = view(arr.advantages, "<f4").clone()
            handles.append((f"{t}x{r}", run, bool(torch.equal(got, want)), lib, h))
        handles.append(("product", fn, True, None, None))
        for rnd in range(3):  # alternating
            for name, run, ok, _, _ in handles:
                for _ in range(3):
                    run()
                us, _ = event_us(torch, run, reps, inner=20)
                runs.setdefault(name, {"bit_identical": ok, "us": []})["us"].append(round(us, 2))
        for name, _, _, lib, h in handles:
            if lib is not None:
                lib.fleet_rollout_destroy(h)
        res["variants_threads_x_rows"] = runs
    return res


def measure_gather(torch, buf, reps, B=65536):
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    buf.pos, buf.full = K, True
    idx = torch.randperm(K * E, device="cuda:0", dtype=torch.int32, generator=gen)[:B].contiguous()
    out = buf.gather(idx)
    e, t = (idx // K).long(), (idx % K).long()
    arrays = (buf.observations, buf.actions, buf.values, buf.log_probs, buf.advantages, buf.returns)
    ref = [a[t, e] for a in arrays]
    torch.cuda.synchronize()
    res = {"rows": B, "bit_identical_to_torch_indexing": bool(all(torch.equal(o, r) for o, r in zip(out, ref)))}
    ptrs = [o.data_ptr() for o in out]
    fn = lambda: buf.gather_dev(idx.data_ptr(), B, *ptrs)  # noqa: E731
    for _ in range(5):
        fn()
    res["kernel_us"], res["kernel_runs"] = event_us(torch, fn, reps, inner=10)
    nbytes = B * (D + A + 4) * 4
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0"), torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    cp = lambda: dst.copy_(src)  # noqa: E731
    for _ in range(5):
        cp()
    res["memcpy_same_bytes_us"], res["memcpy_same_bytes_runs"] = event_us(torch, cp, reps, inner=10)

    def indexing():
        for a, o in zip(arrays, out):
            o.copy_(a[t, e])

    for _ in range(3):
        indexing()
    res["torch_indexing_us"], res["torch_indexing_runs"] = event_us(torch, indexing, reps, inner=3)
    res["bytes_out"] = nbytes
    res["bytes_moved"] = 2 * nbytes + 4 * B
    res["GBps_moved"] = res["bytes_moved"] / res["kernel_us"] / 1e3
    res["ratio_to_memcpy"] = res["kernel_us"] / res["memcpy_same_bytes_us"]
    res["speedup_vs_torch_indexing"] = res["torch_indexing_us"] / res["kernel_us"]
    buf.check_errors()
    return res


def measure_rollout(torch, buf, reps):
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
    nrew = torch.empty_like(g.reward)
    value, logp = torch.randn(E, device=dev), torch.randn(E, device=dev)
    spare_obs, spare_done = torch.empty((E, D), device=dev), torch.empty(E, device=dev, dtype=torch.uint8)
    slots = [buf.slot_dev(t) for t in range(K)]
    g.batch.reset_dev(g.obs.data_ptr())

    def rollout(store):
        for t in range(K):
            if store:
                nobs, ndone = (slots[t + 1].obs, slots[t + 1].episode_start) if t + 1 < K else (spare_obs.data_ptr(), spare_done.data_ptr())
            else:
                nobs, ndone = spare_obs.data_ptr(), spare_done.data_ptr()
            g.batch.step_dev(g.tape[t % g.L].data_ptr(), g.obs.data_ptr(), g.reward.data_ptr(), ndone)
            norm.step_dev(g.obs.data_ptr(), g.reward.data_ptr(), ndone, None, nobs, nrew.data_ptr(), None)
            if store:
                s = slots[t]
                buf.add_dev(t, s.obs, g.tape[t % g.L].data_ptr(), nrew.data_ptr(), _capi.ACT_F64, s.episode_start, value.data_ptr(),
                            logp.data_ptr())

    res = {}
    for _ in range(2):
        rollout(True), rollout(False)
    for key, store in (("without_storage", False), ("with_buffer", True), ("without_storage", False), ("with_buffer", True)):
        us, runs = event_us(torch, lambda: rollout(store), reps)
        res.setdefault(key + "_runs_us_per_step", []).extend(round(v / K, 2) for v in runs)
    for key in ("without_storage", "with_buffer"):
        res[key + "_us_per_step"] = float(np.median(res[key + "_runs_us_per_step"]))
    res["add_us_per_step"] = res["with_buffer_us_per_step"] - res["without_storage_us_per_step"]
    tape0 = g.tape[0].data_ptr()
    s = slots[3]
    add_only = lambda: buf.add_dev(3, s.obs, tape0, nrew.data_ptr(), _capi.ACT_F64, s.episode_start, value.data_ptr(), logp.data_ptr())  # noqa: E731
    res["add_alone_us"], res["add_alone_runs"] = event_us(torch, add_only, reps, inner=50)
    add_copy = lambda: buf.add_dev(3, spare_obs.data_ptr(), tape0, nrew.data_ptr(), _capi.ACT_F64, spare_done.data_ptr(), value.data_ptr(), logp.data_ptr())  # noqa: E731
    res["add_with_obs_copy_us"], res["add_with_obs_copy_runs"] = event_us(torch, add_copy, reps, inner=50)
    norm.close()
    g.batch.close()
    return res


def trace_loop(torch, n):
    """n rollouts of K steps of FleetVecNormalize(FleetVecEnv) through DeviceRolloutBuffer under a small torch policy, GAE and one
    epoch of minibatch gathers included; one synchronise at the very end."""
    from bench import bench_config
    from fleetrl_amd import DeviceRolloutBuffer, FleetVecEnv, FleetVecNormalize
    from fleetrl_amd.synth import synth_tables

    dev = torch.device("cuda", 0)
    env = FleetVecNormalize(FleetVecEnv(bench_config(E, A, "ct"), E, tables=synth_tables("ct", A), seed=5), clip_reward=10.0)
    buf = DeviceRolloutBuffer(E, K, D, A)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    w, wv = torch.randn((D, A), device=dev, generator=gen) / D ** 0.5, torch.randn(D, device=dev, generator=gen) / D
    carry_obs, carry_start = torch.empty((E, D), device=dev), torch.ones(E, device=dev, dtype=torch.uint8)
    rew = torch.empty(E, device=dev, dtype=torch.float64)
    env.reset_torch(obs_out=carry_obs)
    torch.cuda.synchronize()
    for _ in range(n):
        buf.reset()
        obs, start = carry_obs, carry_start
        for t in range(K):
            act = torch.tanh(obs @ w)
            value, logp = obs @ wv, -0.5 * (act * act).sum(1)
            nxt = buf.slot(t + 1) if t + 1 < K else None
            nobs, ndone = (nxt.obs, nxt.episode_start) if nxt else (carry_obs, carry_start)
            env.step_torch(act, obs_out=nobs, reward_out=rew, done_out=ndone)
            buf.add(obs, act, rew, start, value, logp)
            obs, start = nobs, ndone
        buf.compute_returns_and_advantage(obs @ wv, start)
        for b in buf.get(65536):
            b.advantages.sum()
    torch.cuda.synchronize()
    buf.check_errors()
    buf.close()
    env.close()


def trace_summary(out_dir):
    """What a rocprofv3 --kernel-trace --memory-copy-trace run of --trace-loop shows between the first and the last step kernel."""
    import csv

    def rows(pattern):
        files = glob.glob(os.path.join(out_dir, "**", pattern), recursive=True)
        return [r for f in files for r in csv.DictReader(open(f))]

    kt, mc = rows("*kernel_trace.csv"), rows("*memory_copy_trace.csv")
    steps = [r for r in kt if "fleet_step_kernel" in r["Kernel_Name"]]
    t0, t1 = min(int(r["Start_Timestamp"]) for r in steps), max(int(r["End_Timestamp"]) for r in steps)
    inside = [r for r in kt if t0 <= int(r["Start_Timestamp"]) <= t1]
    names = {}
    for r in inside:
        n = r["Kernel_Name"].replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "").split("(")[0][:60]
        k = names.setdefault(n, {"calls": 0, "ns": 0})
        k["calls"] += 1
        k["ns"] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    copies = {}
    for r in mc:
        if t0 <= int(r["Start_Timestamp"]) <= t1:
            copies[r.get("Direction", "?")] = copies.get(r.get("Direction", "?"), 0) + 1
    all_copies = {}
    for r in mc:
        all_copies[r.get("Direction", "?")] = all_copies.get(r.get("Direction", "?"), 0) + 1
    res = {"shape": {"envs": E, "steps": K, "obs_dim": D, "act_dim": A}, "step_kernels": len(steps), "span_ms": (t1 - t0) / 1e6,
           "kernels_between_first_and_last_step": {n: {"calls": k["calls"], "avg_us": round(k["ns"] / k["calls"] / 1e3, 2)}
                                                   for n, k in sorted(names.items(), key=lambda kv: -kv[1]["ns"])},
           "memory_copies_between_first_and_last_step": copies, "memory_copies_in_the_whole_process": all_copies,
           "device_to_host_copies_between_first_and_last_step": sum(v for d, v in copies.items() if "DEVICE_TO_HOST" in d.upper())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--variants", default="")
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--trace-loop", type=int, default=0)
    ap.add_argument("--trace-summary", default="")
    ap.add_argument("--only", default="gae,gather,rollout")
    args = ap.parse_args()
    variants = [tuple(int(x) for x in v.split(":")) for v in args.variants.split(",") if v]
    if args.build_variants:
        build_variants(variants)
        return
    if args.trace_summary:
        res = trace_summary(args.trace_summary)
        print(json.dumps(res))
        if args.write:
            with open(os.path.join(ROOT, "profiles", "rollout_trace_c3.json"), "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")
        return
    import torch

    if args.trace_loop:
        trace_loop(torch, args.trace_loop)
        return
    from fleetrl_amd import DeviceRolloutBuffer

    buf = DeviceRolloutBuffer(E, K, D, A)
    buf.use_torch_stream()
    res = {"envs": E, "n_steps": K, "obs_dim": D, "act_dim": A, "reps": args.reps}
    only = args.only.split(",")
    if "gae" in only:
        res["gae"] = measure_gae(torch, buf, args.reps, variants)
    if "gather" in only:
        res["gather"] = measure_gather(torch, buf, args.reps)
    if "rollout" in only:
        res["rollout"] = measure_rollout(torch, buf, args.reps)
    buf.close()
    print(json.dumps(res))
    if args.write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "rollout_rate_c3.json"), "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
